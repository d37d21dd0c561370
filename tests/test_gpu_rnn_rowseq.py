"""Row-owned sequence passes for narrow recurrent cores (sf_rnn_rowseq_fwd / sf_rnn_rowseq_bwd, csrc/sf_rnn_rowseq.h):
one work-group owns a tile of chunk rows for all R steps of a BPTT pass, H in {32, 64, 128}, GRU and LSTM.

Kernel level: against a float64 torch loop written from the cell equations of include/sf_hip.h, with the per-step launches
(the path these widths took before) as the yardstick of what f32 can do; bitwise independence of a row from its
neighbours; no write outside the problem; refusals.  Model level: ActorCritic with the passes on and off; a Runner run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRU, LSTM = 0, 1
WIDTHS = (32, 64, 128)  # what sf_rnn_rowseq_supported offers (every width measured faster than the per-step path)
R = 5
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def make_inputs(kind, H, Cn, seed):
    """the issue's inputs: gx, dout ~ N(0, 1); whh, bhh ~ U(+-1/sqrt(H)); chunk-start states ~ U(-1, 1); keep ~ Bernoulli(0.7)
    with chunk 0 all ones, chunk 1 all zeros and chunk 2 a single zero at t = 0 (as far as Cn has such chunks)"""
    G = 4 if kind else 3
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(s, generator=g) * 2 - 1
    x = dict(gx=torch.randn((R, Cn, G * H), generator=g), dout=torch.randn((R, Cn, H), generator=g),
             whh=u(H, G * H) / np.sqrt(H), bhh=u(G * H) / np.sqrt(H), h0=u(Cn, H), c0=u(Cn, H),
             keep=(torch.rand((R, Cn), generator=g) < 0.7).float())
    x["keep"][:, 0] = 1.0
    if Cn > 1:
        x["keep"][:, 1] = 0.0
    if Cn > 2:
        x["keep"][:, 2] = 1.0
        x["keep"][0, 2] = 0.0
    return x


def truth_fp64(kind, H, x):
    """float64 loop with autograd; gates {r, z, n, hn} / {i, f, g, o}; dgh is read off the retained h W_hh + b_hh of each step"""
    gx = x["gx"].double().requires_grad_(True)
    W, b, keep = x["whh"].double().requires_grad_(True), x["bhh"].double(), x["keep"].double()  # (so that step 0's gh has a gradient)
    h, c = x["h0"].double(), x["c0"].double()
    out = dict(gates=[], hout=[], cout=[], hprev=[h], cprev=[c])
    ghs = []
    for t in range(R):
        gh = h @ W + b
        gh.retain_grad()
        ghs.append(gh)
        if kind == GRU:
            xr, xz, xn = gx[t].split(H, dim=1)
            hr, hz, hn = gh.split(H, dim=1)
            r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
            n = torch.tanh(xn + r * hn)
            h = (1.0 - z) * n + z * h
            out["gates"].append(torch.cat([r, z, n, hn], 1))
        else:
            i_, f_, g_, o_ = (gx[t] + gh).split(H, dim=1)
            ig, fg, gg, og = torch.sigmoid(i_), torch.sigmoid(f_), torch.tanh(g_), torch.sigmoid(o_)
            c = fg * c + ig * gg
            h = og * torch.tanh(c)
            out["gates"].append(torch.cat([ig, fg, gg, og], 1))
            out["cout"].append(c)
            c = c * keep[t][:, None]
            out["cprev"].append(c)
        out["hout"].append(h)
        h = h * keep[t][:, None]
        out["hprev"].append(h)
    (torch.stack(out["hout"]) * x["dout"].double()).sum().backward()
    names = ("gates", "hout", "hprev") + (("cout", "cprev") if kind else ())
    res = {k: torch.stack([v.detach() for v in out[k]]) for k in names}
    res["dgx"] = gx.grad
    res["dgh"] = torch.stack([g_.grad for g_ in ghs])
    return res


def run_per_step(lib, kind, H, Cn, x):
    """the per-step launches of ActorCritic._rnn_sequence_fwd / _rnn_sequence_bwd, time-major"""
    from sample_factory_amd.model.actor_critic import _linear_desc
    G = 4 if kind else 3
    GH = G * H
    desc = _linear_desc(H, GH, 0)
    d = lambda t: t.cuda().contiguous()
    z = lambda *s: torch.zeros(s, device="cuda")
    gx, whh, bhh, keep, dout = d(x["gx"]), d(x["whh"]), d(x["bhh"]), d(x["keep"]), d(x["dout"])
    gates, hout, hprev = z(R, Cn, 4 * H), z(R, Cn, H), z(R + 1, Cn, H)
    cout, cprev = (z(R, Cn, H), z(R + 1, Cn, H)) if kind else (None, None)
    hprev[0] = d(x["h0"])
    if kind:
        cprev[0] = d(x["c0"])
    gh = z(Cn, GH)
    for t in range(R):
        lib.conv_fwd_raw(hprev[t], H, None, 0, whh, bhh, gh, Cn, desc)
        lib.rnn_cell_fwd(kind, gx[t], gh, hprev[t], H, cprev[t] if kind else None, H, keep[t], Cn, H, gates[t], hout[t],
                         cout[t] if kind else None, hprev[t + 1], cprev[t + 1] if kind else None)
    dgx = z(R, Cn, GH)
    dgh = z(R, Cn, GH) if kind == GRU else dgx
    dh, dhW, carry_h = z(Cn, H), z(Cn, H), z(Cn, H)
    dh_direct = z(Cn, H) if kind == GRU else None
    carry_c, dc_prev = (z(Cn, H), z(Cn, H)) if kind else (None, None)
    for t in range(R - 1, -1, -1):
        last = t == R - 1
        lib.rows_add_scale(dout[t], None if last else carry_h, None, Cn, H, dh)
        lib.rnn_cell_bwd(kind, dh, None if (last or kind == GRU) else carry_c, gates[t], hprev[t], H, cprev[t] if kind else None, H,
                         cout[t] if kind else None, Cn, H, dgx[t], dgh[t] if kind == GRU else None, dh_direct, dc_prev)
        if t > 0:
            lib.conv_dgrad(dgh[t], whh, None, dhW, Cn, desc)
            lib.rows_add_scale(dhW, dh_direct, keep[t - 1], Cn, H, carry_h)
            if kind:
                lib.rows_add_scale(dc_prev, None, keep[t - 1], Cn, H, carry_c)
    torch.cuda.synchronize()
    res = dict(gates=gates, hout=hout, hprev=hprev, dgx=dgx, dgh=dgh)
    if kind:
        res.update(cout=cout, cprev=cprev)
    return res


SENTINEL = 7.25


def run_rowseq(lib, kind, H, Cn, x, env_major=False, guard=False):
    """the two row-owned launches.  guard: every output lies in a buffer with one more time slot and 8 more rows behind it,
    filled with a sentinel; returns the outputs (time-major views, hout as the pass wrote it) and the guard regions"""
    G = 4 if kind else 3
    d = lambda t: t.cuda().contiguous()
    guards = []

    def out(slots, width):
        n = slots * Cn * width
        extra = (Cn + 8) * width if guard else 0
        buf = torch.full((n + extra,), SENTINEL, device="cuda")
        if guard:
            guards.append(buf[n:])
        return buf[:n]
    gx, whh, bhh, keep = d(x["gx"]), d(x["whh"]), d(x["bhh"]), d(x["keep"])
    gates = out(R, 4 * H).view(R, Cn, 4 * H)
    hprev = out(R + 1, H).view(R + 1, Cn, H)
    hout = out(R, H).view((Cn, R, H) if env_major else (R, Cn, H))
    cprev = out(R + 1, H).view(R + 1, Cn, H) if kind else None
    cout = out(R, H).view(R, Cn, H) if kind else None
    hprev[0] = d(x["h0"])
    if kind:
        cprev[0] = d(x["c0"])
    lib.rnn_rowseq_fwd(kind, gx, whh, bhh, keep, gates, hprev, hout, cprev, cout, R, Cn, H, env_major=env_major)
    dout = d(x["dout"].transpose(0, 1)) if env_major else d(x["dout"])
    dgx = out(R, G * H).view(R, Cn, G * H)
    dgh = out(R, G * H).view(R, Cn, G * H) if kind == GRU else None
    lib.rnn_rowseq_bwd(kind, dout, gates, hprev, cprev, cout, keep, whh, dgx, dgh, R, Cn, H, env_major=env_major)
    torch.cuda.synchronize()
    res = dict(gates=gates, hout=hout.transpose(0, 1) if env_major else hout, hprev=hprev, dgx=dgx, dgh=dgh if kind == GRU else dgx)
    if kind:
        res.update(cout=cout, cprev=cprev)
    return res, guards


_cache = {}


def case(lib, kind, H, Cn):
    """inputs, float64 truth, per-step results and row-owned results (time-major hout) of one case: computed once, shared"""
    key = (kind, H, Cn)
    if key not in _cache:
        x = make_inputs(kind, H, Cn, seed=1000 * kind + 10 * H + Cn)
        _cache[key] = (x, truth_fp64(kind, H, x), run_per_step(lib, kind, H, Cn, x), run_rowseq(lib, kind, H, Cn, x)[0])
    return _cache[key]


@pytest.mark.parametrize("env_major", [0, 1])
@pytest.mark.parametrize("Cn", [1, 37])
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_forward_and_backward_against_float64(lib, kind, H, Cn, env_major):
    """every output tensor in full (gates, all R+1 hprev / cprev slots, hout, cout, dgx, dgh) against the float64 loop: the
    row-owned pass may be at most twice as far from the truth as the per-step launches on the same inputs (two summation
    orders of equal-length f32 dot products), with a floor of 4 ulp of the tensor's largest element"""
    assert lib.rnn_rowseq_supported(kind, Cn, H)
    x, truth, step, new_tm = case(lib, kind, H, Cn)
    new = run_rowseq(lib, kind, H, Cn, x, env_major=True)[0] if env_major else new_tm
    for name in sorted(truth):
        want = truth[name]
        assert new[name].shape == want.shape == step[name].shape, name
        e_new = float((new[name].cpu().double() - want).abs().max())
        e_step = float((step[name].cpu().double() - want).abs().max())
        bound = max(2.0 * e_step, 4.0 * EPS * float(want.abs().max()))
        print(f"kind={kind} H={H} Cn={Cn} env_major={env_major} {name}: row-owned {e_new:.3e} per-step {e_step:.3e} bound {bound:.3e}")
        assert e_new <= bound, (name, e_new, e_step, bound)
    if env_major:  # the row order of hout / dout changes nothing else
        for name in new:
            assert torch.equal(new[name], new_tm[name]), name


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_a_row_does_not_depend_on_its_neighbours(lib, kind, H):
    """the 37 rows of the case above, run again behind five other rows and in reversed order (Cn = 42) and inside a batch
    of 300 (many work-groups): bit-identical outputs, forward and backward.  (Every width has one tile height — 16 rows,
    32 at H = 32 — so there is no launcher threshold to straddle; the three runs put a row into different tiles, waves and
    lanes.)"""
    x, _, _, base = case(lib, kind, H, 37)
    for Cn in (42, 300):
        big = make_inputs(kind, H, Cn, seed=77 + Cn + H)
        big["whh"], big["bhh"] = x["whh"], x["bhh"]
        where = torch.arange(5 + 36, 4, -1)  # row i of the small problem sits at row 41 - i
        for k in ("gx", "dout", "keep"):
            big[k][:, where] = x[k]
        for k in ("h0", "c0"):
            big[k][where] = x[k]
        got = run_rowseq(lib, kind, H, Cn, big)[0]
        for name, want in base.items():
            assert torch.equal(got[name][:, where.cuda()], want), (name, Cn)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_nothing_outside_the_problem_is_written(lib, kind, H):
    """the layouts are dense ([slot][Cn][width], Cn is the row count AND the row pitch), so the rows behind Cn of slot t ARE the
    first rows of slot t + 1 and cannot be guard rows.  What this test guards: one more slot and 8 more rows behind the last
    slot of every output, filled with a sentinel that must survive both passes — a ragged last tile storing past Cn in the
    last slot, or a pass walking one slot too far, lands there — and the guarded run must equal the unguarded one bit for bit
    (the guard changes nothing).  What it cannot see: a store past Cn in an INNER slot lands in the neighbouring slot of both
    runs alike; that case is covered by the float64 comparison of test_forward_and_backward_against_float64 at Cn = 1 and
    37 (ragged tiles), where the backward pass, walking the slots downwards, would leave the stray values standing."""
    for env_major in (False, True):
        x, _, _, base = case(lib, kind, H, 37)
        got, guards = run_rowseq(lib, kind, H, 37, x, env_major=env_major, guard=True)
        assert len(guards) == (6 if kind else 5)
        for gd in guards:
            assert gd.numel() > 0 and bool((gd == SENTINEL).all())
        for name, want in base.items():
            assert torch.equal(got[name], want), name


def test_refusals(lib):
    for H in WIDTHS:
        assert lib.rnn_rowseq_supported(GRU, 5, H) and lib.rnn_rowseq_supported(LSTM, 100000, H)
    assert not lib.rnn_rowseq_supported(2, 64, 64)
    for H in (16, 48, 256, 512):
        assert not lib.rnn_rowseq_supported(GRU, 64, H) and not lib.rnn_rowseq_supported(LSTM, 64, H)
    assert not lib.rnn_rowseq_supported(GRU, 0, 64)
    assert not lib.lstm_seq_supported(64, 64)
    H, Cn = 48, 8
    z = lambda *s: torch.zeros(s, device="cuda")
    outs = [torch.full(s, SENTINEL, device="cuda") for s in [(R, Cn, 4 * H), (R + 1, Cn, H), (R, Cn, H)]]
    with pytest.raises(lib.SfHipError, match="unsupported"):
        lib.rnn_rowseq_fwd(GRU, z(R, Cn, 3 * H), z(H, 3 * H), z(3 * H), z(R, Cn), outs[0], outs[1], outs[2], None, None, R, Cn, H)
    with pytest.raises(lib.SfHipError, match="unsupported"):
        lib.rnn_rowseq_bwd(GRU, z(R, Cn, H), z(R, Cn, 4 * H), z(R + 1, Cn, H), None, None, z(R, Cn), z(H, 3 * H), outs[0], outs[0],
                           R, Cn, H)
    H = 64
    with pytest.raises(lib.SfHipError, match="LSTM needs"):  # a missing operand is refused before any launch, too
        lib.rnn_rowseq_fwd(LSTM, z(R, Cn, 4 * H), z(H, 4 * H), z(4 * H), z(R, Cn), outs[0], outs[1], outs[2], None, None, R, Cn, H)
    with pytest.raises(lib.SfHipError, match="aligned"):
        lib.rnn_rowseq_fwd(GRU, z(R, Cn, 3 * H), z(H * 3 * H + 1)[1:].view(H, 3 * H), z(3 * H), z(R, Cn), outs[0], outs[1], outs[2],
                           None, None, R, Cn, H)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENTINEL).all())


@pytest.mark.parametrize("rnn_type,layers", [("gru", 2), ("lstm", 1)])
def test_model_takes_the_row_owned_passes_and_matches_the_per_step_path(lib, rnn_type, layers, monkeypatch):
    """ActorCritic on Box(24,) observations, MLP encoder [64] + GRU-64 x 2 / LSTM-64, recurrence 8, 24 chunks: the training
    forward + backward with the fused passes on (the saved dict says fused and names the row-owned family) and off; heads,
    final states, one-step new states and every parameter gradient agree within 2e-5 of the tensor's largest element (the
    bound of the width-256 fused-versus-per-step test in tests/test_gpu_nn.py)"""
    import sample_factory_amd.model.actor_critic as acm
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    cfg = default_cfg(use_rnn=True, rnn_type=rnn_type, rnn_size=64, rnn_num_layers=layers, recurrence=8, nonlinearity="tanh",
                      encoder_mlp_layers=[64], normalize_input=False, normalize_returns=False)
    cfg.dp_world = 1
    obs_space = spaces.Dict({"obs": spaces.Box(-1, 1, (24,), np.float32)})
    ac = acm.ActorCritic(cfg, obs_space, spaces.Discrete(5), "cuda")
    Rm, Cn = 8, 24
    n = Rm * Cn
    g = torch.Generator().manual_seed(11)
    obs = (torch.rand((n, 24), generator=g) * 2 - 1).cuda()
    keep = (torch.rand((Rm, Cn), generator=g) < 0.8).float().cuda()
    h0 = (torch.rand((Cn, ac.rnn_S), generator=g) * 2 - 1).cuda()
    g_heads = torch.zeros((n, ac.heads_ld), device="cuda")
    g_heads[:, :1 + ac.num_action_params] = torch.randn((n, 1 + ac.num_action_params), generator=g).cuda() / n
    st_in = (torch.rand((16, ac.rnn_S), generator=g) * 2 - 1).cuda()
    li_rnn = [i for i, L in enumerate(ac.layers) if L.role == "rnn_ih"]
    assert len(li_rnn) == layers
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(acm, "_LSTM_SEQ", fused)
        ac.train()
        ac.flat_grads.zero_()
        acts = ac.forward_heads(obs, n, sample_stride=24, tag="train", rnn=dict(R=Rm, h0=h0, keep_tm=keep))
        heads = acts[-1].clone()
        for li in li_rnn:
            sv = ac._rnn_saved_l[li]
            assert bool(sv["fused"]) == fused and sv["family"] == ("row_owned" if fused else "per_step"), sv["family"]
        last = [ac._rnn_saved_l[li]["Hprev"][Rm].clone() for li in li_rnn]
        ac.backward(acts, g_heads.clone(), obs, n, sample_stride=24)
        torch.cuda.synchronize()
        grads = ac.flat_to_ref(ac.flat_grads)
        ac.forward_heads(obs[:16], 16, sample_stride=24, tag="inf", rnn=dict(states=st_in))
        runs[fused] = dict(heads=heads, new_states=ac.new_rnn_states_of("inf").clone(),
                           **{f"last_h{i}": t for i, t in enumerate(last)}, **{f"grad {k}": v for k, v in grads.items()})
    assert any(k.startswith("grad ") and "weight_hh" in k for k in runs[True]), list(runs[True])
    for name, want in runs[False].items():
        got = runs[True][name]
        scale = float(want.abs().max())
        err = float((got.double().cpu() - want.double().cpu()).abs().max())
        print(f"{rnn_type} {name}: {err:.3e} (largest element {scale:.3e})")
        assert scale > 0 and err <= 2e-5 * scale, (name, err, scale)


def test_runner_trains_gru64_through_the_row_owned_passes(lib):
    """synthetic_ant, GRU-64, recurrence 8, async: three training iterations through the Runner; finite losses, the policy
    version advances and the BPTT passes ran as the row-owned kernels"""
    import sample_factory_amd.model.actor_critic as acm
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_continuous_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_ant", make_synthetic_continuous_env)
    assert acm._LSTM_SEQ
    cfg = default_cfg(env="synthetic_ant", use_rnn=True, rnn_type="gru", rnn_size=64, nonlinearity="tanh", normalize_input=True,
                      encoder_mlp_layers=[64, 64], rollout=8, recurrence=8, batch_size=512, num_batches_per_epoch=2, num_epochs=1,
                      num_workers=1, num_envs_per_worker=1, async_rl=True, serial_mode=False, seed=3, synthetic_num_agents=128,
                      normalize_returns=False)
    cfg, runner = make_runner(cfg)
    runner.init()
    lib.PROFILE = {}
    losses = []
    try:
        for _ in range(4):  # the first iteration only collects: three trained datasets
            stats = runner.iteration()
            if stats and "train" in stats:
                losses.append(stats["train"]["loss"])
        torch.cuda.synchronize()
        names = {k[-1] for k in lib.PROFILE}
    finally:
        lib.PROFILE = None
    ac = runner.learner.actor_critic
    assert runner.learner.train_step == 3 * 2
    assert len(losses) >= 1 and all(np.isfinite(v) for v in losses)
    assert ac._rnn_saved["fused"] and ac._rnn_saved["family"] == "row_owned"
    assert "k_rowseq_fwd<0, 64>" in names and "k_rowseq_bwd<0, 64>" in names, names
    assert torch.isfinite(ac.flat_params).all()
