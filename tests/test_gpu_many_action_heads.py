"""Tuple action spaces of 9 to 64 members (SF_MAX_ACTION_HEADS) on the sampler, PPO loss and V-trace kernels of
csrc/sf_rl.hip, against the float64 references of tests/test_gpu_action_heads.py and, for the sampler and V-trace, the
CPU oracle.  (oracle.ppo_loss keeps eight members on its stack and is not called here.)

Head lists, the smallest that reach each path:

  (3,) * 9             the first list over eight members, A = 27              k_ppo_loss_mh, narrow sampler / ratio
  (5,) * 17            A = 85                                                 the same
  (2,) * 64            capacity, A = 128: the last narrow width               the same
  (3,) * 43            A = 129: the first wide width, many members            k_*_wide, 43 rows of per-member LDS state
  (11,) * 17           A = 187, a discretised Humanoid                        k_*_wide
  (2,) * 63 + (130,)   a wide member behind 63 narrow ones                    k_*_wide, member 63 strides three chunks
  (3,) * 9 + (-2, 4)   a Box(2) member at index 9                             k_ppo_loss_mh
  (21,) * 8 + (-3, 5)  a mixed wide list, A = 179                             k_*_wide

259 rows (envs) everywhere: one 256-thread block plus three rows, 64 four-row blocks plus three waves — a partial block
and a partial wave group both occur.  The loss reads through a shuffled index into a dataset three times the
minibatch, with invalid rows.  Tolerances are those of the two existing suites, unchanged; what is per member there
(logp_tol) is added up over the members here."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import oracle
from test_gpu_action_heads import (SCALARS, _cfg, _slab, check_inverse_cdf, check_loss, dev, finish_loss_data,
                                   log_softmax64, logp_size, logp_tol, make_loss_data, normal_logp64, normals, ref_logp,
                                   ref_loss, ref_vtrace, run_tuple, uniforms_discrete)
from test_gpu_wide_action_heads import agree_with_oracle, check_wide_draw, n_params, tuple_logits

pytestmark = pytest.mark.gpu

LISTS = [(3,) * 9, (5,) * 17, (2,) * 64, (3,) * 43, (11,) * 17, (2,) * 63 + (130,), (3,) * 9 + (-2, 4),
         (21,) * 8 + (-3, 5)]
ROWS = 259


def list_id(hs):
    return f"{len(hs)}heads_A{n_params(hs)}"


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def members(hs):
    """(member index, size, first parameter column, first action column) of every member"""
    off = col = 0
    for i, h in enumerate(hs):
        yield i, h, off, col
        off, col = off + (h if h > 0 else -2 * h), col + (1 if h > 0 else -h)


# ------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("hs", LISTS, ids=list_id)
def test_many_head_sampler_vs_float64(lib, hs):
    """Discrete member h: the float64 inverse CDF of the uniform of counter (step, h, 2, 0) (check_inverse_cdf on the
    lane-per-row sampler, check_wide_draw on the wave-per-row one, as in their own suites); Box member h: float64
    Box-Muller normals of counter (step, k / 2, 3, h).  The recorded log-prob is the float64 sum over the members at the
    recorded actions, the recorded logits are the raw ones (run_tuple compares them bit for bit) and the int32
    env_actions of an all-Discrete list equal the recorded row.  Deterministic mode: first maxima / means."""
    B, seed, step, row0 = ROWS, 21 + len(hs), 8, 3001
    rng = np.random.default_rng(len(hs) * 1000 + n_params(hs))
    logits = tuple_logits(rng, list(hs), B, 8.0)
    values = rng.standard_normal(B).astype(np.float32)
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    wide = n_params(hs) > 128
    a, lp = run_tuple(lib, logits, values, list(hs), seed=seed, step=step, row0=row0)
    am, lpm = run_tuple(lib, logits, values, list(hs), seed=seed, step=step, row0=row0, deterministic=True)
    lp_want, lpm_want, tol = np.zeros(B), np.zeros(B), np.zeros(B)
    r = np.arange(B)
    for i, h, off, col in members(hs):
        if h > 0:
            ls = log_softmax64(logits[:, off:off + h])
            u = uniforms_discrete(seed, step, rows, head=i)
            if wide:
                check_wide_draw(a[:, col], np.exp(ls), u, f"member {i}")
            else:
                check_inverse_cdf(a[:, col], np.exp(ls), u, f"member {i}")
            got = ls[r, a[:, col].astype(np.int64)]
            lp_want += got
            tol += logp_tol(got, h)
            first = np.argmax(logits[:, off:off + h], 1)
            np.testing.assert_array_equal(am[:, col], first)
            lpm_want += ls[r, first]
        else:
            D = -h
            mu, ls_ = logits[:, off:off + D], logits[:, off + D:off + 2 * D]
            sd = np.clip(np.exp(ls_.astype(np.float64)), 1e-4, 1e4)
            want = mu + sd * normals(seed, step, rows, D, member=i)
            got = a[:, col:col + D]
            np.testing.assert_array_less(np.abs(got - want), 1e-5 * (1 + np.abs(want)) + 4e-6 * sd)
            t = normal_logp64(got, mu, ls_)
            lp_want += t.sum(1)
            tol += 2e-6 * (D + np.abs(t).sum(1))
            np.testing.assert_array_equal(am[:, col:col + D], mu)
            lpm_want += normal_logp64(mu, mu, ls_).sum(1)
    np.testing.assert_array_less(np.abs(lp - lp_want), tol)
    np.testing.assert_array_less(np.abs(lpm - lpm_want), tol + 1e-5)


@pytest.mark.parametrize("hs", LISTS, ids=list_id)
def test_many_head_sampler_deterministic_ties(lib, hs):
    """integer logits with exact ties in every Discrete member, and rows where all are equal: torch.argmax's FIRST maximum"""
    B = ROWS
    rng = np.random.default_rng(3 + len(hs))
    logits = np.round(rng.standard_normal((B, n_params(hs)))).astype(np.float32)
    logits[:32] = 1.0
    a, _ = run_tuple(lib, logits, np.zeros(B, np.float32), list(hs), seed=1, step=2, row0=3, deterministic=True)
    ties = 0
    for i, h, off, col in members(hs):
        if h > 0:
            z = logits[:, off:off + h]
            np.testing.assert_array_equal(a[:, col], np.argmax(z, 1), err_msg=f"member {i}")
            ties += int(((z == z.max(1, keepdims=True)).sum(1) > 1).sum())
        else:
            np.testing.assert_array_equal(a[:, col:col - h], logits[:, off:off - h])
    assert ties > 32 * sum(h > 0 for h in hs) and np.all(a[:32, [c for _, h, _, c in members(hs) if h > 0]] == 0)


@pytest.mark.parametrize("hs", LISTS, ids=list_id)
def test_many_head_sampler_vs_oracle(lib, hs):
    """oracle.sample_tuple restates the sampler in float32 on the host: the bounds of test_wide_samplers_vs_oracle"""
    B, seed, step, row0 = ROWS, 11, 77, 5
    rng = np.random.default_rng(77 + len(hs))
    logits = tuple_logits(rng, list(hs), B, 3.0)
    for i, h, off, col in members(hs):
        if h < 0:
            logits[:, off - h:off - 2 * h] = rng.uniform(-2, 1, (B, -h))
    values = rng.standard_normal(B).astype(np.float32)
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    a, lp = run_tuple(lib, logits, values, list(hs), seed=seed, step=step, row0=row0)
    a_ref, lp_ref = oracle.sample_tuple(logits, list(hs), seed, step, row0=row0)
    same = np.ones(B, bool)
    for i, h, off, col in members(hs):
        if h > 0:
            p = np.exp(log_softmax64(logits[:, off:off + h]))
            agree_with_oracle(a[:, col], a_ref[:, col], p, uniforms_discrete(seed, step, rows, head=i), f"member {i}")
            same &= a[:, col] == a_ref[:, col]
        else:
            np.testing.assert_allclose(a[:, col:col - h], a_ref[:, col:col - h], rtol=1e-5, atol=1e-5)
    assert same.mean() > 0.9
    np.testing.assert_allclose(lp[same], lp_ref[same], atol=5e-5, rtol=1e-5)


def test_replayed_sampler_launch_reads_the_long_head_list(lib):
    """a launch program keeps the CONVERTED arguments: the int32 array of a 17-member list lives on in the recorded
    argument tuple after the wrapper's locals are gone, and a replay with the next Philox step draws what a direct call
    with that step draws"""
    hs = [5] * 17
    B, A, T = ROWS, 85, 2
    rng = np.random.default_rng(5)
    heads = dev(np.concatenate([rng.standard_normal((B, 1)), rng.standard_normal((B, A)) * 2], 1).astype(np.float32))
    tr, tr2 = _slab(B, T, 17, A), _slab(B, T, 17, A)
    ea, ea2 = (torch.zeros((B, 17), dtype=torch.int32, device="cuda") for _ in range(2))
    step = C.c_uint32(5)
    with lib.record_launches() as prog:
        lib.sample_write_step_tuple(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, B, hs, T, 0, 11, step, 7, 1.0, False,
                                    tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], ea)
    assert [c[2] for c in prog.calls] == ["sf_sample_write_step_tuple"] and prog.unsafe is None
    kept = [x for x in prog.calls[0][1] if isinstance(x, C.Array)]
    assert len(kept) == 1 and list(kept[0]) == hs
    first = tr["actions"][:, 0].clone()
    del hs
    gc.collect()
    _ = [(C.c_int32 * 17)(*([-9] * 17)) for _ in range(64)]  # a freed array's memory would be handed out again here
    step.value = 6
    prog.replay()
    lib.sample_write_step_tuple(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, B, [5] * 17, T, 0, 11, 6, 7, 1.0, False,
                                tr2["actions"], tr2["logits"], tr2["logp"], tr2["values"], tr2["ver"], ea2)
    torch.cuda.synchronize()
    assert torch.equal(tr["actions"], tr2["actions"]) and torch.equal(tr["logp"], tr2["logp"]) and torch.equal(ea, ea2)
    assert not torch.equal(first, tr["actions"][:, 0])
    assert ((ea >= 0) & (ea < 5)).all()


# ------------------------------------------------------------------------------------------------ PPO loss
def run_loss_heads(lib, params, values, ds, heads, c, index, dense=None, ov_T=0, entry="wrapper"):
    """sf_moments + the loss + sf_loss_scalars with the head list passed as an ARGUMENT (sf_ppo_loss_heads); the struct's
    own list stays empty.  dense: (adv, targets) in minibatch order (what V-trace leaves behind).  ov_T > 0: old_values is
    the slab's [E, ov_T + 1] array read in place.  entry="raw": sf_ppo_loss_heads called directly (any list length)."""
    n, A = params.shape
    cfg = lib.sf_loss_cfg(clip_ratio=c["clip_ratio"], clip_value=c["clip_value"], value_loss_coeff=c["value_coeff"],
                          exploration_coeff=c["expl_coeff"], kl_coeff=c["kl_coeff"], exploration_kind=c["expl_kind"],
                          action_kind=0, dense_adv=int(dense is not None), old_values_T=ov_T)
    m = torch.cat([dev(values)[:, None], dev(params)], 1).contiguous()
    g = torch.zeros_like(m)
    idx = dev(index, torch.int32)
    valids = dev(ds["valids"], torch.bool)
    old_values = ds["old_values"]
    if ov_T:  # dataset row e * T + t lives at e * (T + 1) + t; the last column is never read
        ov = np.full((len(old_values) // ov_T, ov_T + 1), 1e9, np.float32)
        ov[:, :ov_T] = old_values.reshape(-1, ov_T)
        old_values = ov.reshape(-1)
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    out = torch.zeros(16, device="cuda")
    if dense is None:
        adv, tgt = dev(ds["adv"]), dev(ds["targets"])
        lib.moments(adv, valids, idx, n, mom)
    else:
        adv, tgt = dev(dense[0]), dev(dense[1])
        lib.moments(adv, valids[idx.long()].contiguous(), None, n, mom)
    args = (m[:, 1:], 1 + A, m[:, 0], 1 + A, dev(ds["actions"]), dev(ds["old_logp"]), dev(ds["old_params"]),
            dev(old_values), adv, tgt, valids, idx, 0, n, A, cfg, mom, sums, g[:, 1:], g[:, 0])
    if entry == "wrapper":
        lib.ppo_loss(*args, head_sizes=list(heads))
    else:
        p = lambda t: C.c_void_p(t.data_ptr())
        hn = (C.c_int32 * len(heads))(*heads)
        rc = lib.load().sf_ppo_loss_heads(p(args[0]), 1 + A, p(args[2]), 1 + A, *[p(t) for t in args[4:12]], C.c_int64(0),
                                          C.c_int64(n), A, C.byref(cfg), p(mom), p(sums), p(args[18]), p(args[19]), None,
                                          hn, len(heads), lib.stream())
        assert rc == 0, lib.load().sf_last_error()
    assert cfg.num_heads == 0 and list(cfg.head_n) == [0] * 8
    lib.loss_scalars(sums, mom, cfg, out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    res = {k: float(o[i]) for i, k in enumerate(SCALARS)}
    res["grad_params"], res["grad_values"] = g[:, 1:].cpu().numpy(), g[:, 0].cpu().numpy()
    return res


def loss_cases():
    for hs in LISTS:
        yield hs, 1, 0.1                                         # entropy exploration + KL loss
        yield (hs, 2, 0.2) if all(h > 0 for h in hs) else (hs, 0, 0.3)  # symmetric KL: categorical lists only


@pytest.mark.parametrize("hs,expl_kind,kl_coeff", list(loss_cases()),
                         ids=lambda v: list_id(v) if isinstance(v, tuple) else str(v))
def test_many_head_ppo_loss_vs_float64_autograd(lib, hs, expl_kind, kl_coeff):
    """one minibatch of 259 rows and one float64 autograd reference, launched three ways: dataset advantages through a
    shuffled index, dense (minibatch-order) advantages and targets, and old_values read in place from a [E, T + 1] slab.
    Losses, scalars and every gradient row to check_loss's tolerances; invalid rows carry exact zeros; the three reads
    differ in addressing only, so their gradients are equal bit for bit."""
    heads = list(hs)
    c = _cfg(expl_kind, kl_coeff)
    rng = np.random.default_rng(n_params(hs) * 31 + len(hs) + expl_kind)
    n, T = ROWS, 7
    N = 3 * n
    assert N % T == 0
    ds = make_loss_data(rng, heads, N, n)
    index = rng.permutation(N)[:n].astype(np.int32)
    values, g = finish_loss_data(rng, ds, heads, index, c)
    assert (~g["valids"]).sum() >= 5
    ref = ref_loss(ds["params"], values, g["actions"], g["old_logp"], g["old_params"], g["old_values"], g["adv"],
                   g["targets"], g["valids"], heads, c)
    outs = dict(index=run_loss_heads(lib, ds["params"], values, ds, heads, c, index),
                dense_adv=run_loss_heads(lib, ds["params"], values, ds, heads, c, index, dense=(g["adv"], g["targets"])),
                old_values_T=run_loss_heads(lib, ds["params"], values, ds, heads, c, index, ov_T=T))
    for read, out in outs.items():
        check_loss(out, ref, f"{hs} expl={expl_kind} kl={kl_coeff} {read}")
        assert np.all(out["grad_params"][~g["valids"]] == 0) and np.all(out["grad_values"][~g["valids"]] == 0)
    np.testing.assert_array_equal(outs["index"]["grad_params"], outs["dense_adv"]["grad_params"])
    np.testing.assert_array_equal(outs["index"]["grad_params"], outs["old_values_T"]["grad_params"])
    np.testing.assert_array_equal(outs["index"]["grad_values"], outs["old_values_T"]["grad_values"])


@pytest.mark.parametrize("hs", [(3, -2, 5), (7, 4, 2), (21,) * 8], ids=list_id)
def test_head_list_entry_point_equals_the_struct_one_up_to_eight_members(lib, hs):
    """sf_ppo_loss_heads with a list the struct could hold runs the kernels sf_ppo_loss runs: the same bits"""
    from test_gpu_action_heads import run_loss
    heads = list(hs)
    c = _cfg(1, 0.1)
    rng = np.random.default_rng(n_params(hs))
    n, N = ROWS, 3 * ROWS
    ds = make_loss_data(rng, heads, N, n)
    index = rng.permutation(N)[:n].astype(np.int32)
    values, _ = finish_loss_data(rng, ds, heads, index, c)
    a = run_loss(lib, ds["params"], values, ds["actions"], ds["old_logp"], ds["old_params"], ds["old_values"], ds["adv"],
                 ds["targets"], ds["valids"], heads, c, index=index)
    b = run_loss_heads(lib, ds["params"], values, ds, heads, c, index, entry="raw")
    for k in SCALARS:
        assert a[k] == b[k], k
    np.testing.assert_array_equal(a["grad_params"], b["grad_params"])
    np.testing.assert_array_equal(a["grad_values"], b["grad_values"])


# ------------------------------------------------------------------------------------------------ V-trace
def vtrace_inputs(rng, heads, rec, ntraj, read):
    """the inputs of test_vtrace_vs_float64 at ntraj * rec rows: ratios from float64 log-probs, logp - old_logp > 88 and
    below log 0.05 in some rows, dones on the first and the last step of some trajectories"""
    A = n_params(heads)
    n, N = ntraj * rec, 2 * ntraj * rec
    ds = make_loss_data(rng, heads, N, n, edges=False)
    params = ds["params"]
    if read == "index":
        index = rng.permutation(N)[:n].astype(np.int32)
        rows, offset = index, 0
    else:
        index, offset = None, rec * 5
        rows = np.arange(offset, offset + n)
    for i, h, off, col in members(heads):  # Box members: actions drawn from the current policy, as a rollout's are
        if h < 0:
            D = -h
            mu, sd = params[:, off:off + D], np.exp(params[:, off + D:off + 2 * D].astype(np.float64))
            ds["actions"][rows, col:col + D] = (mu + sd * rng.standard_normal((n, D))).astype(np.float32)
    g_act = ds["actions"][rows]
    lp = ref_logp(params, dict(old_params=ds["old_params"][rows], actions=g_act), heads)
    shift = rng.standard_normal(n) * 0.5
    k = rng.random(n)
    shift[k < 0.04] = -90.0
    shift[(k >= 0.04) & (k < 0.08)] = 4.0
    old_logp = np.zeros(N, np.float32)
    old_logp[rows] = (lp + shift).astype(np.float32)
    values = rng.standard_normal(n).astype(np.float32)
    rewards = rng.standard_normal(N).astype(np.float32)
    dones = rng.random(N) < 0.1
    first, last = np.arange(0, n, rec), np.arange(rec - 1, n, rec)
    dones[rows[first[::3]]] = True
    dones[rows[last[1::3]]] = True
    return dict(A=A, n=n, params=params, actions=ds["actions"], g_act=g_act, lp=lp, old_logp=old_logp, values=values,
                rewards=rewards, dones=dones, index=index, offset=offset, rows=rows)


def launch_vtrace(lib, d, heads, rec, gamma, rho_hat, c_hat):
    vs, adv = torch.zeros(d["n"], device="cuda"), torch.zeros(d["n"], device="cuda")
    lib.vtrace(dev(d["params"]), d["A"], dev(d["values"]), 1, dev(d["actions"]), dev(d["old_logp"]), dev(d["rewards"]),
               dev(d["dones"], torch.bool), dev(d["index"], torch.int32) if d["index"] is not None else None,
               d["offset"], d["n"], d["A"], 0, rec, gamma, rho_hat, c_hat, vs, adv, head_sizes=heads)
    torch.cuda.synchronize()
    return vs.cpu().numpy(), adv.cpu().numpy()


@pytest.mark.parametrize("read", ["index", "offset"])
@pytest.mark.parametrize("hs", LISTS, ids=list_id)
def test_many_head_vtrace_vs_float64(lib, hs, read):
    """259 rows = 37 trajectories of 7 steps, the (rho_hat, c_hat) settings of test_vtrace_vs_float64; its tolerance: 2e-5
    relative; absolute, (2e-5 + eps) times the value scale with eps = 2e-6 of the largest sum of the log-prob's term sizes"""
    heads, rec, gamma = list(hs), 7, 0.99
    rng = np.random.default_rng(rec * 7 + n_params(hs) + len(hs))
    d = vtrace_inputs(rng, heads, rec, ROWS // rec, read)
    assert d["n"] == ROWS
    rows = d["rows"]
    scale = 1.0 + np.abs(d["values"]).max()
    eps = 2e-6 * logp_size(d["params"], d["g_act"], heads).max()
    for rho_hat, c_hat in ((1.0, 1.0), (0.5, 2.0), (2.0, 0.5)):
        vs, adv = launch_vtrace(lib, d, heads, rec, gamma, rho_hat, c_hat)
        rvs, radv = ref_vtrace(d["lp"], d["old_logp"][rows], d["values"], d["rewards"][rows], d["dones"][rows], rec, gamma,
                               rho_hat, c_hat)
        np.testing.assert_allclose(vs, rvs, rtol=2e-5, atol=(2e-5 + eps) * scale)
        np.testing.assert_allclose(adv, radv, rtol=2e-5, atol=(2e-5 + eps) * scale)


@pytest.mark.parametrize("hs", [(5,) * 17, (11,) * 17, (3,) * 9 + (-2, 4)], ids=list_id)
def test_many_head_vtrace_vs_oracle(lib, hs):
    """against the oracle's recursion fed with float64 ratios: the tolerance of test_wide_vtrace_vs_oracle"""
    heads, rec = list(hs), 7
    rng = np.random.default_rng(rec + n_params(hs))
    d = vtrace_inputs(rng, heads, rec, ROWS // rec, "offset")
    rows = d["rows"]
    d["old_logp"][rows] = (d["lp"] + rng.standard_normal(d["n"]) * 0.3).astype(np.float32)  # ratios inside the clamp
    vs, adv = launch_vtrace(lib, d, heads, rec, 0.99, 0.9, 0.8)
    ratio = np.clip(np.exp(d["lp"] - d["old_logp"][rows]), 0.05, 20.0).astype(np.float32)
    rvs, radv = oracle.vtrace(ratio, d["values"], d["rewards"][rows], d["dones"][rows].astype(np.float32), rec, 0.99, 0.9, 0.8)
    np.testing.assert_allclose(vs, rvs, atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(adv, radv, atol=2e-5, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_head_lists_are_refused_before_any_launch(lib):
    """65 members, sizes that do not sum to A, and nine members in sf_ppo_loss's struct: SfHipError with the limit in the
    text, and nothing written — the outputs keep their sentinels (sums included: not even the memset ran)"""
    n, SENT = 16, -7.0
    full = lambda *s: torch.full(s, SENT, device="cuda")
    cfg = lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.5, value_loss_coeff=0.5, exploration_coeff=0.01, kl_coeff=0.1,
                          exploration_kind=1, action_kind=0)
    for hs, A, entry, what in (([2] * 65, 130, "heads", "limit is 64"), ([3] * 9, 28, "heads", "sum to 27, A = 28"),
                               ([3] * 9, 27, "struct", "limit is 8")):
        m, g = full(n, 1 + A), full(n, 1 + A)
        sums = torch.full((8,), SENT, dtype=torch.float64, device="cuda")
        mom = torch.tensor([1.0, 2.0, 8.0], dtype=torch.float64, device="cuda")
        z = lambda *s: torch.zeros(s, device="cuda")
        if entry == "struct":
            cfg.num_heads = 9
        with pytest.raises(lib.SfHipError, match=what):
            lib.ppo_loss(m[:, 1:], 1 + A, m[:, 0], 1 + A, z(n, len(hs)), z(n), z(n, A), z(n), z(n), z(n),
                         torch.ones(n, dtype=torch.bool, device="cuda"), None, 0, n, A, cfg, mom, sums, g[:, 1:], g[:, 0],
                         head_sizes=hs if entry == "heads" else None)
        torch.cuda.synchronize()
        assert (g == SENT).all() and (sums == SENT).all()
        cfg.num_heads = 0
        if entry == "heads":
            vs, adv = full(n), full(n)
            with pytest.raises(lib.SfHipError, match=what):
                lib.vtrace(m[:, 1:], 1 + A, m[:, 0], 1 + A, z(n, len(hs)), z(n), z(n), torch.zeros(n, dtype=torch.bool, device="cuda"),
                           None, 0, n, A, 0, 8, 0.99, 1.0, 1.0, vs, adv, head_sizes=hs)
            torch.cuda.synchronize()
            assert (vs == SENT).all() and (adv == SENT).all()
    hs, A = [2] * 65, 130
    tr = _slab(n, 2, 65, A)
    heads = torch.zeros(n, 1 + A, device="cuda")
    with pytest.raises(lib.SfHipError, match="limit is 64"):
        lib.sample_write_step_tuple(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, n, hs, 2, 0, 1, 1, 0, 1.0, False, tr["actions"],
                                    tr["logits"], tr["logp"], tr["values"], tr["ver"], None)
    torch.cuda.synchronize()
    assert all((v == SENT).all() for v in tr.values())
