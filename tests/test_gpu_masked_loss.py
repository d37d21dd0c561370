"""sf_ppo_loss_masked and sf_vtrace_masked (csrc/sf_rl.hip: k_masked_ppo_loss_md up to 8 members and k_masked_ppo_loss_mh
above, for up to 128 distribution parameters; k_masked_ppo_loss_wide from 129 on; k_masked_vtrace_ratio /
k_masked_vtrace_ratio_wide) against the float64 yardstick of tests/test_masked_loss_cpu.py (masked_dist_terms, held there
to the action-distribution objects) and its autograd.  Never another GPU path.

Which case reaches which kernel:
  k_masked_ppo_loss_md     [2] [6] [33] [128] (a plain Discrete as a one-member list), [4,3], [5]*8, [3,-2,5],
                           [100,-3,7,5,1,-1,3]
  k_masked_ppo_loss_mh     [3]*12
  k_masked_ppo_loss_wide   [300], [21]*8, [150,5]

Every case is 1024 rows read through a shuffled index into a dataset of 3072; the mask lives either in a [E, 9, A] slab
(mask_T = 8; the extra step of every env holds the complement of its step 0, so a launch that mapped rows as a flat
array would read wrong masks from env 1 on) or in a flat [N, A + 3] array with garbage in the padding."""
import numpy as np
import pytest
import torch

import oracle
from test_gpu_action_heads import (SCALARS, _cfg, check_loss, dev, finish_loss_data, logp_tol, make_loss_data,
                                   normal_logp64)
from test_gpu_wide_action_heads import tuple_logits
from test_masked_loss_cpu import (MASK_T, MASKED_LOSS_CASES, N_ROWS, make_mask, masked_case_ref, masked_dist_terms,
                                  masked_ref_loss, n_params)

pytestmark = pytest.mark.gpu

SENT = -7.0


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def device_mask(mask, slab):
    """the dataset's mask [N, A] on the device -> (tensor, mask_T): the slab layout [N / 8, 9, A] with mask_T = 8, or a
    flat view [N, A] of a [N, A + 3] array"""
    N, A = mask.shape
    m = dev(mask, torch.uint8)
    if slab:
        E = N // MASK_T
        s = torch.empty((E, MASK_T + 1, A), dtype=torch.uint8, device="cuda")
        s[:, :MASK_T] = m.view(E, MASK_T, A)
        s[:, MASK_T] = 1 - s[:, 0]
        return s, MASK_T
    s = torch.full((N, A + 3), 1, dtype=torch.uint8, device="cuda")
    s[:, :A] = m
    return s[:, :A], 0


def run_masked_loss(lib, params, values, ds, heads, c, index, mask, slab, masked=True):
    """sf_moments + sf_ppo_loss_masked + sf_loss_scalars on [values | params | 2 padding columns] heads; the gradient
    matrix, the ratios and the sums sit inside sentinel guard bands.  masked=False: the unmasked lib.ppo_loss on the same
    buffers.  Returns the scalars, the gradients, the ratios, the KL sum and the guards' state."""
    n, A = params.shape
    cfg = lib.sf_loss_cfg(clip_ratio=c["clip_ratio"], clip_value=c["clip_value"], value_loss_coeff=c["value_coeff"],
                          exploration_coeff=c["expl_coeff"], kl_coeff=c["kl_coeff"], exploration_kind=c["expl_kind"],
                          action_kind=0, dense_adv=0)
    if 1 < len(heads) <= 8:
        cfg.num_heads = len(heads)
        for i, h in enumerate(heads):
            cfg.head_n[i] = int(h)
    ld = 1 + A + 2
    m = torch.cat([dev(values)[:, None], dev(params), torch.zeros(n, 2, device="cuda")], 1).contiguous()
    G = torch.full((n + 2, ld), SENT, device="cuda")
    g = G[1:n + 1]
    R = torch.full((n + 32,), SENT, device="cuda")
    S = torch.full((24,), SENT, dtype=torch.float64, device="cuda")
    ratio, sums = R[16:16 + n], S[8:16]
    d = {k: dev(ds[k]) for k in ("actions", "old_logp", "old_params", "old_values", "adv", "targets")}
    valids = dev(ds["valids"], torch.bool)
    idx = dev(index, torch.int32)
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    out = torch.zeros(16, device="cuda")
    kw = {}
    if masked:
        mk, mask_T = device_mask(mask, slab)
        kw = dict(mask=mk, mask_T=mask_T)
    lib.moments(d["adv"], valids, idx, n, mom, offset=0)
    lib.ppo_loss(m[:, 1:], ld, m[:, 0], ld, d["actions"], d["old_logp"], d["old_params"], d["old_values"], d["adv"],
                 d["targets"], valids, idx, 0, n, A, cfg, mom, sums, g[:, 1:], g[:, 0], ratio_out=ratio,
                 head_sizes=heads if len(heads) > 1 else None, **kw)
    lib.loss_scalars(sums, mom, cfg, out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    res = {k: float(o[i]) for i, k in enumerate(SCALARS)}
    Gh, Rh, Sh = G.cpu().numpy(), R.cpu().numpy(), S.cpu().numpy()
    res["grad_params"], res["grad_values"] = Gh[1:n + 1, 1:1 + A], Gh[1:n + 1, 0]
    res["ratio"], res["kl_sum"] = Rh[16:16 + n], float(Sh[10])
    res["guards_intact"] = bool(np.all(Gh[0] == SENT) and np.all(Gh[n + 1] == SENT) and np.all(Gh[1:n + 1, 1 + A:] == SENT)
                                and np.all(Rh[:16] == SENT) and np.all(Rh[16 + n:] == SENT) and np.all(Sh[:8] == SENT)
                                and np.all(Sh[16:] == SENT))
    return res


_RUNS = {}


def gpu_case(lib, heads, expl_kind, kl_coeff, slab):
    """one launch per case, shared by the tests below"""
    key = (tuple(heads), expl_kind, kl_coeff, slab)
    if key not in _RUNS:
        (c, ds, index, values, g, mask, gm), ref = masked_case_ref(heads, expl_kind, kl_coeff)
        _RUNS[key] = run_masked_loss(lib, ds["params"], values, ds, heads, c, index, mask, slab)
    return _RUNS[key]


@pytest.mark.parametrize("heads,expl_kind,kl_coeff,slab", MASKED_LOSS_CASES, ids=str)
def test_masked_loss_vs_float64_autograd(lib, heads, expl_kind, kl_coeff, slab):
    """scalars and gradients within check_loss's bounds (the project's own for the unmasked loss) of float64 autograd of
    the yardstick.  Data as test_ppo_loss_vs_float64_autograd generates it, at 1024 rows; masks allow a column with
    probability 0.5, always the taken action.  check_loss asks for more than 0.98 of the samples off a kink:
    tests/test_masked_loss_cpu.py::test_gpu_cases_keep_their_samples_off_the_kinks confirms it for every case here from
    the float64 yardstick alone (the smallest fraction over the twelve cases is 0.997)."""
    (c, ds, index, values, g, mask, gm), ref = masked_case_ref(heads, expl_kind, kl_coeff)
    out = gpu_case(lib, heads, expl_kind, kl_coeff, slab)
    for k in SCALARS:
        print(f"{heads} {k}: got {out[k]!r} want {ref[k]!r}")
    keep = ~ref["kink"]
    err = np.abs(out["grad_params"][keep] - ref["grad_params"][keep])
    print(f"{heads} grad_params: max abs err {err.max():.3e}, largest gradient {np.abs(ref['grad_params']).max():.3e}")
    check_loss(out, ref, f"{heads} expl={expl_kind} kl={kl_coeff} slab={slab}")
    assert np.all(out["grad_params"][~g["valids"]] == 0) and np.all(out["grad_values"][~g["valids"]] == 0)


@pytest.mark.parametrize("heads,expl_kind,kl_coeff,slab", MASKED_LOSS_CASES, ids=str)
def test_masked_columns_get_exact_zeros_and_nothing_else_is_written(lib, heads, expl_kind, kl_coeff, slab):
    """g_params is 0.0 on every masked-out column of a Discrete slice (every slice here allows something), also where an
    entropy / KL term is on; the padding columns beyond A, the rows before and after the gradient matrix, and the bands
    around ratio_out and sums keep their sentinel"""
    (c, ds, index, values, g, mask, gm), ref = masked_case_ref(heads, expl_kind, kl_coeff)
    out = gpu_case(lib, heads, expl_kind, kl_coeff, slab)
    off = 0
    checked = 0
    for h in heads:
        if h > 0:
            z = out["grad_params"][:, off:off + h][gm[:, off:off + h] == 0]
            assert np.all(z == 0.0), (heads, off, np.abs(z).max())
            checked += z.size
        off += h if h > 0 else -2 * h
    assert checked > 0.25 * N_ROWS * sum(h for h in heads if h > 1) or max(heads) <= 2
    assert np.isfinite(out["grad_params"]).all() and np.isfinite(out["grad_values"]).all()
    assert out["guards_intact"]


@pytest.mark.parametrize("heads,slab", [([6], True), ([5] * 8, False), ([3] * 12, True), ([3, -2, 5], False),
                                        ([300], True), ([150, 5], False)], ids=str)
def test_all_ones_mask_is_the_unmasked_loss(lib, heads, slab):
    """a mask that allows everything: the same outputs, within check_loss, as the float64 UNMASKED yardstick"""
    c = _cfg(1, 0.2)
    rng = np.random.default_rng(n_params(heads) + 5)
    N, n = 3 * N_ROWS, N_ROWS
    ds = make_loss_data(rng, heads, N, n)
    index = rng.permutation(N)[:n].astype(np.int32)
    values, g = finish_loss_data(rng, ds, heads, index, c)
    out = run_masked_loss(lib, ds["params"], values, ds, heads, c, index, np.ones((N, n_params(heads)), np.uint8), slab)
    ref = masked_ref_loss(ds["params"], values, g["actions"], g["old_logp"], g["old_params"], g["old_values"], g["adv"],
                          g["targets"], g["valids"], heads, c, None)
    check_loss(out, ref, f"{heads} all-ones")
    assert out["guards_intact"]


@pytest.mark.parametrize("heads", [[5, 3], [3] * 12, [300, 4]], ids=str)
def test_all_zero_slices_behave_as_equal_logits(lib, heads):
    """every fourth row masks the whole first member out, with logits up to +-31 there (z - 1e9 absorbs |z| < 32 in f32):
    forward and gradient against the yardstick's equal-logits rule (log-prob -log n, p = 0, entropy 0, KL 0, gradient
    delta - 1 / n), within check_loss; and directly: with no entropy / KL term the slice's gradient is
    dL/dlogp * (delta - 1 / n), read off the neighbouring member's taken column"""
    for expl_kind, kl_coeff in ((1, 0.2), (0, 0.0)):
        c = _cfg(expl_kind, kl_coeff)
        rng = np.random.default_rng(n_params(heads) + expl_kind)
        N, n = 3 * N_ROWS, N_ROWS
        ds = make_loss_data(rng, heads, N, n, edges=False)
        h0 = heads[0]
        dead_mb = np.arange(n) % 4 == 0
        ds["params"][dead_mb, :h0] = rng.uniform(-31, 31, (int(dead_mb.sum()), h0)).astype(np.float32)
        index = rng.permutation(N)[:n].astype(np.int32)
        mask = make_mask(rng, heads, ds["actions"])
        mask[index[dead_mb], :h0] = 0
        ds["old_params"][index[dead_mb], :h0] = rng.uniform(-31, 31, (int(dead_mb.sum()), h0)).astype(np.float32)
        values, _ = finish_loss_data(rng, ds, heads, index, c)
        t = lambda x: torch.tensor(np.asarray(x, np.float64))
        lp, _, _ = masked_dist_terms(t(ds["params"]), t(ds["old_params"][index]), t(ds["actions"][index]), heads, mask[index])
        ds["old_logp"][index] = (lp.numpy() + rng.standard_normal(n) * 0.15).astype(np.float32)
        g = {k: ds[k][index] for k in ("actions", "old_logp", "old_params", "old_values", "adv", "targets", "valids")}
        ref = masked_ref_loss(ds["params"], values, g["actions"], g["old_logp"], g["old_params"], g["old_values"],
                              g["adv"], g["targets"], g["valids"], heads, c, mask[index])
        out = run_masked_loss(lib, ds["params"], values, ds, heads, c, index, mask, slab=bool(expl_kind))
        check_loss(out, ref, f"{heads} all-zero slices expl={expl_kind}")
        if expl_kind == 0:
            rows = np.flatnonzero(dead_mb & g["valids"] & ~ref["kink"])
            a0 = g["actions"][rows, 0].astype(int)
            gs = out["grad_params"][rows, :h0].astype(np.float64)
            taken = gs[np.arange(len(rows)), a0]
            dL = taken / (1.0 - 1.0 / h0)                       # dL/dlogp from the taken column: dL * (1 - 1 / n)
            want = -dL[:, None] / h0 * np.ones((1, h0))
            want[np.arange(len(rows)), a0] = taken
            np.testing.assert_allclose(gs, want, rtol=1e-5, atol=1e-6 * np.abs(gs).max())
            assert np.abs(dL).max() > 0


def _sample(lib, logits, values, mask, hs):
    """one masked sampler launch at B rows, T = 1: the slab's flat dataset arrays (actions, logits, log-probs) and the
    [B, 2, A] mask slab"""
    B, A = logits.shape
    nact = len(hs)
    heads = dev(np.concatenate([values[:, None], logits], 1))
    slab_mask = torch.empty((B, 2, A), dtype=torch.uint8, device="cuda")
    slab_mask[:, 0] = dev(mask, torch.uint8)
    slab_mask[:, 1] = 1 - slab_mask[:, 0]
    mview = slab_mask[:, 0]
    s = lambda *sh: torch.full(sh, SENT, device="cuda")
    tr = dict(actions=s(B, 1, nact), logits=s(B, 1, A), logp=s(B, 1), values=s(B, 2), ver=s(B, 1))
    if len(hs) == 1:
        lib.sample_write_step_masked(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, mview, mview.stride(0), B, A, 1, 0, 11, 5, 0,
                                     1.0, False, tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], None)
    else:
        lib.sample_write_step_tuple_masked(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, mview, mview.stride(0), B, hs, 1, 0, 11,
                                           5, 0, 1.0, False, tr["actions"], tr["logits"], tr["logp"], tr["values"],
                                           tr["ver"], None)
    torch.cuda.synchronize()
    return tr, slab_mask


@pytest.mark.parametrize("hs", [[6], [300], [4, 3], [21] * 8], ids=str)
def test_sampler_and_loss_agree_on_the_distribution(lib, hs):
    """512 rows sampled under a mask; the written logits, actions and log-probs go to the masked loss with the same
    logits as the current policy: per row |log ratio_out| <= 2 * logp_tol(logp, A) (one f32 log-prob on each side), the
    KL sum at most the rows' bounds added up.  The unmasked loss on the same data violates the bound: the control"""
    B, A = 512, n_params(hs)
    rng = np.random.default_rng(A)
    logits = tuple_logits(rng, hs, B, 3.0)
    values = rng.standard_normal(B).astype(np.float32)
    mask = (rng.random((B, A)) < 0.5).astype(np.uint8)
    off = 0
    for h in hs:
        mask[np.arange(B), off + rng.integers(0, h, B)] = 1
        off += h
    tr, slab_mask = _sample(lib, logits, values, mask, hs)
    acts, lgt, lp = tr["actions"].view(B, len(hs)), tr["logits"].view(B, A), tr["logp"].view(B)
    a_h, lp_h = acts.cpu().numpy(), lp.cpu().numpy()
    off = 0
    for i, h in enumerate(hs):
        assert mask[np.arange(B), off + a_h[:, i].astype(int)].all()
        off += h
    c = _cfg(1, 0.2)
    ds = dict(actions=a_h, old_logp=lp_h, old_params=lgt.cpu().numpy(), old_values=values,
              adv=rng.standard_normal(B).astype(np.float32), targets=rng.standard_normal(B).astype(np.float32),
              valids=np.ones(B, bool))
    index = np.arange(B, dtype=np.int32)
    bound = 2 * logp_tol(lp_h.astype(np.float64), A)
    out = run_masked_loss(lib, logits, values, ds, hs, c, index, mask, slab=False)
    # the slab the sampler read, in place (mask_T = 1: dataset row e at mask row 2 e)
    cfg = lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.5, value_loss_coeff=0.5, exploration_coeff=0.01, kl_coeff=0.2,
                          exploration_kind=1, action_kind=0, dense_adv=0)
    m = torch.cat([dev(values)[:, None], dev(logits)], 1).contiguous()
    g = torch.zeros_like(m)
    ratio = torch.zeros(B, device="cuda")
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    valids = torch.ones(B, dtype=torch.bool, device="cuda")
    lib.moments(dev(ds["adv"]), valids, None, B, mom)
    lib.ppo_loss(m[:, 1:], 1 + A, m[:, 0], 1 + A, acts, lp, lgt, dev(values), dev(ds["adv"]), dev(ds["targets"]), valids,
                 None, 0, B, A, cfg, mom, sums, g[:, 1:], g[:, 0], ratio_out=ratio, head_sizes=hs, mask=slab_mask, mask_T=1)
    torch.cuda.synchronize()
    for name, r, kl_sum in (("flat", out["ratio"], out["kl_sum"]), ("slab", ratio.cpu().numpy(), float(sums[2]))):
        lr = np.abs(np.log(r.astype(np.float64)))
        print(f"{hs} {name}: max |log ratio| {lr.max():.3e} (bound {bound.min():.3e}..), KL sum {kl_sum:.3e}")
        assert np.all(lr <= bound), (hs, name, lr.max(), bound.min())
        assert abs(kl_sum) <= bound.sum(), (hs, name, kl_sum)
    plain = run_masked_loss(lib, logits, values, ds, hs, c, index, mask, slab=False, masked=False)
    lr = np.abs(np.log(plain["ratio"].astype(np.float64)))
    assert (lr > bound).mean() > 0.5, (hs, (lr > bound).mean())


def _logp_size(params, actions, heads, mask):
    """per row, the sum of the sizes of the masked log-prob's terms (logp_size of tests/test_gpu_action_heads.py with the
    masked log-softmax)"""
    size = np.zeros(len(params))
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    off = col = 0
    for h in heads:
        if h > 0:
            l, _, _ = masked_dist_terms(t(params[:, off:off + h]), t(params[:, off:off + h]), t(actions[:, col:col + 1]),
                                        [h], mask[:, off:off + h])
            size += np.abs(l.numpy()) + 1.0
            off, col = off + h, col + 1
        else:
            D = -h
            size += np.abs(normal_logp64(actions[:, col:col + D], params[:, off:off + D],
                                         params[:, off + D:off + 2 * D])).sum(1) + D
            off, col = off + 2 * D, col + D
    return size


@pytest.mark.parametrize("heads,rec,rho_hat,c_hat,slab", [([6], 8, 1.0, 1.0, True), ([4, 3], 4, 0.5, 2.0, False),
                                                          ([150, 5], 8, 2.0, 0.5, True), ([3, -2, 5], 8, 1.0, 1.0, False)],
                         ids=str)
def test_masked_vtrace_vs_oracle_on_float64_masked_ratios(lib, heads, rec, rho_hat, c_hat, slab):
    """lib.vtrace(..., mask=...) against oracle.vtrace fed clamp(exp(logp64 - old_logp), 0.05, 20) of the float64 MASKED
    log-probs; rows read through a shuffled index; logp - old_logp beyond 88 and below log 0.05 in some rows.  Tolerances
    of test_vtrace_vs_float64: 2e-5 relative, (2e-5 + eps) * value scale absolute, eps = 2e-6 of the largest sum of the
    log-prob's term sizes"""
    rng = np.random.default_rng(rec * 7 + sum(abs(h) for h in heads))
    A, gamma = n_params(heads), 0.99
    n, N = N_ROWS, 2 * N_ROWS
    ds = make_loss_data(rng, heads, N, n, edges=False)
    params = ds["params"]
    index = rng.permutation(N)[:n].astype(np.int32)
    off = col = 0
    for h in heads:  # Box members: actions drawn from the current policy, as a rollout's are
        if h < 0:
            D = -h
            mu, sd = params[:, off:off + D], np.exp(params[:, off + D:off + 2 * D].astype(np.float64))
            ds["actions"][index, col:col + D] = (mu + sd * rng.standard_normal((n, D))).astype(np.float32)
        off, col = off + (h if h > 0 else -2 * h), col + (1 if h > 0 else -h)
    mask = make_mask(rng, heads, ds["actions"])
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    lp = masked_dist_terms(t(params), t(params), t(ds["actions"][index]), heads, mask[index])[0].numpy()
    shift = rng.standard_normal(n) * 0.5
    k = rng.random(n)
    shift[k < 0.04] = -90.0
    shift[(k >= 0.04) & (k < 0.08)] = 4.0
    old_logp = np.zeros(N, np.float32)
    old_logp[index] = (lp + shift).astype(np.float32)
    values = rng.standard_normal(n).astype(np.float32)
    rewards = rng.standard_normal(N).astype(np.float32)
    dones = rng.random(N) < 0.1
    mk, mask_T = device_mask(mask, slab)
    vs, adv = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lib.vtrace(dev(params), A, dev(values), 1, dev(ds["actions"]), dev(old_logp), dev(rewards), dev(dones, torch.bool),
               dev(index, torch.int32), 0, n, A, 0, rec, gamma, rho_hat, c_hat, vs, adv,
               head_sizes=heads if len(heads) > 1 else None, mask=mk, mask_T=mask_T)
    torch.cuda.synchronize()
    ratio = np.clip(np.exp(lp - old_logp[index].astype(np.float64)), 0.05, 20.0)
    rvs, radv = oracle.vtrace(ratio, values, rewards[index], dones[index], rec, gamma, rho_hat, c_hat)
    scale = 1.0 + np.abs(values).max()
    eps = 2e-6 * _logp_size(params, ds["actions"][index], heads, mask[index]).max()
    np.testing.assert_allclose(vs.cpu().numpy(), rvs, rtol=2e-5, atol=(2e-5 + eps) * scale)
    np.testing.assert_allclose(adv.cpu().numpy(), radv, rtol=2e-5, atol=(2e-5 + eps) * scale)
    # the control: the unmasked ratios are other numbers
    vs2, adv2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lib.vtrace(dev(params), A, dev(values), 1, dev(ds["actions"]), dev(old_logp), dev(rewards), dev(dones, torch.bool),
               dev(index, torch.int32), 0, n, A, 0, rec, gamma, rho_hat, c_hat, vs2, adv2,
               head_sizes=heads if len(heads) > 1 else None)
    torch.cuda.synchronize()
    assert np.abs(adv2.cpu().numpy() - radv).max() > 100 * (2e-5 + eps) * scale
