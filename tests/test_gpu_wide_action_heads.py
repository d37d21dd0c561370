"""The wave-per-row kernel family of csrc/sf_rl.hip (k_sample_write_wide, k_ppo_loss_wide, k_vtrace_ratio_wide), which
serves every distribution with more than 128 parameters, against the float64 references of
tests/test_gpu_action_heads.py and against the CPU oracle.

Widths sit where a wave that strides a row 64 columns at a time can go wrong: 129 (one column past two full strides),
191 / 192 / 193 (the tail around a multiple of 64), 1000 (not a multiple of 4, 16 chunks), 4096 (64 chunks of CDF
carry).  Head lists: a wide member first ([129, 3], [200, 1, ..., 2]), a wide member between narrow ones and a Box
([5, 300, -2, 7]) and narrow members whose TOTAL is wide ([21] * 8 = 168 logits).

Inverse-CDF draws are checked per row against the float64 CDF: the drawn action's interval must lie within 1e-5 of the
uniform and at most 0.5 % of the rows may differ from the float64 first crossing.  (check_inverse_cdf's own cap on the
share of uniforms within 1e-5 of a boundary is a property of the inputs: with A boundaries per row that share grows
with A, 1.7 % at A = 1000.)  A float32 serial inverse CDF on such inputs differs from float64 in 0-3 of 4096 rows for
A <= 1000 and in 7-14 rows at A = 4096, where the f32 CDF is up to 1.8e-5 from the float64 one; A = 4096 therefore gets
the range, probability and log-prob checks only."""
import math

import numpy as np
import pytest
import torch

import oracle
from test_gpu_action_heads import (ROWS_HEAD0, SEED_HI, STEP_HI, _cfg, _slab, check_loss, dev, finish_loss_data,
                                   log_softmax64, logp_size, logp_tol, make_loss_data, normal_logp64, normals, ref_logp,
                                   ref_loss, ref_vtrace, run_loss, run_masked, run_sampler, run_tuple, uniforms_discrete,
                                   SCALARS)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def n_params(heads):
    return sum(h if h > 0 else -2 * h for h in heads)


def check_wide_draw(a, p, u, what, allowed=None, crossing=True):
    """a: drawn actions, p: float64 probabilities [B, A], u: float64 uniforms.  Every draw is in range, has float64
    probability >= 1e-30 and (crossing) its CDF interval lies within 1e-5 of its uniform; at most 0.5 % of the rows
    differ from the float64 first crossing.  Returns the rows that differ."""
    B, A = p.shape
    ai = a.astype(np.int64)
    assert np.all((ai >= 0) & (ai < A) & (a == ai)), what
    r = np.arange(B)
    assert np.all(p[r, ai] >= 1e-30), (what, "drew an action of zero probability")
    if allowed is not None:
        assert np.all(allowed[r, ai]), (what, "drew a masked-out action")
    if not crossing:
        return None
    cdf = np.cumsum(p, 1)
    lo = np.concatenate([np.zeros((B, 1)), cdf[:, :-1]], 1)
    want = np.minimum((cdf <= u[:, None]).sum(1), A - 1)
    in_band = (lo[r, ai] - 1e-5 <= u) & (u < cdf[r, ai] + 1e-5)
    assert in_band.all(), (what, np.flatnonzero(~in_band)[:8], ai[~in_band][:8], want[~in_band][:8], u[~in_band][:8])
    diff = ai != want
    assert diff.mean() <= 5e-3, (what, "rows that differ from the float64 first crossing", int(diff.sum()))
    return diff


# ------------------------------------------------------------------------------------------------ samplers
@pytest.mark.parametrize("A", [129, 192, 193, 1000, 4096])
def test_wide_categorical_sampler_vs_float64_inverse_cdf(lib, A):
    """logits at scales 1, 8 and 40 through the [value | logits | pad] layout; log-prob = float64 log_softmax at the
    drawn action; deterministic mode returns the FIRST maximum (integer logits with many ties, all-equal rows: 0)"""
    B = 2048 if A == 4096 else 4096
    seed, step, row0 = 1234 + A, 77, 100003 + 17 * A
    rng = np.random.default_rng(A)
    values = rng.standard_normal(B).astype(np.float32)
    u = uniforms_discrete(seed, step, np.arange(row0, row0 + B, dtype=np.uint32))
    for scale in (1.0, 8.0, 40.0):
        logits = (rng.standard_normal((B, A)) * scale).astype(np.float32)
        a, lp = run_sampler(lib, logits, values, kind=0, seed=seed, step=step, row0=row0)
        ls = log_softmax64(logits)
        check_wide_draw(a[:, 0], np.exp(ls), u, f"A={A} scale={scale}", crossing=A <= 1000)
        want = ls[np.arange(B), a[:, 0].astype(np.int64)]
        np.testing.assert_array_less(np.abs(lp - want), logp_tol(want, A))
    logits = np.round(rng.standard_normal((B, A)) * 1.5).astype(np.float32)
    logits[:64] = 3.0
    a, lp = run_sampler(lib, logits, values, kind=0, seed=seed, step=step, row0=row0, deterministic=True)
    np.testing.assert_array_equal(a[:, 0], np.argmax(logits, 1))
    assert np.all(a[:64, 0] == 0)
    ls = log_softmax64(logits)
    want = ls[np.arange(B), np.argmax(logits, 1)]
    np.testing.assert_array_less(np.abs(lp - want), logp_tol(want, A))


@pytest.mark.parametrize("A,tail", [(129, 3), (1000, 70)])
def test_wide_categorical_sampler_never_draws_an_underflowed_action(lib, A, tail):
    """zero logits and a tail of -200 (f32 probability 0; the tail crosses a 64-column chunk boundary): at the pinned
    top uniforms the f32 CDF ends below u, and the draw must still have non-zero probability"""
    u = uniforms_discrete(SEED_HI, STEP_HI, np.array(ROWS_HEAD0, np.uint32))
    assert np.all(u >= 1.0 - 4.0 / 2 ** 24)
    R = len(ROWS_HEAD0)
    z = np.zeros((1, A), np.float32)
    z[0, -tail:] = -200.0
    heads = dev(np.concatenate([np.zeros((1, 1), np.float32), z], 1))
    tr = _slab(1, R, 1, A)
    env_a = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t, row in enumerate(ROWS_HEAD0):  # one B = 1 launch per row, written to step t
        lib.sample_write_step(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, 1, A, R, t, SEED_HI, STEP_HI, row, 1.0, False,
                              tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], env_a)
    a = tr["actions"][0, :, 0].cpu().numpy().astype(np.int64)
    lp = tr["logp"][0].cpu().numpy()
    ls = log_softmax64(z[0])
    assert np.all((a >= 0) & (a < A - tail)), a
    assert np.all(ls[a] >= math.log(1e-30))
    np.testing.assert_array_less(np.abs(lp - ls[a]), logp_tol(ls[a], A))


def test_wide_categorical_sampler_zero_tail_sweep(lib):
    """A - 1 zero logits and a last logit of -200, every width from 129 to 320: the wave scan adds in a different order
    in every lane, so the f32 CDF of the zero-probability last column can sit one ulp above its neighbour's and be the
    only one above a top uniform; it must not be drawn (the sweep of test_categorical_sampler_never_draws_an_underflowed_
    action, continued past 128)"""
    R = len(ROWS_HEAD0)
    bad = []
    for A in range(129, 321):
        z = np.zeros((1, A), np.float32)
        z[0, -1] = -200.0
        heads = dev(np.concatenate([np.zeros((1, 1), np.float32), z], 1))
        tr = _slab(1, R, 1, A)
        env_a = torch.zeros(1, dtype=torch.int32, device="cuda")
        for t, row in enumerate(ROWS_HEAD0):
            lib.sample_write_step(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, 1, A, R, t, SEED_HI, STEP_HI, row, 1.0, False,
                                  tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], env_a)
        a = tr["actions"][0, :, 0].cpu().numpy().astype(np.int64)
        lp = tr["logp"][0].cpu().numpy()
        ls = log_softmax64(z[0])
        if np.any(ls[a] < math.log(1e-30)):
            bad.append(A)
        np.testing.assert_array_less(np.abs(lp - ls[a]), logp_tol(ls[a], A))
    assert not bad, f"the sampler drew the zero-probability last action for A in {bad}"


@pytest.mark.parametrize("A", [129, 1000])
def test_wide_masked_sampler_vs_float64(lib, A):
    """rows cycle through: only action 0 allowed, only action A - 1, none (uniform draw), a random mask.  A masked-out
    action is never drawn; log-prob = float64 masked log-softmax; deterministic mode: arg-max over the allowed ones"""
    B, seed, step, row0 = 4096, 9, 4, 555 + A
    rng = np.random.default_rng(7 * A)
    logits = (rng.standard_normal((B, A)) * 3).astype(np.float32)
    values = rng.standard_normal(B).astype(np.float32)
    mask = np.zeros((B, A), bool)
    kind = np.arange(B) % 4
    mask[kind == 0, 0] = True
    mask[kind == 1, -1] = True
    r3 = np.flatnonzero(kind == 3)
    mask[r3] = rng.random((len(r3), A)) < 0.5
    mask[r3, 0] = True
    u = uniforms_discrete(seed, step, np.arange(row0, row0 + B, dtype=np.uint32))
    a, lp = run_masked(lib, logits, values, mask, seed=seed, step=step, row0=row0)
    none = kind == 2
    zm = np.where(mask, logits.astype(np.float64), -np.inf)
    ls = log_softmax64(np.where(none[:, None], 0.0, zm))   # all masked: uniform
    check_wide_draw(a, np.exp(ls), u, f"masked A={A}", allowed=np.where(none[:, None], True, mask))
    assert np.all(a[kind == 0] == 0) and np.all(a[kind == 1] == A - 1)
    some = ~none
    want = ls[np.arange(B), a.astype(np.int64)]
    np.testing.assert_array_less(np.abs(lp[some] - want[some]), logp_tol(want[some], A))
    a, _ = run_masked(lib, logits, values, mask, seed=seed, step=step, row0=row0, deterministic=True)
    np.testing.assert_array_equal(a[some], np.argmax(zm, 1)[some])
    np.testing.assert_array_equal(a[none], 0)


TUPLES = [[129, 3], [5, 300, -2, 7], [21] * 8, [200, 1, 1, 1, 1, 1, 1, 2]]


def tuple_logits(rng, hs, B, scale):
    logits = (rng.standard_normal((B, n_params(hs))) * scale).astype(np.float32)
    off = 0
    for h in hs:
        if h < 0:
            logits[:, off - h:off - 2 * h] = rng.uniform(-12, 12, (B, -h))
        off += h if h > 0 else -2 * h
    return logits


@pytest.mark.parametrize("hs", TUPLES, ids=str)
def test_wide_tuple_sampler_vs_float64(lib, hs):
    """Discrete member h draws from counter (step, h, 2, 0), a Box member's normals from (step, k / 2, 3, h); the
    log-prob is the sum of the members' float64 log-probs at the recorded actions; head 0 draws from the stream of the
    single-head sampler; deterministic mode: first maxima / means"""
    B, seed, step, row0 = 4096, 21, 8, 3001
    rng = np.random.default_rng(len(hs) + hs[0])
    logits = tuple_logits(rng, hs, B, 8.0)
    values = rng.standard_normal(B).astype(np.float32)
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    a, lp = run_tuple(lib, logits, values, hs, seed=seed, step=step, row0=row0)
    am, lpm = run_tuple(lib, logits, values, hs, seed=seed, step=step, row0=row0, deterministic=True)
    lp_want, lp_size, lpm_want = np.zeros(B), np.zeros(B), np.zeros(B)
    off = col = 0
    for h_i, h in enumerate(hs):
        if h > 0:
            ls = log_softmax64(logits[:, off:off + h])
            check_wide_draw(a[:, col], np.exp(ls), uniforms_discrete(seed, step, rows, head=h_i), f"member {h_i}")
            got = ls[np.arange(B), a[:, col].astype(np.int64)]
            lp_want += got
            lp_size += np.maximum(1.0, np.abs(got)) + h * 2.0 ** -26 / 2e-6
            np.testing.assert_array_equal(am[:, col], np.argmax(logits[:, off:off + h], 1))
            lpm_want += ls[np.arange(B), np.argmax(logits[:, off:off + h], 1)]
            off, col = off + h, col + 1
        else:
            D = -h
            mu, ls_ = logits[:, off:off + D], logits[:, off + D:off + 2 * D]
            sd = np.clip(np.exp(ls_.astype(np.float64)), 1e-4, 1e4)
            want = mu + sd * normals(seed, step, rows, D, member=h_i)
            got = a[:, col:col + D]
            np.testing.assert_array_less(np.abs(got - want), 1e-5 * (1 + np.abs(want)) + 4e-6 * sd)
            t = normal_logp64(got, mu, ls_)
            lp_want += t.sum(1)
            lp_size += D + np.abs(t).sum(1)
            np.testing.assert_array_equal(am[:, col:col + D], mu)
            lpm_want += normal_logp64(mu, mu, ls_).sum(1)
            off, col = off + 2 * D, col + D
    # per member 2e-6 of its size (+ the log-sum-exp term of logp_tol, folded into lp_size above)
    np.testing.assert_array_less(np.abs(lp - lp_want), 2e-6 * lp_size)
    np.testing.assert_array_less(np.abs(lpm - lpm_want), 2e-6 * lp_size + 1e-5)
    # head 0: the single-head sampler's stream (same kernel for a wide head 0: the same draw in every row)
    a0, _ = run_sampler(lib, np.ascontiguousarray(logits[:, :hs[0]]), values, kind=0, seed=seed, step=step, row0=row0)
    if hs[0] > 128:
        np.testing.assert_array_equal(a0[:, 0], a[:, 0])
    else:
        assert (a0[:, 0] != a[:, 0]).mean() <= 5e-3


def test_wide_box_sampler_vs_float64_box_muller(lib):
    """a single Box(100) (200 parameters) through sf_sample_write_step: same draw rule as the narrow sampler"""
    D, B, seed, step, row0 = 100, 4096, 105, 9, 7100
    rng = np.random.default_rng(100 + D)
    mu = (rng.standard_normal((B, D)) * 2).astype(np.float32)
    log_std = rng.uniform(-12, 12, (B, D)).astype(np.float32)
    params = np.concatenate([mu, log_std], 1)
    values = rng.standard_normal(B).astype(np.float32)
    a, lp = run_sampler(lib, params, values, kind=1, seed=seed, step=step, row0=row0)
    sd = np.clip(np.exp(log_std.astype(np.float64)), 1e-4, 1e4)
    want = mu + sd * normals(seed, step, np.arange(row0, row0 + B, dtype=np.uint32), D)
    np.testing.assert_array_less(np.abs(a - want), 1e-5 * (1 + np.abs(want)) + 4e-6 * sd)
    terms = normal_logp64(a, mu, log_std)
    np.testing.assert_array_less(np.abs(lp - terms.sum(1)), 2e-6 * (D + np.abs(terms).sum(1)))
    a, lp = run_sampler(lib, params, values, kind=1, seed=seed, step=step, row0=row0, deterministic=True)
    np.testing.assert_array_equal(a, mu)


# ------------------------------------------------------------------------------------------------ PPO loss
WIDE_LOSS_CASES = [  # (heads, exploration kind, kl_coeff): kinds 0, 1, 2 in turn (2 on categorical-only lists)
    ([129], 1, 0.2), ([193], 2, 0.0), ([1000], 0, 0.0), ([4096], 2, 0.2), ([-65], 1, 0.0), ([-100], 0, 0.2),
    ([129, 3], 2, 0.2), ([5, 300, -2, 7], 1, 0.2), ([21] * 8, 0, 0.0),
]


def run_loss_dense(lib, params, values, ds, adv_mb, targets_mb, heads, c, index):
    """run_loss with dense_adv = 1: advantages / targets in minibatch order (what V-trace leaves behind), everything
    else read through the index"""
    n, A = params.shape
    kind = 1 if len(heads) == 1 and heads[0] < 0 else 0
    cfg = lib.sf_loss_cfg(clip_ratio=c["clip_ratio"], clip_value=c["clip_value"], value_loss_coeff=c["value_coeff"],
                          exploration_coeff=c["expl_coeff"], kl_coeff=c["kl_coeff"], exploration_kind=c["expl_kind"],
                          action_kind=kind, dense_adv=1)
    if len(heads) > 1:
        cfg.num_heads = len(heads)
        for i, h in enumerate(heads):
            cfg.head_n[i] = int(h)
    m = torch.cat([dev(values)[:, None], dev(params)], 1).contiguous()
    g = torch.zeros_like(m)
    idx = dev(index, torch.int32)
    valids = dev(ds["valids"], torch.bool)
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    out = torch.zeros(16, device="cuda")
    lib.moments(dev(adv_mb), valids[idx.long()].contiguous(), None, n, mom)
    lib.ppo_loss(m[:, 1:], 1 + A, m[:, 0], 1 + A, dev(ds["actions"]), dev(ds["old_logp"]), dev(ds["old_params"]),
                 dev(ds["old_values"]), dev(adv_mb), dev(targets_mb), valids, idx, 0, n, A, cfg, mom, sums, g[:, 1:],
                 g[:, 0])
    lib.loss_scalars(sums, mom, cfg, out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    res = {k: float(o[i]) for i, k in enumerate(SCALARS)}
    res["grad_params"], res["grad_values"] = g[:, 1:].cpu().numpy(), g[:, 0].cpu().numpy()
    return res


@pytest.mark.parametrize("heads,expl_kind,kl_coeff", WIDE_LOSS_CASES, ids=str)
def test_wide_ppo_loss_vs_float64_autograd(lib, heads, expl_kind, kl_coeff):
    """one minibatch and one float64 autograd reference per head list, launched three ways: through a shuffled index
    into a dataset 3x the minibatch, through an offset into a dataset that holds the same rows in minibatch order, and
    with dense (minibatch-order) advantages and targets.  Tolerances: check_loss's, unchanged, at every width."""
    c = _cfg(expl_kind, kl_coeff)
    A = n_params(heads)
    rng = np.random.default_rng(abs(sum(heads)) * 31 + expl_kind)
    n = 2048 if A >= 4096 else 4096
    N = 3 * n
    ds = make_loss_data(rng, heads, N, n)
    index = rng.permutation(N)[:n].astype(np.int32)
    values, g = finish_loss_data(rng, ds, heads, index, c)
    ref = ref_loss(ds["params"], values, g["actions"], g["old_logp"], g["old_params"], g["old_values"], g["adv"],
                   g["targets"], g["valids"], heads, c)
    what = f"{heads} expl={expl_kind} kl={kl_coeff}"
    outs = {}
    outs["index"] = run_loss(lib, ds["params"], values, ds["actions"], ds["old_logp"], ds["old_params"], ds["old_values"],
                             ds["adv"], ds["targets"], ds["valids"], heads, c, index=index)
    offset = 700
    moved = {}
    for k in ("actions", "old_logp", "old_params", "old_values", "adv", "targets", "valids"):
        moved[k] = np.zeros((offset + n + 5,) + ds[k].shape[1:], ds[k].dtype)
        moved[k][offset:offset + n] = g[k]
    outs["offset"] = run_loss(lib, ds["params"], values, moved["actions"], moved["old_logp"], moved["old_params"],
                              moved["old_values"], moved["adv"], moved["targets"], moved["valids"], heads, c,
                              offset=offset)
    outs["dense_adv"] = run_loss_dense(lib, ds["params"], values, ds, g["adv"], g["targets"], heads, c, index)
    for read, out in outs.items():
        check_loss(out, ref, f"{what} {read}")
        assert np.all(out["grad_params"][~g["valids"]] == 0) and np.all(out["grad_values"][~g["valids"]] == 0)
        # samples whose raw ratio is beyond the hard clamp carry no policy gradient: with no exploration / KL term, 0
        if expl_kind == 0 and kl_coeff == 0.0:
            raw = np.exp(ref_logp(ds["params"], g, heads) - g["old_logp"])
            out_hard = (raw > 20.5) | (raw < 0.049)
            assert out_hard.sum() > 100 and np.all(out["grad_params"][out_hard] == 0)
    # the same rows in the same order: the three reads differ in addressing only
    np.testing.assert_array_equal(outs["index"]["grad_params"], outs["offset"]["grad_params"])
    np.testing.assert_array_equal(outs["index"]["grad_params"], outs["dense_adv"]["grad_params"])


# ------------------------------------------------------------------------------------------------ V-trace
def vtrace_inputs(rng, heads, rec, read):
    A = n_params(heads)
    ntraj = 4096 // rec
    n, N = ntraj * rec, 2 * ntraj * rec
    ds = make_loss_data(rng, heads, N, n, edges=False)
    params = ds["params"]
    if read == "index":
        index = rng.permutation(N)[:n].astype(np.int32)
        rows, offset = index, 0
    else:
        index, offset = None, rec * 5
        rows = np.arange(offset, offset + n)
    off = col = 0
    for h in heads:  # Box members: actions drawn from the current policy, as a rollout's are
        if h < 0:
            D = -h
            mu, sd = params[:, off:off + D], np.exp(params[:, off + D:off + 2 * D].astype(np.float64))
            ds["actions"][rows, col:col + D] = (mu + sd * rng.standard_normal((n, D))).astype(np.float32)
        off, col = off + (h if h > 0 else -2 * h), col + (1 if h > 0 else -h)
    g_act = ds["actions"][rows]
    lp = ref_logp(params, dict(old_params=ds["old_params"][rows], actions=g_act), heads)
    shift = rng.standard_normal(n) * 0.5
    k = rng.random(n)
    shift[k < 0.04] = -90.0                                     # logp - old_logp = 90 > 88
    shift[(k >= 0.04) & (k < 0.08)] = 4.0                       # ratio e^-4 < 0.05
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
               d["offset"], d["n"], d["A"], 1 if heads[0] < 0 and len(heads) == 1 else 0, rec, gamma, rho_hat, c_hat, vs,
               adv, head_sizes=heads if len(heads) > 1 else None)
    torch.cuda.synchronize()
    return vs.cpu().numpy(), adv.cpu().numpy()


@pytest.mark.parametrize("read", ["index", "offset"])
@pytest.mark.parametrize("heads", [[129], [1000], [5, 300, -2, 7]], ids=str)
def test_wide_vtrace_vs_float64(lib, heads, read):
    """recurrence 8; inputs and tolerance of test_vtrace_vs_float64: 2e-5 relative; absolute, (2e-5 + eps) times the value
    scale with eps = 2e-6 of the largest sum of the log-prob's term sizes"""
    rec, gamma, rho_hat, c_hat = 8, 0.99, 0.5, 2.0
    rng = np.random.default_rng(rec * 7 + abs(sum(heads)))
    d = vtrace_inputs(rng, heads, rec, read)
    vs, adv = launch_vtrace(lib, d, heads, rec, gamma, rho_hat, c_hat)
    rows = d["rows"]
    rvs, radv = ref_vtrace(d["lp"], d["old_logp"][rows], d["values"], d["rewards"][rows], d["dones"][rows], rec, gamma,
                           rho_hat, c_hat)
    scale = 1.0 + np.abs(d["values"]).max()
    eps = 2e-6 * logp_size(d["params"], d["g_act"], heads).max()
    np.testing.assert_allclose(vs, rvs, rtol=2e-5, atol=(2e-5 + eps) * scale)
    np.testing.assert_allclose(adv, radv, rtol=2e-5, atol=(2e-5 + eps) * scale)


# ------------------------------------------------------------------------------------------------ oracle agreement
def agree_with_oracle(a, a_ref, p, u, what):
    """sampled actions may differ from the oracle's in at most 0.5 % of the rows, and a differing row's draw must lie
    within 1e-5 of its uniform's float64 CDF interval (never exact equality: with A * B ~ 1e7 CDF boundaries a last-bit
    difference between the device and the host expf moves one)"""
    diff = a != a_ref
    assert diff.mean() <= 5e-3, (what, int(diff.sum()))
    r = np.flatnonzero(diff)
    if len(r):
        cdf = np.cumsum(p[r], 1)
        lo = np.concatenate([np.zeros((len(r), 1)), cdf[:, :-1]], 1)
        k = np.arange(len(r))
        ai = a[r].astype(np.int64)
        assert np.all((lo[k, ai] - 1e-5 <= u[r]) & (u[r] < cdf[k, ai] + 1e-5)), what


def test_wide_samplers_vs_oracle(lib):
    B, seed, step, row0 = 4096, 11, 77, 5
    rng = np.random.default_rng(77)
    values = rng.standard_normal(B).astype(np.float32)
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    A = 1000
    logits = (rng.standard_normal((B, A)) * 3).astype(np.float32)
    u = uniforms_discrete(seed, step, rows)
    a, lp = run_sampler(lib, logits, values, kind=0, seed=seed, step=step, row0=row0)
    a_ref, lp_ref = oracle.sample_categorical(logits, seed, step, row0=row0)
    agree_with_oracle(a[:, 0], a_ref, np.exp(log_softmax64(logits)), u, "categorical")
    same = a[:, 0] == a_ref
    np.testing.assert_allclose(lp[same], lp_ref[same], atol=2e-5, rtol=1e-5)
    mask = rng.random((B, A)) < 0.5
    mask[::7] = False
    mask[1::7, 1:] = False
    mask[1::7, 0] = True
    a, lp = run_masked(lib, logits, values, mask, seed=seed, step=step, row0=row0)
    a_ref, lp_ref = oracle.sample_masked(logits, mask, seed, step, row0=row0)
    none = ~mask.any(1)
    zm = np.where(none[:, None], 0.0, np.where(mask, logits.astype(np.float64), -np.inf))
    agree_with_oracle(a, a_ref, np.exp(log_softmax64(zm)), u, "masked")
    same = (a == a_ref) & ~none
    np.testing.assert_allclose(lp[same], lp_ref[same], atol=2e-5, rtol=1e-5)
    hs = [5, 300, -2, 7]
    logits = tuple_logits(rng, hs, B, 3.0)
    logits[:, 305 + 2:305 + 4] = rng.uniform(-2, 1, (B, 2))
    a, lp = run_tuple(lib, logits, values, hs, seed=seed, step=step, row0=row0)
    a_ref, lp_ref = oracle.sample_tuple(logits, hs, seed, step, row0=row0)
    off = col = 0
    same = np.ones(B, bool)
    for h_i, h in enumerate(hs):
        if h > 0:
            p = np.exp(log_softmax64(logits[:, off:off + h]))
            agree_with_oracle(a[:, col], a_ref[:, col], p, uniforms_discrete(seed, step, rows, head=h_i), f"member {h_i}")
            same &= a[:, col] == a_ref[:, col]
            off, col = off + h, col + 1
        else:
            np.testing.assert_allclose(a[:, col:col - h], a_ref[:, col:col - h], rtol=1e-5, atol=1e-5)
            off, col = off - 2 * h, col - h
    np.testing.assert_allclose(lp[same], lp_ref[same], atol=5e-5, rtol=1e-5)


@pytest.mark.parametrize("heads,expl,klc", [([1000], 1, 0.2), ([5, 300, -2, 7], 1, 0.1), ([21] * 8, 2, 0.3)], ids=str)
def test_wide_ppo_loss_vs_oracle(lib, heads, expl, klc):
    """the inputs, tolerances and size-independent properties of test_ppo_loss_vs_oracle_full_size, at 4096 rows"""
    A = n_params(heads)
    rng = np.random.default_rng(A * 7)
    N, n = 16384, 4096
    old_params = rng.standard_normal((N, A)).astype(np.float32)
    cols = []
    for h in heads:
        cols.append(rng.integers(0, h, (N, 1)) if h > 0 else rng.standard_normal((N, -h)))
    actions = np.concatenate(cols, 1).astype(np.float32)
    old_logp = (-rng.random(N) * 2 - 0.3 * len(heads) - math.log(A) + 1.0).astype(np.float32)
    old_values = rng.standard_normal(N).astype(np.float32)
    adv = rng.standard_normal(N).astype(np.float32) * 3 + 0.5
    targets = rng.standard_normal(N).astype(np.float32)
    valids = rng.random(N) > 0.07
    index = rng.permutation(N)[:n].astype(np.int32)
    params = (old_params[index] + 0.3 * rng.standard_normal((n, A))).astype(np.float32)
    values = (old_values[index] + rng.standard_normal(n) * 0.7).astype(np.float32)
    c = dict(clip_ratio=0.1, clip_value=0.5, value_coeff=0.5, expl_coeff=0.01, expl_kind=expl, kl_coeff=klc)
    out = run_loss(lib, params, values, actions, old_logp, old_params, old_values, adv, targets, valids, heads, c,
                   index=index)
    ref = oracle.ppo_loss(params, values, actions[index], old_logp[index], old_params[index], old_values[index],
                          adv[index], targets[index], valids[index], action_kind=0, clip_ratio=0.1, clip_value=0.5,
                          value_loss_coeff=0.5, exploration_coeff=0.01, exploration_kind=expl, kl_coeff=klc,
                          head_sizes=heads if len(heads) > 1 else None)
    assert out["n_valid"] == ref["n_valid"]
    for k in ["policy_loss", "exploration_loss", "kl_loss", "value_loss", "adv_mean", "adv_std", "kl_mean"]:
        assert abs(out[k] - ref[k]) < 1e-6 + 2e-5 * abs(ref[k]), (k, out[k], ref[k])
    assert abs(out["kl_max"] - ref["kl_max"]) < 1e-4 * max(1.0, abs(ref["kl_max"]))
    np.testing.assert_allclose(out["grad_params"], ref["grad_params"], atol=1e-9, rtol=5e-4)
    np.testing.assert_allclose(out["grad_values"], ref["grad_values"], atol=1e-9, rtol=5e-4)
    assert np.all(out["grad_params"][~valids[index]] == 0) and np.all(out["grad_values"][~valids[index]] == 0)
    if all(h > 0 for h in heads):  # every categorical member's gradient sums to ~0 (softmax Jacobian)
        assert np.abs(out["grad_params"].sum(1)).max() < 1e-8


@pytest.mark.parametrize("heads", [[1000], [5, 300, -2, 7]], ids=str)
def test_wide_vtrace_vs_oracle(lib, heads):
    """sf_vtrace on wide parameters against the oracle's recursion fed with float64 ratios: the tolerance of
    test_vtrace_vs_oracle / test_vtrace_tuple_heads_vs_oracle"""
    rec = 8
    rng = np.random.default_rng(rec + abs(sum(heads)))
    d = vtrace_inputs(rng, heads, rec, "offset")
    rows = d["rows"]
    # (keep the ratios inside the clamp: the oracle is handed the ratio itself)
    d["old_logp"][rows] = (d["lp"] + rng.standard_normal(d["n"]) * 0.3).astype(np.float32)
    vs, adv = launch_vtrace(lib, d, heads, rec, 0.99, 0.9, 0.8)
    ratio = np.clip(np.exp(d["lp"] - d["old_logp"][rows]), 0.05, 20.0).astype(np.float32)
    rvs, radv = oracle.vtrace(ratio, d["values"], d["rewards"][rows], d["dones"][rows].astype(np.float32), rec, 0.99,
                              0.9, 0.8)
    np.testing.assert_allclose(vs, rvs, atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(adv, radv, atol=2e-5, rtol=1e-5)
