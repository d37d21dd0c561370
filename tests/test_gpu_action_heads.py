"""Action sampling, PPO loss and V-trace kernels (csrc/sf_rl.hip) against INDEPENDENT float64 references.

The expected values here are written from the distributions' definitions and the learner's loss formulas (categorical
inverse CDF, Normal log-density, Box-Muller, PPO clipped surrogate, clipped value loss, entropy / symmetric-KL / KL
terms, the V-trace recursion), in float64 numpy and float64 torch autograd.  Nothing here calls the CPU oracle's
samplers, loss or V-trace: that oracle restates the kernels' own float32 algorithm, so a mistake shared by both would
pass tests/test_gpu_rl_kernels.py.  Only the Philox words are shared; they are pinned by a known-answer test.

Each kernel family is a template over MAXA, picked by A <= 8 / A <= 32 / otherwise (A = number of distribution
parameters: logits, or 2 * D for Box(D)).  Which case reaches which instantiation:

  family            MAXA = 8                       MAXA = 32                      MAXA = 128
  k_sample_write    discrete A in {1,2,7,8}        discrete A in {9,31,32}        discrete A in {33,64,127,128}
                    continuous D in {1,4}          continuous D in {5,16}         continuous D = 64
                    zero-probability sweep 2..8    sweep 9..32                    sweep 33..128
  k_vtrace_ratio    discrete A = 8, cont. D in     discrete A = 32, cont. D = 16  discrete A = 128, cont. D = 64
  (then k_vtrace,   {1,3}                          tuple [3,-2,5] (A = 12)        tuple [100,-3,7,5,1,-1,3] (A = 124)
  one kernel)
  k_ppo_loss        discrete A in {2,7,8},         discrete A in {9,32},          discrete A in {33,128},
                    cont. D in {1,4}               cont. D in {5,16}              cont. D = 64
  k_ppo_loss_md     (no MAXA: the members' statistics kept in the lane, ppo_loss_tuple<true>) tuples [3,-2,5], [7,4,2]
                    (symmetric KL) and an 8-member tuple with Discrete(100)
  masked / tuple    (no MAXA) masked A in {2,33,128}; tuples with 2 and 8 heads

Out of scope: Discrete spaces wider than 128 (every kernel refuses them with SfHipError) and NaN logits."""
import math

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

LN2PI_2 = 0.5 * math.log(2.0 * math.pi)


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda().contiguous()


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


# ------------------------------------------------------------------------------------------------ Philox, vectorised
def philox(c, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) over numpy arrays: counter words c[0..3], key (k0, k1) -> 4 uint32 arrays"""
    shape = np.broadcast(*c, k0, k1).shape
    m32 = np.uint64(0xFFFFFFFF)
    x = [np.broadcast_to(np.asarray(v, np.uint64), shape).copy() for v in c]
    ka = np.broadcast_to(np.asarray(k0, np.uint64), shape).copy()
    kb = np.broadcast_to(np.asarray(k1, np.uint64), shape).copy()
    for _ in range(10):
        p0, p1 = x[0] * np.uint64(0xD2511F53), x[2] * np.uint64(0xCD9E8D57)
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ ka, p1 & m32, (p0 >> np.uint64(32)) ^ x[3] ^ kb, p0 & m32]
        ka, kb = (ka + np.uint64(0x9E3779B9)) & m32, (kb + np.uint64(0xBB67AE85)) & m32
    return [v.astype(np.uint32) for v in x]


def uniforms_discrete(seed, step, rows, head=0):
    """the uniform of a categorical draw: 24 high bits of word 0 of counter (step, head, 2, 0), key (seed, row)"""
    w = philox((step, head, 2, 0), seed, rows)
    return (w[0] >> 8).astype(np.float64) / 2.0 ** 24


def normals(seed, step, rows, D, member=0):
    """float64 Box-Muller normals [len(rows), D] from counter (step, k // 2, 3, member): dims 2j / 2j+1 use words 0,1 / 2,3.
    u1 = f32((w >> 8) + 0.5) / 2^24: the sampler defines u1 through that f32 sum, which rounds to even from 2^23 up
    (u1 can be exactly 1, eps 0); modelling it matters near u1 = 1, where d eps / d u1 is unbounded."""
    eps = np.empty((len(rows), D))
    for j in range((D + 1) // 2):
        w = philox((step, j, 3, member), seed, rows)
        for k, (a, b) in ((2 * j, (0, 1)), (2 * j + 1, (2, 3))):
            if k < D:
                u1 = np.float32((w[a] >> 8).astype(np.float64) + 0.5).astype(np.float64) / 2.0 ** 24
                u2 = (w[b] >> 8).astype(np.float64) / 2.0 ** 24
                eps[:, k] = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return eps


def test_vectorised_philox_matches_the_pinned_one():
    rows = np.array([0, 1, 5, 77777, 2 ** 32 - 1], np.uint32)
    for c in ((0, 0, 0, 0), (77, 1, 2, 0), (9, 31, 3, 7)):
        got = philox(c, 11, rows)
        for i, r in enumerate(rows):
            assert [int(w[i]) for w in got] == [int(x) for x in oracle.philox(c, (11, int(r)))]


# ------------------------------------------------------------------------------------------------ float64 references
def log_softmax64(z):
    z = np.asarray(z, np.float64)
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def check_inverse_cdf(a, p, u, what, allowed=None):
    """a: drawn actions, p: float64 probabilities [B, A], u: float64 uniforms.  The draw must be the first k with
    u < cdf[k]; where u lies within 1e-5 of a cdf boundary (f32 vs f64 rounding), any action whose interval lies within
    1e-5 of u is accepted, and those rows are < 0.5 % of all.  A drawn action never has probability < 1e-30."""
    B = len(a)
    cdf = np.cumsum(p, 1)
    lo = np.concatenate([np.zeros((B, 1)), cdf[:, :-1]], 1)
    want = np.minimum((cdf <= u[:, None]).sum(1), p.shape[1] - 1)
    near = np.abs(cdf - u[:, None]).min(1) < 1e-5
    ai = a.astype(np.int64)
    assert np.all((ai >= 0) & (ai < p.shape[1])), what
    r = np.arange(B)
    in_band = (lo[r, ai] - 1e-5 <= u) & (u < cdf[r, ai] + 1e-5)
    ok = (ai == want) | (near & in_band)
    assert ok.all(), (what, np.flatnonzero(~ok)[:8], ai[~ok][:8], want[~ok][:8], u[~ok][:8])
    assert near.mean() < 5e-3, (what, near.mean())
    assert np.all(p[r, ai] >= 1e-30), (what, "drew an action of zero probability")
    if allowed is not None:
        assert np.all(allowed[r, ai]), (what, "drew a masked-out action")


def logp_tol(want, A):
    """2e-6, relative for |log-prob| > 1, plus A * 2^-26 for the f32 running sum of A exponentials in the log-sum-exp
    (its rounding grows with the number of terms; at A = 127 it alone can reach 2e-6)"""
    return 2e-6 * np.maximum(1.0, np.abs(want)) + A * 2.0 ** -26


def normal_logp64(a, mu, log_std):
    """per-dim Normal log-density with sd = clamp(exp(log_std), 1e-4, 1e4), float64"""
    sd = np.clip(np.exp(np.asarray(log_std, np.float64)), 1e-4, 1e4)
    d = np.asarray(a, np.float64) - np.asarray(mu, np.float64)
    return -(d * d) / (2.0 * sd * sd) - np.log(sd) - LN2PI_2


# ------------------------------------------------------------------------------------------------ sampler launchers
SENT = -7.0


def _slab(B, T, nact, A):
    s = lambda *sh: torch.full(sh, SENT, device="cuda")
    return dict(actions=s(B, T, nact), logits=s(B, T, A), logp=s(B, T), values=s(B, T + 1), ver=s(B, T))


def _read_slab(tr, logits, values, t, version):
    """slab arrays after one sampler launch at step t: the recorded logits / values / version are exact copies and every
    other step keeps its sentinel"""
    o = {k: v.cpu().numpy() for k, v in tr.items()}
    np.testing.assert_array_equal(o["logits"][:, t], logits)
    np.testing.assert_array_equal(o["values"][:, t], values)
    assert np.all(o["ver"][:, t] == version)
    for k in o:
        rest = np.delete(o[k], t, axis=1)
        assert np.all(rest == SENT), f"{k}: a step other than t was written"
    return o["actions"][:, t], o["logp"][:, t]


def run_sampler(lib, logits, values, *, kind, seed, step, row0, deterministic=False, T=3, t=1):
    """sf_sample_write_step on [values | logits | pad] heads (ld > A + 1) -> (actions [B, nact], logp [B], env_a)"""
    B, A = logits.shape
    nact = 1 if kind == 0 else A // 2
    heads = dev(np.concatenate([values[:, None], logits, np.zeros((B, 3), np.float32)], 1))
    ld = heads.shape[1]
    tr = _slab(B, T, nact, A)
    env_a = torch.full((B,), -5, dtype=torch.int32, device="cuda") if kind == 0 else None
    lib.sample_write_step(heads[:, 1:], ld, heads[:, 0], ld, B, A, T, t, seed, step, row0, 42.0, deterministic,
                          tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], env_a, action_kind=kind)
    torch.cuda.synchronize()
    a, lp = _read_slab(tr, logits, values, t, 42.0)
    ea = env_a.cpu().numpy() if env_a is not None else None
    if ea is not None:
        np.testing.assert_array_equal(ea, a[:, 0].astype(np.int32))
    return a, lp


def run_masked(lib, logits, values, mask, *, seed, step, row0, deterministic=False, T=3, t=2):
    B, A = logits.shape
    heads = dev(np.concatenate([values[:, None], logits], 1))
    slab_mask = torch.zeros((B, T + 1, A), dtype=torch.uint8, device="cuda")
    slab_mask[:, t] = dev(mask, torch.uint8)
    mview = slab_mask[:, t]
    tr = _slab(B, T, 1, A)
    env_a = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    lib.sample_write_step_masked(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, mview, mview.stride(0), B, A, T, t, seed, step,
                                 row0, 3.0, deterministic, tr["actions"], tr["logits"], tr["logp"], tr["values"],
                                 tr["ver"], env_a)
    torch.cuda.synchronize()
    a, lp = _read_slab(tr, logits, values, t, 3.0)
    np.testing.assert_array_equal(env_a.cpu().numpy(), a[:, 0].astype(np.int32))
    return a[:, 0], lp


def run_tuple(lib, logits, values, hs, *, seed, step, row0, deterministic=False, T=2, t=0):
    B, A = logits.shape
    nact = sum(1 if h > 0 else -h for h in hs)
    heads = dev(np.concatenate([values[:, None], logits, np.zeros((B, 1), np.float32)], 1))
    ld = heads.shape[1]
    tr = _slab(B, T, nact, A)
    all_discrete = all(h > 0 for h in hs)
    env_a = torch.full((B, len(hs)), -5, dtype=torch.int32, device="cuda") if all_discrete else None
    lib.sample_write_step_tuple(heads[:, 1:], ld, heads[:, 0], ld, B, hs, T, t, seed, step, row0, 5.0, deterministic,
                                tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], env_a)
    torch.cuda.synchronize()
    a, lp = _read_slab(tr, logits, values, t, 5.0)
    if env_a is not None:
        np.testing.assert_array_equal(env_a.cpu().numpy(), a.astype(np.int32))
    return a, lp


# ------------------------------------------------------------------------------------------------ samplers
DISCRETE_A = [1, 2, 7, 8, 9, 31, 32, 33, 64, 127, 128]


@pytest.mark.parametrize("A", DISCRETE_A)
def test_categorical_sampler_vs_float64_inverse_cdf(lib, A):
    """logits at scales 1, 8 and 40 (at 40 most probabilities underflow in f32): the action is the float64 inverse CDF
    of the Philox uniform, the log-prob the float64 log_softmax at it; deterministic mode is the FIRST maximum"""
    B, seed, step, row0 = 8192, 1234 + A, 77, 100003 + 17 * A
    rng = np.random.default_rng(A)
    values = rng.standard_normal(B).astype(np.float32)
    u = uniforms_discrete(seed, step, np.arange(row0, row0 + B, dtype=np.uint32))
    for scale in (1.0, 8.0, 40.0):
        logits = (rng.standard_normal((B, A)) * scale).astype(np.float32)
        a, lp = run_sampler(lib, logits, values, kind=0, seed=seed, step=step, row0=row0)
        ls = log_softmax64(logits)
        check_inverse_cdf(a[:, 0], np.exp(ls), u, f"A={A} scale={scale}")
        want = ls[np.arange(B), a[:, 0].astype(np.int64)]
        np.testing.assert_array_less(np.abs(lp - want), logp_tol(want, A))
    # exact ties: integer logits, many rows with several maxima
    logits = np.round(rng.standard_normal((B, A)) * 1.5).astype(np.float32)
    logits[:64] = 3.0                                                 # all-equal rows: action 0
    a, lp = run_sampler(lib, logits, values, kind=0, seed=seed, step=step, row0=row0, deterministic=True)
    np.testing.assert_array_equal(a[:, 0], np.argmax(logits, 1))
    ls = log_softmax64(logits)
    want = ls[np.arange(B), np.argmax(logits, 1)]
    np.testing.assert_array_less(np.abs(lp - want), logp_tol(want, A))


# the rows of seed 11, step 77 whose uniform is within 4 ulps of 1 - 2^-24 (a scan of all 2^24 rows; the asserts on u pin
# them): there the f32 CDF can end below u
SEED_HI, STEP_HI = 11, 77
ROWS_HEAD0 = [2645352, 4510266, 4895190, 4940176, 8564387, 13543208, 14296987, 14701484]
ROWS_HEAD1 = [2720876, 3738850, 4481874]


def _high_rows_pinned():
    for head, rows in ((0, ROWS_HEAD0), (1, ROWS_HEAD1)):
        u = uniforms_discrete(SEED_HI, STEP_HI, np.array(rows, np.uint32), head=head)
        assert np.all(u >= 1.0 - 4.0 / 2 ** 24), (head, u)


def test_categorical_sampler_never_draws_an_underflowed_action(lib):
    """A - 1 zero logits and a last logit of -200 (its f32 probability underflows to 0): at the top uniforms the f32 CDF
    ends below u, and the draw must still be an action of non-zero probability (torch.multinomial never draws a zero
    weight), with the log-prob of the action drawn"""
    _high_rows_pinned()
    R = len(ROWS_HEAD0)
    bad = []
    for A in range(2, 129):
        z = np.zeros((1, A), np.float32)
        z[0, -1] = -200.0
        heads = dev(np.concatenate([np.zeros((1, 1), np.float32), z], 1))
        tr = _slab(1, R, 1, A)
        env_a = torch.zeros(1, dtype=torch.int32, device="cuda")
        for t, row in enumerate(ROWS_HEAD0):  # one B = 1 launch per row, written to step t
            lib.sample_write_step(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, 1, A, R, t, SEED_HI, STEP_HI, row, 1.0, False,
                                  tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], env_a)
        a = tr["actions"][0, :, 0].cpu().numpy().astype(np.int64)
        lp = tr["logp"][0].cpu().numpy()
        ls = log_softmax64(z[0])
        if np.any(ls[a] < math.log(1e-30)):
            bad.append(A)
        np.testing.assert_allclose(lp, ls[a], rtol=2e-6, atol=2e-6)
    assert not bad, f"the sampler drew the zero-probability last action for A in {bad}"


def test_tuple_sampler_never_draws_an_underflowed_action(lib):
    """the same sweep for a Tuple of two such Discrete(A) heads, at the top uniforms of head 0 and of head 1"""
    _high_rows_pinned()
    rows = ROWS_HEAD0 + ROWS_HEAD1
    bad = []
    for A in range(2, 129):
        z = np.zeros((1, 2 * A), np.float32)
        z[0, A - 1] = z[0, 2 * A - 1] = -200.0
        heads = dev(np.concatenate([np.zeros((1, 1), np.float32), z], 1))
        tr = _slab(1, len(rows), 2, 2 * A)
        for t, row in enumerate(rows):
            lib.sample_write_step_tuple(heads[:, 1:], 1 + 2 * A, heads[:, 0], 1 + 2 * A, 1, [A, A], len(rows), t,
                                        SEED_HI, STEP_HI, row, 1.0, False, tr["actions"], tr["logits"], tr["logp"],
                                        tr["values"], tr["ver"], None)
        a = tr["actions"][0].cpu().numpy().astype(np.int64)
        lp = tr["logp"][0].cpu().numpy()
        ls = log_softmax64(z[0, :A])
        if np.any(ls[a] < math.log(1e-30)):
            bad.append(A)
        np.testing.assert_allclose(lp, ls[a[:, 0]] + ls[a[:, 1]], rtol=2e-6, atol=4e-6)
    assert not bad, f"the Tuple sampler drew a zero-probability action for A in {bad}"


@pytest.mark.parametrize("D", [1, 4, 5, 16, 64])
def test_continuous_sampler_vs_float64_box_muller(lib, D):
    """Box(D): a = mu + clamp(exp(log_std), 1e-4, 1e4) * eps with eps the float64 Box-Muller normal of the same Philox
    words; log_std in [-12, 12] hits both clamp ends.  Tolerance on a: 1e-5 * (1 + |a|), widened by 4e-6 * sd because
    the f32 Box-Muller carries an ABSOLUTE error of a few 1e-7 * sqrt(-2 log u1) in eps (the f32 product 2*pi*u2 is
    rounded before cos), which the scale multiplies and which is unbounded relative to a where cos crosses 0.
    The log-prob is the float64 Normal log-density of the RECORDED action, to 2e-6 of the sum of its terms' sizes."""
    A, B, seed, step, row0 = 2 * D, 4096, 5 + D, 9, 7000 + D
    rng = np.random.default_rng(100 + D)
    mu = (rng.standard_normal((B, D)) * 2).astype(np.float32)
    log_std = rng.uniform(-12, 12, (B, D)).astype(np.float32)
    params = np.concatenate([mu, log_std], 1)
    values = rng.standard_normal(B).astype(np.float32)
    a, lp = run_sampler(lib, params, values, kind=1, seed=seed, step=step, row0=row0)
    sd = np.clip(np.exp(log_std.astype(np.float64)), 1e-4, 1e4)
    assert (sd == 1e-4).any() and (sd == 1e4).any()
    eps = normals(seed, step, np.arange(row0, row0 + B, dtype=np.uint32), D)
    want = mu + sd * eps
    np.testing.assert_array_less(np.abs(a - want), 1e-5 * (1 + np.abs(want)) + 4e-6 * sd)
    terms = normal_logp64(a, mu, log_std)
    np.testing.assert_array_less(np.abs(lp - terms.sum(1)), 2e-6 * (D + np.abs(terms).sum(1)))
    # deterministic: the mean, log-prob at the mean
    a, lp = run_sampler(lib, params, values, kind=1, seed=seed, step=step, row0=row0, deterministic=True)
    np.testing.assert_array_equal(a, mu)
    terms = normal_logp64(mu, mu, log_std)
    np.testing.assert_array_less(np.abs(lp - terms.sum(1)), 2e-6 * (D + np.abs(terms).sum(1)))


@pytest.mark.parametrize("A", [2, 33, 128])
def test_masked_sampler_vs_float64(lib, A):
    """rows cycle through: only the first action allowed, only the last, none (uniform fallback), and a random mask
    with an allowed action whose probability underflows (logit 200 below the allowed maximum).  The draw is the float64
    inverse CDF of the masked distribution and always allowed; log-prob = float64 log_softmax over the allowed ones."""
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
    mask[r3, -1] = True
    mask[r3, 0] = True
    logits[r3, -1] = logits[r3, 0] - 200.0             # allowed, probability 0 in f32
    logits[r3, 0] = np.maximum(logits[r3, 0], logits[r3].max(1))
    u = uniforms_discrete(seed, step, np.arange(row0, row0 + B, dtype=np.uint32))
    a, lp = run_masked(lib, logits, values, mask, seed=seed, step=step, row0=row0)
    none = kind == 2
    zm = np.where(mask, logits.astype(np.float64), -np.inf)
    ls = log_softmax64(np.where(none[:, None], 0.0, zm))   # all masked: uniform
    p = np.exp(ls)
    check_inverse_cdf(a, p, u, f"masked A={A}", allowed=np.where(none[:, None], True, mask))
    some = ~none
    want = ls[np.arange(B), a.astype(np.int64)]
    np.testing.assert_array_less(np.abs(lp[some] - want[some]), logp_tol(want[some], A))
    a, _ = run_masked(lib, logits, values, mask, seed=seed, step=step, row0=row0, deterministic=True)
    np.testing.assert_array_equal(a[some], np.argmax(zm, 1)[some])
    np.testing.assert_array_equal(a[none], 0)


def test_tuple_sampler_eight_members_vs_float64(lib):
    """the maximum of 8 members: Discrete(100), Box(3), Discrete(7), Discrete(5), Discrete(1), Box(1), Discrete(3),
    Discrete(2); each Discrete member h draws from counter (step, h, 2, 0), each Box member's normals from (step, k/2, 3,
    h).  Log-prob = sum of the members' float64 log-probs at the recorded actions.  Deterministic: first maxima / means"""
    hs = [100, -3, 7, 5, 1, -1, 3, 2]
    A = sum(h if h > 0 else -2 * h for h in hs)
    B, seed, step, row0 = 4096, 21, 8, 3001
    rng = np.random.default_rng(8)
    logits = (rng.standard_normal((B, A)) * 8).astype(np.float32)
    values = rng.standard_normal(B).astype(np.float32)
    off, boxes = 0, []
    for h in hs:
        if h < 0:
            logits[:, off - h:off - 2 * h] = rng.uniform(-12, 12, (B, -h))
            boxes.append(off)
        off += h if h > 0 else -2 * h
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    a, lp = run_tuple(lib, logits, values, hs, seed=seed, step=step, row0=row0)
    am, lpm = run_tuple(lib, logits, values, hs, seed=seed, step=step, row0=row0, deterministic=True)
    lp_want, lp_size = np.zeros(B), np.zeros(B)
    lpm_want = np.zeros(B)
    off = col = 0
    for h_i, h in enumerate(hs):
        if h > 0:
            ls = log_softmax64(logits[:, off:off + h])
            check_inverse_cdf(a[:, col], np.exp(ls), uniforms_discrete(seed, step, rows, head=h_i), f"member {h_i}")
            got = ls[np.arange(B), a[:, col].astype(np.int64)]
            lp_want += got
            lp_size += np.maximum(1.0, np.abs(got))
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
    np.testing.assert_array_less(np.abs(lp - lp_want), 2e-6 * lp_size)
    np.testing.assert_array_less(np.abs(lpm - lpm_want), 2e-6 * lp_size + 1e-5)


def test_tuple_sampler_deterministic_ties(lib):
    """exact ties in every Discrete member: torch.argmax's first maximum"""
    hs = [3, 9, 40, 1]
    A, B = sum(hs), 2048
    rng = np.random.default_rng(3)
    logits = np.round(rng.standard_normal((B, A))).astype(np.float32)
    logits[:32] = 1.0
    a, _ = run_tuple(lib, logits, np.zeros(B, np.float32), hs, seed=1, step=2, row0=3, deterministic=True)
    off = np.cumsum([0] + hs)
    want = np.stack([np.argmax(logits[:, off[i]:off[i + 1]], 1) for i in range(len(hs))], 1)
    np.testing.assert_array_equal(a, want)


# ------------------------------------------------------------------------------------------------ PPO loss
SCALARS = ("policy_loss", "exploration_loss", "kl_loss", "value_loss", "kl_mean", "kl_max", "adv_mean", "adv_std",
           "n_valid")


def dist_terms(z, zo, act, heads):
    """float64 torch: per-sample log-prob of act, entropy, KL(new || old), symmetric KL with the uniform prior.
    heads: list of members, n > 0 Discrete(n) logits, -D Box(D) [means | log_std] with sd = clamp(exp, 1e-4, 1e4)"""
    lp = ent = kl = sym = 0.0
    off = col = 0
    for h in heads:
        if h > 0:
            l, lo = torch.log_softmax(z[:, off:off + h], 1), torch.log_softmax(zo[:, off:off + h], 1)
            p = l.exp()
            idx = act[:, col].long()
            lp = lp + l.gather(1, idx[:, None])[:, 0]
            ent = ent - (p * l).sum(1)
            kl = kl + (p * (l - lo)).sum(1)
            lu = math.log(1.0 / h)
            sym = sym + 0.5 * ((p * (l - lu)).sum(1) + ((1.0 / h) * (lu - l)).sum(1))
            off, col = off + h, col + 1
        else:
            D = -h
            mu, sd = z[:, off:off + D], torch.clamp(torch.exp(z[:, off + D:off + 2 * D]), 1e-4, 1e4)
            muo, sdo = zo[:, off:off + D], torch.clamp(torch.exp(zo[:, off + D:off + 2 * D]), 1e-4, 1e4)
            x = act[:, col:col + D]
            lp = lp + (-((x - mu) ** 2) / (2 * sd * sd) - torch.log(sd) - LN2PI_2).sum(1)
            ent = ent + (0.5 + LN2PI_2 + torch.log(sd)).sum(1)
            kl = kl + (torch.log(sdo / sd) + (sd * sd + (mu - muo) ** 2) / (2 * sdo * sdo) - 0.5).sum(1)
            off, col = off + 2 * D, col + D
    return lp, ent, kl, sym


def ref_loss(params, values, actions, old_logp, old_params, old_values, adv, targets, valids, heads, c):
    """float64 autograd of the learner's total loss over the minibatch (rows already gathered)"""
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    z = t(params).requires_grad_(True)
    v = t(values).requires_grad_(True)
    m = torch.tensor(np.asarray(valids, bool))
    lp, ent, kl, sym = dist_terms(z, t(old_params), t(actions).reshape(len(values), -1), heads)
    ratio = torch.clamp(torch.exp(lp - t(old_logp)), 0.05, 20.0)
    a = t(adv)
    mean, n = a[m].mean(), int(m.sum())
    std = a[m].std() if n > 1 else torch.tensor(float("nan"), dtype=torch.float64)
    # the kernel's denominator is fmaxf(std, 1e-7): a NaN std (one valid sample) gives 1e-7
    denom = torch.clamp_min(std, 1e-7) if torch.isfinite(std) else torch.tensor(1e-7, dtype=torch.float64)
    advn = (a - mean) / denom
    hi = 1.0 + c["clip_ratio"]
    lo = 1.0 / hi
    policy = -torch.min(ratio * advn, torch.clamp(ratio, lo, hi) * advn)[m].mean()
    if c["expl_kind"] == 1:
        expl = -c["expl_coeff"] * ent[m].mean()
    elif c["expl_kind"] == 2:
        s = sym[m].mean()
        s = s if torch.isfinite(s) else torch.zeros((), dtype=torch.float64)
        expl = c["expl_coeff"] * torch.clamp(s, max=30.0)
    else:
        expl = torch.zeros((), dtype=torch.float64)
    kl_loss = c["kl_coeff"] * kl[m].mean()
    vo, R = t(old_values), t(targets)
    vclip = vo + torch.clamp(v - vo, -c["clip_value"], c["clip_value"])
    value = c["value_coeff"] * torch.max((v - R) ** 2, (vclip - R) ** 2)[m].mean()
    (policy + expl + kl_loss + value).backward()
    out = dict(policy_loss=policy.item(), exploration_loss=expl.item(), kl_loss=kl_loss.item(), value_loss=value.item(),
               kl_mean=kl[m].mean().item(), kl_max=kl[m].max().item(), adv_mean=mean.item(),
               adv_std=(std.item() if n > 1 else 0.0), n_valid=float(n))  # a NaN variance is reported as 0
    # distance of every sample to the nearest kink of the loss (f32 and f64 may fall on different sides of it)
    with torch.no_grad():
        raw = torch.exp(lp - t(old_logp))
        d = torch.stack([(raw - 0.05).abs() / 0.05, (raw - 20).abs() / 20, (ratio - lo).abs(), (ratio - hi).abs(),
                         ((v - vo).abs() - c["clip_value"]).abs(),
                         torch.where(vclip != v, ((v - R) ** 2 - (vclip - R) ** 2).abs() / (1e-3 + (v - R) ** 2), 1.0)],
                        1).min(1).values
        off = 0
        for h in heads:
            if h < 0:
                e = torch.exp(z[:, off - h:off - 2 * h])
                k = torch.minimum((e / 1e-4).log().abs(), (e / 1e4).log().abs()).min(1).values
                d = torch.minimum(d, k)
            off += h if h > 0 else -2 * h
    out["grad_params"], out["grad_values"] = z.grad.numpy(), v.grad.numpy()
    out["kink"] = d.numpy() < 1e-4
    return out


def run_loss(lib, params, values, actions, old_logp, old_params, old_values, adv, targets, valids, heads, c, index=None,
             offset=0):
    """sf_moments + sf_ppo_loss + sf_loss_scalars; params/values as strided columns of one [n, 1 + A] matrix"""
    n, A = params.shape
    kind = 1 if len(heads) == 1 and heads[0] < 0 else 0
    cfg = lib.sf_loss_cfg(clip_ratio=c["clip_ratio"], clip_value=c["clip_value"], value_loss_coeff=c["value_coeff"],
                          exploration_coeff=c["expl_coeff"], kl_coeff=c["kl_coeff"], exploration_kind=c["expl_kind"],
                          action_kind=kind, dense_adv=0)
    if len(heads) > 1:
        cfg.num_heads = len(heads)
        for i, h in enumerate(heads):
            cfg.head_n[i] = int(h)
    m = torch.cat([dev(values)[:, None], dev(params)], 1).contiguous()
    g = torch.zeros_like(m)
    d = dict(actions=dev(actions), old_logp=dev(old_logp), old_params=dev(old_params), old_values=dev(old_values),
             adv=dev(adv), targets=dev(targets), valids=dev(valids, torch.bool))
    idx = dev(index, torch.int32) if index is not None else None
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    out = torch.zeros(16, device="cuda")
    lib.moments(d["adv"], d["valids"], idx, n, mom, offset=offset)
    lib.ppo_loss(m[:, 1:], 1 + A, m[:, 0], 1 + A, d["actions"], d["old_logp"], d["old_params"], d["old_values"],
                 d["adv"], d["targets"], d["valids"], idx, offset, n, A, cfg, mom, sums, g[:, 1:], g[:, 0])
    lib.loss_scalars(sums, mom, cfg, out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    res = {k: float(o[i]) for i, k in enumerate(SCALARS)}
    res["grad_params"], res["grad_values"] = g[:, 1:].cpu().numpy(), g[:, 0].cpu().numpy()
    return res


def make_loss_data(rng, heads, N, n, edges=True):
    """a dataset of N rows and a minibatch of n current-policy rows, with the loss's edges built in: logit gaps > 100,
    log_std beyond both clamp ends, raw ratios above 20 and below 0.05, ratios inside and outside the clip range,
    v - v_old beyond +-clip_value, invalid samples"""
    A = sum(h if h > 0 else -2 * h for h in heads)
    nact = sum(1 if h > 0 else -h for h in heads)
    old_params = rng.standard_normal((N, A))
    params = rng.standard_normal((n, A)) * 1.5
    actions = np.zeros((N, nact))
    off = col = 0
    for h in heads:
        if h > 0:
            actions[:, col] = rng.integers(0, h, N)
            if edges and h > 1:  # gaps > 100 in 1/8 of the rows, in the current and the old logits
                r = rng.random(n) < 0.125
                params[r, off + rng.integers(0, h)] -= 120.0
                r = rng.random(N) < 0.125
                old_params[r, off + rng.integers(0, h)] -= 110.0
            off, col = off + h, col + 1
        else:
            D = -h
            actions[:, col:col + D] = rng.standard_normal((N, D)) * 1.3
            params[:, off + D:off + 2 * D] = rng.uniform(-1.5, 1.0, (n, D))
            old_params[:, off + D:off + 2 * D] = rng.uniform(-1.5, 1.0, (N, D))
            if edges:  # log_std beyond the clamp: exp < 1e-4 (-12..-9.3) or > 1e4 (9.3..12)
                r = rng.random((n, D)) < 0.08
                params[:, off + D:off + 2 * D][r] = rng.choice([-1, 1], r.sum()) * rng.uniform(9.5, 12.0, r.sum())
            off, col = off + 2 * D, col + D
    return dict(params=params.astype(np.float32), old_params=old_params.astype(np.float32),
                actions=actions.astype(np.float32), old_values=rng.standard_normal(N).astype(np.float32),
                adv=(rng.standard_normal(N) * 2 + 0.3).astype(np.float32), targets=rng.standard_normal(N).astype(np.float32),
                valids=rng.random(N) > 0.1)


def finish_loss_data(rng, ds, heads, rows, c):
    """old log-probs (ratio placement) and current values for the minibatch rows; returns the gathered minibatch.
    Where the current sd is clamped to 1e-4, the row's action is moved to mu + 1e-4 * N(0, 1): a typical action there
    has a log-density of -1e8, and the f32 log-prob of such a row cannot place a ratio."""
    n = len(rows)
    off = col = 0
    for h in heads:
        if h < 0:
            D = -h
            mu, ls = ds["params"][:, off:off + D], ds["params"][:, off + D:off + 2 * D]
            r, k = np.nonzero(np.exp(ls.astype(np.float64)) < 1e-4)
            ds["actions"][rows[r], col + k] = (mu[r, k] + 1e-4 * rng.standard_normal(len(r))).astype(np.float32)
        off, col = off + (h if h > 0 else -2 * h), col + (1 if h > 0 else -h)
    lp, *_ = dist_terms(torch.tensor(ds["params"], dtype=torch.float64), torch.tensor(ds["old_params"][rows], dtype=torch.float64),
                        torch.tensor(ds["actions"][rows], dtype=torch.float64), heads)
    shift = rng.standard_normal(n) * 0.15                       # ratios around 1, in and out of [1/(1+c), 1+c]
    k = rng.random(n)
    shift[k < 0.05] = -math.log(60.0)                           # raw ratio 60 > 20
    shift[(k >= 0.05) & (k < 0.1)] = math.log(60.0)             # raw ratio 1/60 < 0.05
    old_logp = ds.setdefault("old_logp", np.zeros(len(ds["adv"]), np.float32))
    old_logp[rows] = (lp.numpy() + shift).astype(np.float32)
    values = (ds["old_values"][rows] + rng.standard_normal(n) * 1.5 * c["clip_value"]).astype(np.float32)
    g = {k2: ds[k2][rows] for k2 in ("actions", "old_logp", "old_params", "old_values", "adv", "targets", "valids")}
    return values, g


LOSS_CASES = [  # (heads, exploration kind, kl_coeff)
    ([2], 1, 0.0), ([7], 0, 0.2), ([8], 2, 0.3), ([9], 1, 0.1), ([32], 2, 0.0), ([33], 0, 0.3), ([128], 1, 0.2),
    ([128], 2, 0.1),
    ([-1], 1, 0.0), ([-4], 0, 0.2), ([-5], 1, 0.1), ([-16], 0, 0.0), ([-64], 1, 0.3),
    ([3, -2, 5], 1, 0.1), ([7, 4, 2], 2, 0.2), ([100, -3, 7, 5, 1, -1, 3], 1, 0.1),
]


def _cfg(expl_kind, kl_coeff):
    return dict(clip_ratio=0.1, clip_value=0.5, value_coeff=0.5, expl_coeff=0.01 if expl_kind else 0.0,
                expl_kind=expl_kind, kl_coeff=kl_coeff)


def check_loss(out, ref, what):
    """scalars to 1e-6 + 2e-5 relative; kl_max (one sample's f32 KL, nothing averaged) to 1e-4 relative as in
    test_ppo_loss_vs_oracle_full_size; gradients to 5e-4 relative with a floor of 1e-5 of the largest gradient, on the
    samples not within 1e-4 of a kink of the loss (clamps, clip range, min / max switch)"""
    for k in SCALARS:
        tol = 1e-4 * max(1.0, abs(ref[k])) if k == "kl_max" else 1e-6 + 2e-5 * abs(ref[k])
        assert abs(out[k] - ref[k]) <= tol, (what, k, out[k], ref[k])
    keep = ~ref["kink"]
    assert keep.mean() > 0.98, (what, "too many samples at a kink", keep.mean())
    for k in ("grad_params", "grad_values"):
        g, gr = out[k][keep], ref[k][keep]
        np.testing.assert_allclose(g, gr, rtol=5e-4, atol=1e-5 * np.abs(ref[k]).max(), err_msg=f"{what} {k}")


@pytest.mark.parametrize("heads,expl_kind,kl_coeff", LOSS_CASES)
def test_ppo_loss_vs_float64_autograd(lib, heads, expl_kind, kl_coeff):
    """read through a shuffled index into a dataset 3x the minibatch"""
    c = _cfg(expl_kind, kl_coeff)
    rng = np.random.default_rng(abs(sum(heads)) * 31 + expl_kind)
    N, n = 3 * 4096, 4096
    ds = make_loss_data(rng, heads, N, n)
    index = rng.permutation(N)[:n].astype(np.int32)
    values, g = finish_loss_data(rng, ds, heads, index, c)
    out = run_loss(lib, ds["params"], values, ds["actions"], ds["old_logp"], ds["old_params"], ds["old_values"], ds["adv"],
                   ds["targets"], ds["valids"], heads, c, index=index)
    ref = ref_loss(ds["params"], values, g["actions"], g["old_logp"], g["old_params"], g["old_values"], g["adv"],
                   g["targets"], g["valids"], heads, c)
    check_loss(out, ref, f"{heads} expl={expl_kind} kl={kl_coeff}")
    assert np.all(out["grad_params"][~g["valids"]] == 0) and np.all(out["grad_values"][~g["valids"]] == 0)
    # samples whose raw ratio is beyond the hard clamp carry no policy gradient: with no exploration / KL term, exactly 0
    if expl_kind == 0 and kl_coeff == 0.0:
        raw = np.exp(ref_logp(ds["params"], g, heads) - g["old_logp"])
        out_hard = (raw > 20.5) | (raw < 0.049)
        assert out_hard.sum() > 100 and np.all(out["grad_params"][out_hard] == 0)


def logp_size(params, actions, heads):
    """per row, the sum of the sizes of the log-prob's terms (per-member log_softmax, per-dim Normal log-density): the
    f32 log-prob is good to ~2e-6 of it"""
    size = np.zeros(len(params))
    off = col = 0
    for h in heads:
        if h > 0:
            ls = log_softmax64(params[:, off:off + h])
            size += np.abs(ls[np.arange(len(params)), actions[:, col].astype(np.int64)]) + 1.0
            off, col = off + h, col + 1
        else:
            D = -h
            t = normal_logp64(actions[:, col:col + D], params[:, off:off + D], params[:, off + D:off + 2 * D])
            size += np.abs(t).sum(1) + D
            off, col = off + 2 * D, col + D
    return size


def ref_logp(params, g, heads):
    lp, *_ = dist_terms(torch.tensor(params, dtype=torch.float64), torch.tensor(g["old_params"], dtype=torch.float64),
                        torch.tensor(g["actions"], dtype=torch.float64), heads)
    return lp.numpy()


@pytest.mark.parametrize("heads", [[6], [33], [-5]])
@pytest.mark.parametrize("case", ["offset", "one_valid", "constant_adv"])
def test_ppo_loss_edges_vs_float64_autograd(lib, heads, case):
    """read through an offset; a minibatch with one valid sample (std NaN -> denominator 1e-7); constant advantages
    (std 0 -> denominator 1e-7)"""
    c = _cfg(1, 0.1)
    rng = np.random.default_rng(len(case) * 13 + abs(heads[0]))
    N, n, offset = 2048, 1024, 700
    ds = make_loss_data(rng, heads, N, n)
    if case == "one_valid":
        ds["valids"][:] = False
        ds["valids"][offset + 517] = True
    if case == "constant_adv":
        ds["adv"][:] = 0.75
    rows = np.arange(offset, offset + n)
    values, g = finish_loss_data(rng, ds, heads, rows, c)
    out = run_loss(lib, ds["params"], values, ds["actions"], ds["old_logp"], ds["old_params"], ds["old_values"], ds["adv"],
                   ds["targets"], ds["valids"], heads, c, offset=offset)
    ref = ref_loss(ds["params"], values, g["actions"], g["old_logp"], g["old_params"], g["old_values"], g["adv"],
                   g["targets"], g["valids"], heads, c)
    check_loss(out, ref, f"{heads} {case}")


# ------------------------------------------------------------------------------------------------ V-trace
def ref_vtrace(lp, old_logp, values, rewards, dones, rec, gamma, rho_hat, c_hat):
    """float64 V-trace over minibatch order (rows of one trajectory consecutive); lp / old_logp / rewards / dones already
    gathered to that order"""
    ratio = np.clip(np.exp(lp - old_logp.astype(np.float64)), 0.05, 20.0)
    rho, cc = np.minimum(rho_hat, ratio), np.minimum(c_hat, ratio)
    v, r, nd = values.astype(np.float64), rewards.astype(np.float64), 1.0 - dones.astype(np.float64)
    vs, adv = np.zeros_like(v), np.zeros_like(v)
    nxt_v = (v[rec - 1::rec] - r[rec - 1::rec]) / gamma
    nxt_vs = nxt_v.copy()
    for i in reversed(range(rec)):
        sl = slice(i, None, rec)
        ndg = nd[sl] * gamma
        delta = rho[sl] * (r[sl] + ndg * nxt_v - v[sl])
        adv[sl] = rho[sl] * (r[sl] + ndg * nxt_vs - v[sl])
        nxt_vs = v[sl] + delta + ndg * cc[sl] * (nxt_vs - nxt_v)
        vs[sl] = nxt_vs
        nxt_v = v[sl]
    return vs, adv


VTRACE_CASES = [  # (heads, recurrence, rho_hat, c_hat, read through)
    ([8], 1, 1.0, 1.0, "index"), ([8], 32, 0.5, 2.0, "offset"), ([32], 7, 2.0, 0.5, "index"),
    ([128], 32, 1.0, 1.0, "index"), ([128], 7, 0.5, 2.0, "offset"),
    ([-1], 7, 1.0, 1.0, "index"), ([-3], 32, 2.0, 0.5, "offset"), ([-16], 1, 0.5, 2.0, "index"),
    ([-64], 32, 1.0, 1.0, "index"),
    ([3, -2, 5], 7, 0.5, 2.0, "index"), ([100, -3, 7, 5, 1, -1, 3], 32, 2.0, 0.5, "offset"),
]


@pytest.mark.parametrize("heads,rec,rho_hat,c_hat,read", VTRACE_CASES)
def test_vtrace_vs_float64(lib, heads, rec, rho_hat, c_hat, read):
    """ratios clamp(exp(logp64 - old_logp), 0.05, 20) from float64 log-probs, with logp - old_logp > 88 (f32 exp
    overflows) and below log 0.05 in some rows; dones on the first and the last step of some trajectories.
    Tolerance: 2e-5 relative; absolute, (2e-5 + eps) times the value scale, where eps = 2e-6 of the largest sum of the
    log-prob's term sizes is the relative error the ratio inherits from the f32 log-prob (~3e-4 for Box(64), whose
    sequential f32 sum runs over 64 dims; ~1e-5 for a categorical)."""
    rng = np.random.default_rng(rec * 7 + abs(sum(heads)))
    A = sum(h if h > 0 else -2 * h for h in heads)
    ntraj = 4096 // rec
    n, N, gamma = ntraj * rec, 2 * ntraj * rec, 0.99
    ds = make_loss_data(rng, heads, N, n, edges=False)
    params = ds["params"]
    if read == "index":  # minibatch row k reads dataset row index[k], an arbitrary permutation
        index = rng.permutation(N)[:n].astype(np.int32)
        rows, offset = index, 0
    else:
        index, offset = None, rec * 5
        rows = np.arange(offset, offset + n)
    off = col = 0
    for h in heads:  # Box members: actions drawn from the current policy, as a rollout's are (|log-density| ~ D)
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
    vs, adv = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lib.vtrace(dev(params), A, dev(values), 1, dev(ds["actions"]), dev(old_logp), dev(rewards), dev(dones, torch.bool),
               dev(index, torch.int32) if index is not None else None, offset, n, A, 1 if heads[0] < 0 and len(heads) == 1
               else 0, rec, gamma, rho_hat, c_hat, vs, adv, head_sizes=heads if len(heads) > 1 else None)
    torch.cuda.synchronize()
    rvs, radv = ref_vtrace(lp, old_logp[rows], values, rewards[rows], dones[rows], rec, gamma, rho_hat, c_hat)
    scale = 1.0 + np.abs(values).max()
    eps = 2e-6 * logp_size(params, g_act, heads).max()
    np.testing.assert_allclose(vs.cpu().numpy(), rvs, rtol=2e-5, atol=(2e-5 + eps) * scale)
    np.testing.assert_allclose(adv.cpu().numpy(), radv, rtol=2e-5, atol=(2e-5 + eps) * scale)
