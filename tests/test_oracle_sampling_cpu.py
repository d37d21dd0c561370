"""The oracle's inverse-CDF samplers never draw an action of zero probability.

The f32 running CDF of a softmax can end a few ulps below 1 while the 24-bit uniform reaches 1 - 2^-24.  A uniform in
that gap used to fall through to the LAST action even when its logit sat ~200 below the maximum (its exp underflows
to 0); torch.multinomial, which the reference samples with, never picks a zero weight.  The rows below are the ones of
seed 11, step 77 whose uniform is within 4 ulps of 1 (found by a scan of all 2^24 rows); the asserts on u pin them."""
import numpy as np
import pytest

import oracle

SEED, STEP = 11, 77
# rows whose head-0 uniform (Philox counter (step, 0, 2, 0)) is >= 1 - 4 * 2^-24
ROWS_HEAD0 = [2645352, 4510266, 4895190, 4940176, 8564387, 13543208, 14296987, 14701484]
# the same for head 1 of a Tuple (counter (step, 1, 2, 0))
ROWS_HEAD1 = [2720876, 3738850, 4481874]


def uniform24(head, row, seed=SEED, step=STEP):
    w = oracle.philox((step, head, 2, 0), (seed, row))
    return (int(w[0]) >> 8) / float(1 << 24)


def probs64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def test_pinned_rows_have_the_top_uniforms():
    for head, rows in ((0, ROWS_HEAD0), (1, ROWS_HEAD1)):
        for r in rows:
            assert uniform24(head, r) >= 1.0 - 4.0 / (1 << 24), (head, r)


def test_categorical_never_samples_an_underflowed_action():
    bad = {}
    for A in range(2, 129):
        z = np.zeros((1, A), np.float32)
        z[0, -1] = -200.0
        p = probs64(z[0])
        for r in ROWS_HEAD0:
            a, lp = oracle.sample_categorical(z, SEED, STEP, row0=r)
            a = int(a[0])
            if p[a] < 1e-30:
                bad.setdefault(A, []).append(r)
            # the log-prob is still the gather at the chosen action
            assert abs(float(lp[0]) - np.log(p[a])) < 2e-6 * max(1.0, abs(np.log(p[a])))
    assert not bad, f"zero-probability action drawn for A in {sorted(bad)}"


@pytest.mark.parametrize("A", [2, 7, 15, 28, 64, 100, 128])
def test_tuple_never_samples_an_underflowed_action(A):
    hs = [A, A]
    z = np.zeros((1, 2 * A), np.float32)
    z[0, A - 1] = z[0, 2 * A - 1] = -200.0
    p = probs64(z[0, :A])
    for r in ROWS_HEAD0 + ROWS_HEAD1:
        a, lp = oracle.sample_tuple(z, hs, SEED, STEP, row0=r)
        a0, a1 = int(a[0, 0]), int(a[0, 1])
        assert p[a0] >= 1e-30 and p[a1] >= 1e-30, (A, r, a0, a1)
        assert abs(float(lp[0]) - (np.log(p[a0]) + np.log(p[a1]))) < 4e-6


def test_fix_keeps_ordinary_draws():
    """outside the underflow gap the draw is the plain inverse CDF: the first k with u < cdf[k] (float64 here; rows
    whose u lies within 1e-5 of a boundary are skipped)"""
    rng = np.random.default_rng(3)
    for A in (2, 9, 33, 128):
        z = (rng.standard_normal((512, A)) * 3).astype(np.float32)
        a, _ = oracle.sample_categorical(z, 5, 9, row0=1000)
        for i in range(512):
            u = uniform24(0, 1000 + i, seed=5, step=9)
            cdf = np.cumsum(probs64(z[i]))
            if np.min(np.abs(cdf - u)) < 1e-5:
                continue
            assert int(a[i]) == int(np.searchsorted(cdf, u, side="right")), (A, i)

