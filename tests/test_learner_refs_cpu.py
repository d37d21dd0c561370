"""The float64 references of tests/learner_refs.py against what the suite already trusts — the CPU oracle and the `rms`
golden — so that a wrong reference cannot pass as a kernel test in tests/test_gpu_learner_kernels.py.  No GPU."""
import numpy as np
import pytest

from tests import learner_refs as R
import oracle


def test_rms_refs_vs_golden(golden):
    """the scalar running statistics, normalise and de-normalise against the original's recorded run, at the bounds
    test_rms_golden holds the kernels to"""
    g = golden("rms")
    stats = np.array([0.0, 1.0, 1.0])
    for i in range(int(g["num_steps"])):
        stats = R.rms_update(stats, g[f"s{i}_x"])
        np.testing.assert_allclose(stats, g[f"s{i}_stats"], rtol=2e-6)
        np.testing.assert_allclose(R.rms_apply(stats, g[f"s{i}_x"]), g[f"s{i}_normalized"], atol=2e-6, rtol=1e-6)
        np.testing.assert_allclose(R.rms_apply(stats, g[f"s{i}_z"], True), g[f"s{i}_denormalized"], atol=1e-5, rtol=1e-6)
    np.testing.assert_allclose(R.rms_apply(stats, g["eval_x"]), g["eval_normalized"], atol=2e-6)


@pytest.mark.parametrize("n", [2, 3, 37, 1000])
def test_rms_refs_vs_oracle(n):
    rng = np.random.default_rng(n)
    stats = np.array([0.0, 1.0, 1.0])
    for step in range(3):
        x = (rng.standard_normal(n) * 3 + 1.5).astype(np.float32)
        want = oracle.rms_update(stats, x)
        stats = R.rms_update(stats, x)
        np.testing.assert_allclose(stats, want, rtol=2e-6)
        assert stats[2] == want[2]
        np.testing.assert_allclose(R.rms_apply(want, x), oracle.rms_apply(want, x), atol=2e-6)
        z = (rng.standard_normal(n) * 3).astype(np.float32)
        np.testing.assert_allclose(R.rms_apply(want, z, True), oracle.rms_apply(want, z, True), atol=1e-5)
    np.testing.assert_allclose(R.moments(x), [x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum(), n], rtol=1e-15)


@pytest.mark.parametrize("u8,D", [(False, 1), (False, 257), (True, 105)])
def test_obsnorm_refs_columnwise_vs_oracle(u8, D):
    """the vector statistics are the oracle's scalar statistics column by column; three merges of different n, from the
    normaliser's initial state; tables and the applied value against the oracle's f32 normalise"""
    sub, inv = R.OBS_SCALE[u8]
    mean, var, count = np.zeros(D), np.ones(D), 1.0
    cols = sorted({0, D // 2, D - 1})
    per_col = {d: np.array([0.0, 1.0, 1.0]) for d in cols}
    for step, n in enumerate((37, 3, 1000)):
        x = R.obs_data(u8, D, n, seed=10 + step, const_value=(40 + step if u8 else 0.3 + step))
        xp = R.obs_prescale(x, np.arange(n), D, sub, inv)
        mean, var, count = R.obsnorm_update(mean, var, count, xp)
        for d in cols:
            per_col[d] = oracle.rms_update(per_col[d], xp[:, d].astype(np.float32))
            np.testing.assert_allclose([mean[d], var[d], count], per_col[d], rtol=2e-6)
            assert count == per_col[d][2]
    mu, rstd = R.obsnorm_tables(mean, var)
    y, bound, clamped, near = R.obsnorm_apply(xp, mu, rstd)
    for d in cols:
        want = oracle.rms_apply(per_col[d], xp[:, d].astype(np.float32))
        np.testing.assert_allclose(y[:, d], want, atol=2e-6)
    # n == 0 leaves the statistics alone
    m2, v2, c2 = R.obsnorm_update(mean, var, count, None)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var) and c2 == count


def test_obsnorm_ref_layout_bound_and_clamp_census():
    """channels-last position, the outlier rows leaving +-5 on both sides, the constant column's zero batch variance, and
    the share of outputs so close to +-5 that f32 may fall on either side of the clamp: far below 1 %"""
    for u8, D, C, HW in [(False, 257, 0, 0), (False, 1000, 0, 0), (True, 105, 3, 35)]:
        sub, inv = R.OBS_SCALE[u8]
        for n in (2, 3, 37, 1000):
            x = np.concatenate([R.obs_data(u8, D, n, seed=n), R.obs_outlier_rows(u8, D, seed=n + 1)])
            xp = R.obs_prescale(x, np.arange(n + 2), D, sub, inv)
            mean, var, count = R.obsnorm_update(np.zeros(D), np.zeros(D), 0.0, xp[:n])
            assert count == n and abs(var[0]) <= 1e-9          # empty statistics + a constant column: variance 0
            mean, var, count = R.obsnorm_update(np.zeros(D), np.ones(D), 1.0, xp[:n])
            mu, rstd = R.obsnorm_tables(mean, var)
            y, bound, clamped, near = R.obsnorm_apply(xp, mu, rstd, C, HW)
            pos = (D - 1) if C == 0 else ((D - 1) % HW) * C + (D - 1) // HW
            assert y[n, pos] == 5.0 and y[n + 1, pos] == -5.0 and clamped[n, pos] and clamped[n + 1, pos]
            assert near.mean() < 0.01 and bound[~clamped].max() < 1e-4
            if C:
                d = 2 * HW + 11                                   # channel 2, pixel 11 -> position 11 * 3 + 2
                plain = R.obsnorm_apply(xp, mu, rstd)[0]
                assert np.array_equal(y[:, 11 * 3 + 2], plain[:, d])


def test_sample_rows_and_slab():
    E, T = 5, 4
    x = R.obs_data(False, 7, E * T, seed=0)
    slab = R.obs_slab(x, E, T, 9, False)
    rows = R.sample_rows(E * T, traj_T=T)
    np.testing.assert_array_equal(rows, [e * (T + 1) + t for e in range(E) for t in range(T)])
    np.testing.assert_array_equal(slab[rows, :7], x)
    assert np.isnan(slab[np.arange(E) * (T + 1) + T]).all() and np.isnan(slab[:, 7:]).all()
    perm = np.random.default_rng(0).permutation(E * T)
    np.testing.assert_array_equal(R.sample_rows(13, index=perm, traj_T=T), rows[perm[:13]])
    np.testing.assert_array_equal(R.sample_rows(6, offset=3), np.arange(3, 9))


def test_chunk_setup_ref_is_the_named_op_sequence():
    """the torch op sequence the kernel's comment names {arange, gathers, ~, |, transpose, float, index_select}"""
    import torch
    E, T, Rr, S, k = 3, 8, 4, 5, 1
    dones, valids, states = R.chunk_case(E, T, Rr, S, k, seed=0)
    starts = np.random.default_rng(1).permutation(np.arange(0, E * T, Rr))
    index = R.minibatch_expand(starts, Rr)
    np.testing.assert_array_equal(index.reshape(-1, Rr)[:, 0], starts)
    Cn = len(starts)
    keep, h0 = R.chunk_setup(dones, valids, R.obs_slab(states, E, T, S, False), Rr, Cn, index=index, traj_T=T)
    idx = torch.as_tensor(index).view(Cn, Rr)
    d, v = torch.as_tensor(dones)[idx], torch.as_tensor(valids)[idx]
    want_keep = (~(d | ~v)).transpose(0, 1).float().numpy()
    want_h0 = torch.as_tensor(states).index_select(0, idx[:, 0]).numpy()
    np.testing.assert_array_equal(keep, want_keep)
    np.testing.assert_array_equal(h0, want_h0)
    # the patterns the case promises, in chunks k .. k+3
    c = {int(s) // Rr: j for j, s in enumerate(starts)}
    assert keep[0, c[k]] == 0 and keep[1:, c[k]].all()
    assert keep[Rr - 1, c[k + 1]] == 0 and keep[:Rr - 1, c[k + 1]].all()
    assert keep[Rr // 2, c[k + 2]] == 0 and keep[:, c[k + 2]].sum() == Rr - 1
    assert keep[Rr // 2, c[k + 3]] == 0
    # offset mode on the flat layout
    keep2, h02 = R.chunk_setup(dones, valids, states, Rr, 4, offset=k * Rr)
    np.testing.assert_array_equal(h02, states[[4, 8, 12, 16]])
    np.testing.assert_array_equal(keep2[:, 0], [0, 1, 1, 1])


@pytest.mark.parametrize("E,T", R.PREP_SHAPES)
@pytest.mark.parametrize("norm,boot", R.PREP_FLAGS)
def test_gae_f64_vs_oracle_prepare_batch(E, T, norm, boot):
    """mask exact; the f64 recursion within ADV_ORACLE_VS_F64 of the f32 oracle (the figure the GPU bound is twice of);
    returns and the updated statistics follow"""
    c = R.prepare_case(E, T)
    o = oracle.prepare_batch(c["rewards"], c["dones"], c["time_outs"], c["values"], c["policy_id"], c["policy_version"],
                             c["actions"], c["log_prob_actions"], my_policy_id=R.PREP_PID, train_step=R.PREP_TRAIN_STEP,
                             max_policy_lag=R.PREP_MAX_LAG, normalize_returns=norm, value_bootstrap=boot, rms=R.PREP_RMS)
    mask = R.valid_mask(c["policy_id"], c["policy_version"], R.PREP_PID, R.PREP_TRAIN_STEP, R.PREP_MAX_LAG)
    np.testing.assert_array_equal(mask, o["valids"])
    assert o["num_invalids"] == int((~mask[:, :T]).sum())
    if E * T > 1000:
        assert 0.05 < (~mask).mean() < 0.15 and c["dones"].any() and c["time_outs"].any()
        assert (c["time_outs"] & c["dones"]).sum() < c["dones"].sum()
    adv, ret, rew = R.gae(c["rewards"], c["dones"], c["time_outs"], c["values"], mask, 0.99, 0.95,
                          rms=R.PREP_RMS if norm else None, bootstrap=boot)
    err = np.abs(adv - o["advantages"]).max()
    print(f"E={E} T={T} norm={norm} boot={boot}: max|oracle - f64| {err:.3e}, max|adv| {np.abs(adv).max():.3g}")
    assert err <= R.ADV_ORACLE_VS_F64
    np.testing.assert_allclose(rew, o["rewards"], atol=1e-6)
    if norm:
        stats = R.rms_update(R.PREP_RMS, ret)
        np.testing.assert_allclose(stats, o["rms"], rtol=1e-6)
        ret = R.rms_apply(stats, ret)
    np.testing.assert_allclose(ret, o["returns"], atol=1e-5 + R.ADV_ORACLE_VS_F64)


def test_bootstrap_uses_the_denormalised_value():
    """with both flags on, the bootstrap term is gamma * (de-normalised v): one env, one timed-out step, by hand"""
    r, v = np.array([[1.0]], np.float32), np.array([[2.0, 0.5]], np.float32)
    one = np.ones((1, 1), bool)
    adv, ret, rew = R.gae(r, one, one, v, np.ones((1, 2), bool), 0.99, 0.95, rms=(0.7, 2.5, 1000.0), bootstrap=True)
    dv = 2.0 * np.sqrt(float(np.float32(2.5)) + 1e-5) + float(np.float32(0.7))
    np.testing.assert_allclose(rew, 1.0 + float(np.float32(0.99)) * dv, rtol=1e-15)
    np.testing.assert_allclose(adv, rew - dv, rtol=1e-12)


@pytest.mark.parametrize("P", [1, 5, 7, 1003])
def test_adam_ref_vs_oracle(P):
    """three steps of oracle.clip_grad_norm + oracle.adam_step, each against one float64 step from the oracle's own f32
    state: norm and second moment at test_clip_and_adam_vs_oracle's tolerances, the weights at its 1 ulp, the first
    moment at the operand-magnitude bound; the second step's clip binds, the others' does not"""
    rng = np.random.default_rng(P)
    p = rng.standard_normal(P).astype(np.float32)
    m, v = np.zeros(P, np.float32), np.zeros(P, np.float32)
    for step, norm in ((1, 1.0), (2, 40.0), (3, 0.39)):
        g = R.adam_grad(rng, P, norm, 1.0)
        p64, m64, v64, tot64, coef, m_bound = R.adam_step(p, g, m, v, step, 1e-4, max_norm=4.0)
        gc, total = oracle.clip_grad_norm(g, 4.0)
        p, m, v = oracle.adam_step(p, gc, m, v, step, 1e-4, 0.9, 0.999, 1e-6)
        assert abs(tot64 - total) < 1e-5 * max(1.0, total) and (coef < 1.0) == (step == 2)
        assert np.all(np.abs(m - m64) <= m_bound)
        np.testing.assert_allclose(v, v64, rtol=4e-5, atol=1e-14)
        np.testing.assert_allclose(p, p64, rtol=2e-7, atol=2e-7)
    # grad_scale is a factor on the gradient, applied before the norm is taken
    a = R.adam_step(p, g, m, v, 4, 1e-4, max_norm=4.0, grad_scale=0.5)
    b = R.adam_step(p, 0.5 * g.astype(np.float64), m, v, 4, 1e-4, max_norm=4.0)
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x, y, rtol=1e-14)
    # no clip without a norm
    assert R.adam_step(p, g, m, v, 4, 1e-4, max_norm=4.0, grad_scale=0.5, clip=False)[4] == 0.5


def test_lr_kl_adaptive_ref():
    thr = np.float32(0.01)
    f = lambda kl, lr: R.lr_kl_adaptive(kl, lr, thr, 1e-6, 1e-2)
    assert f(0.03, 3e-4) == np.float32(float(np.float32(3e-4)) / 1.5)
    assert f(0.001, 3e-4) == np.float32(float(np.float32(3e-4)) * 1.5)
    assert f(0.01, 3e-4) == np.float32(3e-4)
    assert f(0.5, 1.2e-6) == np.float32(1e-6) and f(0.0, 9e-3) == np.float32(1e-2)
    assert f(np.float32(2) * thr, 3e-4) == np.float32(3e-4) and f(np.float32(0.5) * thr, 3e-4) == np.float32(3e-4)
