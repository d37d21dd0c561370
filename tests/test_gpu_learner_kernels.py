"""The learner-side kernels of sf_rl.hip that prepare a batch, normalise observations and returns, set up a recurrent
minibatch and step the optimiser, called through sample_factory_amd.lib and held to the float64 references of
tests/learner_refs.py (which tests/test_learner_refs_cpu.py holds to the CPU oracle and the `rms` golden) and to the
oracle itself, at the sizes where each kernel changes path: block and wave boundaries, grid caps, scalar tails,
trajectory boundaries of the [E, T+1] slab.  DESIGN.md §4.2 lists which test fixes which entry point."""
import numpy as np
import pytest
import torch

import oracle
from tests import learner_refs as R

pytestmark = pytest.mark.gpu


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


# ================================================================================================ observation normaliser
class Norm:
    """the device state ObservationNormalizer keeps, driven through the three entry points as its update() drives them"""

    def __init__(self, lib, D, mean=None, var=None, count=1.0):
        self.lib, self.D = lib, D
        self.mean = dev(np.zeros(D) if mean is None else mean, torch.float64)
        self.var = dev(np.ones(D) if var is None else var, torch.float64)
        self.count, self.count2 = dev([count], torch.float64), dev([-1.0], torch.float64)
        self.s, self.ss = dev(np.full(D, 7.0)), dev(np.full(D, 7.0))          # stale moments: the entry point clears them
        self.mu, self.rstd = dev(np.full(D, 9.0), torch.float32), dev(np.full(D, 9.0), torch.float32)

    def update(self, buf, u8, stride, n, index=None, offset=0, traj_T=0):
        sub, inv = R.OBS_SCALE[u8]
        self.lib.obsnorm_moments(buf, u8, stride, index, offset, traj_T, n, self.D, sub, inv, self.s, self.ss)
        self.lib.obsnorm_update(self.mean, self.var, self.count, self.count2, self.s, self.ss, n, self.D, self.mu, self.rstd)
        self.count, self.count2 = self.count2, self.count

    def apply(self, buf, u8, stride, n, C=0, HW=0, index=None, offset=0, traj_T=0):
        sub, inv = R.OBS_SCALE[u8]
        out = torch.full((n, self.D), float("nan"), device="cuda")
        self.lib.obsnorm_apply(buf, u8, stride, index, offset, traj_T, n, self.D, C, HW, sub, inv, self.mu, self.rstd, out)
        torch.cuda.synchronize()
        return host(out)

    def check(self, mean, var, count, zero_var_cols=()):
        """count exact; mean, var, mu_tab, rstd_tab rtol 2e-6 (test_rms_golden's bound for the same merge); a column whose
        reference variance is exactly 0 is held to atol 1e-9 (f64 cancellation in sumsq - sum * mean)"""
        assert float(self.count.item()) == count
        np.testing.assert_allclose(host(self.mean), mean, rtol=2e-6, atol=0)
        got_var = host(self.var)
        keep = np.ones(self.D, bool)
        for d in zero_var_cols:
            assert abs(var[d]) <= 1e-20 and abs(got_var[d]) <= 1e-9, (d, var[d], got_var[d])
            keep[d] = False
        np.testing.assert_allclose(got_var[keep], var[keep], rtol=2e-6, atol=0)
        mu, rstd = R.obsnorm_tables(mean, var)
        np.testing.assert_allclose(host(self.mu), mu, rtol=2e-6, atol=0)
        np.testing.assert_allclose(host(self.rstd), rstd, rtol=2e-6, atol=0)


def check_apply(got, xp, norm, C=0, HW=0, what=""):
    """f64 clamp((x' - mu) * rstd) from the kernel's OWN tables; per element 2^-23 (2 (|x'| + |mu|) rstd + 2 |y|); what the
    reference clamps equals +-5 exactly unless it lies within that bound of +-5 (those: under 1 % of the outputs)"""
    y, bound, clamped, near = R.obsnorm_apply(xp, host(norm.mu).astype(np.float64), host(norm.rstd).astype(np.float64), C, HW)
    assert got.shape == y.shape and np.isfinite(got).all(), f"{what}: a sentinel was read"
    err = np.abs(got.astype(np.float64) - y)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: apply max err {err.max():.3e}, max err/bound {worst:.3f}, clamped {int(clamped.sum())}, near {int(near.sum())}")
    assert np.all(err <= bound), f"{what}: err/bound {worst}"
    sure = clamped & ~near
    assert np.array_equal(got[sure], y[sure].astype(np.float32))
    assert near.mean() < 0.01
    return y, sure


OBS_GEOM = [(False, 1, 0, 0), (False, 255, 0, 0), (False, 256, 0, 0), (False, 257, 0, 0), (False, 1000, 0, 0),
            (True, 105, 3, 35)]   # the image: (C, H, W) = (3, 5, 7)


@pytest.mark.parametrize("n", [2, 3, 37, 1000])
@pytest.mark.parametrize("u8,D,C,HW", OBS_GEOM)
def test_obsnorm_update_apply(lib, u8, D, C, HW, n):
    """moments -> update -> apply on rows of stride D + 3 whose padding is a sentinel: a constant column, and two extra
    rows (outside the statistics) whose outlier column must come out as exactly +5 and exactly -5"""
    stride = D + 3
    x = np.concatenate([R.obs_data(u8, D, n, seed=n), R.obs_outlier_rows(u8, D, seed=n + 1)])
    buf = dev(R.obs_pad(x, stride, u8))
    xp = R.obs_prescale(x, np.arange(n + 2), D, *R.OBS_SCALE[u8])
    norm = Norm(lib, D)
    norm.update(buf, u8, stride, n)
    norm.check(*R.obsnorm_update(np.zeros(D), np.ones(D), 1.0, xp[:n]))
    got = norm.apply(buf, u8, stride, n + 2, C, HW)
    y, sure = check_apply(got, xp, norm, C, HW, f"u8={u8} D={D} n={n}")
    pos = (D - 1) if C == 0 else ((D - 1) % HW) * C + (D - 1) // HW
    assert got[n, pos] == 5.0 and got[n + 1, pos] == -5.0 and sure[n, pos] and sure[n + 1, pos]
    assert (got == 5.0).any() and (got == -5.0).any()


@pytest.mark.parametrize("traj", [False, True])
@pytest.mark.parametrize("mode", ["offset", "index"])
@pytest.mark.parametrize("u8,D,C,HW", [(False, 257, 0, 0), (True, 105, 3, 35)])
def test_obsnorm_addressing(lib, u8, D, C, HW, mode, traj):
    """offset > 0 and an index permutation, on flat rows (traj_T = 0) and on the slab [E, T+1, ...] (traj_T = T) whose
    extra row T is a sentinel (NaN / 255): both sides of every trajectory boundary are among the samples"""
    E, T, stride = 5, 4, D + 3
    x = R.obs_data(u8, D, E * T, seed=3)
    flat = R.obs_slab(x, E, T, stride, u8) if traj else R.obs_pad(x, stride, u8)
    buf = dev(flat)
    if mode == "offset":
        index, idx_dev, offset, n = None, None, 3, 13      # dataset rows 3 .. 15: boundaries 3|4, 7|8, 11|12 and row 15
    else:
        index = np.random.default_rng(4).permutation(E * T)
        idx_dev, offset, n = dev(index, torch.int32), 0, E * T
    rows = R.sample_rows(n, index, offset, T if traj else 0)
    ds = R.sample_rows(n, index, offset, 0)
    assert all(e * T + T - 1 in ds and (e + 1) * T in ds for e in range(1, 3))
    xp = R.obs_prescale(flat, rows, D, *R.OBS_SCALE[u8])
    assert np.isfinite(xp).all() and (not u8 or flat[rows, :D].max() <= 100)
    norm = Norm(lib, D)
    norm.update(buf, u8, stride, n, idx_dev, offset, T if traj else 0)
    norm.check(*R.obsnorm_update(np.zeros(D), np.ones(D), 1.0, xp))
    got = norm.apply(buf, u8, stride, n, C, HW, idx_dev, offset, T if traj else 0)
    check_apply(got, xp, norm, C, HW, f"u8={u8} {mode} traj={traj}")


@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("u8,D,C,HW", [(False, 257, 0, 0), (True, 105, 3, 35)])
def test_obsnorm_three_updates(lib, u8, D, C, HW, empty):
    """three merges of different n (count_in / count_out swapped in between) from the normaliser's initial state
    (0, 1, count 1) or from empty statistics (count 0), where the constant column's variance is 0 after the first merge;
    the constant differs from batch to batch, so every batch variance is 0 and the merged one is not"""
    stride, ns = D + 3, (37, 3, 1000)
    xs = [R.obs_data(u8, D, n, seed=20 + i, const_value=(40 + 3 * i if u8 else 0.3 + i)) for i, n in enumerate(ns)]
    buf = dev(R.obs_pad(np.concatenate(xs), stride, u8))
    mean, var, count = (np.zeros(D), np.zeros(D), 0.0) if empty else (np.zeros(D), np.ones(D), 1.0)
    norm = Norm(lib, D, mean, var, count)
    off = 0
    for i, n in enumerate(ns):
        xp = R.obs_prescale(xs[i], np.arange(n), D, *R.OBS_SCALE[u8])
        mean, var, count = R.obsnorm_update(mean, var, count, xp)
        norm.update(buf, u8, stride, n, offset=off)
        norm.check(mean, var, count, zero_var_cols=(0,) if empty and i == 0 else ())
        assert count == (0.0 if empty else 1.0) + sum(ns[:i + 1])
        off += n
    got = norm.apply(buf, u8, stride, ns[2], C, HW, offset=ns[0] + ns[1])
    check_apply(got, xp, norm, C, HW, f"u8={u8} three updates empty={empty}")


def test_obsnorm_update_n0_rebuilds_the_tables(lib):
    """refresh_tables: n = 0 leaves mean / var untouched bit for bit, rebuilds mu / rstd, copies the count; one buffer for
    count_in and count_out is refused"""
    D = 257
    rng = np.random.default_rng(0)
    mean, var = rng.standard_normal(D) * 3, rng.random(D) * 4 + 1e-3
    norm = Norm(lib, D, mean, var, 123.0)
    lib.obsnorm_update(norm.mean, norm.var, norm.count, norm.count2, None, None, 0, D, norm.mu, norm.rstd)
    assert np.array_equal(host(norm.mean), mean) and np.array_equal(host(norm.var), var)
    assert float(norm.count2.item()) == 123.0 and float(norm.count.item()) == 123.0
    norm.check(mean, var, 123.0)
    with pytest.raises(lib.SfHipError):
        lib.obsnorm_update(norm.mean, norm.var, norm.count, norm.count, None, None, 0, D, norm.mu, norm.rstd)


def test_obsnorm_apply_above_the_grid_cap(lib):
    """u8 frames (4, 84, 84), n = 600: n * D = 16.9 M outputs, more than 65536 blocks of 256, so every thread takes a
    second trip of the grid-stride loop; compared in full.  The statistics come from the first 37 frames, where the
    moments grid is (111, 36) and 17 of the 36 sample slices are empty"""
    C, HW, n = 4, 84 * 84, 600
    D = C * HW
    assert n * D > 65536 * 256
    x = np.random.default_rng(5).integers(0, 101, (n, D), dtype=np.uint8)
    buf = dev(x)
    sub, inv = R.OBS_SCALE[True]
    norm = Norm(lib, D)
    norm.update(buf, True, D, 37)
    norm.check(*R.obsnorm_update(np.zeros(D), np.ones(D), 1.0, R.obs_prescale(x, np.arange(37), D, sub, inv)))
    got = norm.apply(buf, True, D, n, C, HW)
    mu, rstd = host(norm.mu).astype(np.float64), host(norm.rstd).astype(np.float64)
    worst = 0.0
    for r0 in range(0, n, 100):
        xp = R.obs_prescale(x, np.arange(r0, r0 + 100), D, sub, inv)
        y, bound, clamped, near = R.obsnorm_apply(xp, mu, rstd, C, HW)
        g = got[r0:r0 + 100]
        err = np.abs(g - y)
        assert np.all(err <= bound), (r0, float((err / bound).max()))
        assert np.array_equal(g[clamped & ~near], y[clamped & ~near].astype(np.float32)) and near.mean() < 0.01
        worst = max(worst, float((err / bound).max()))
    print(f"apply above the cap: max err/bound {worst:.3f}")


# ================================================================================================ recurrent minibatch
CHUNK_SHAPES = [(3, 8, 4, 5, 1), (7, 12, 4, 64, 1), (9, 32, 32, 1024, 1), (5, 6, 1, 3, 5)]   # (E, T, R, S, first chunk k)


@pytest.mark.parametrize("traj", [False, True])
@pytest.mark.parametrize("mode", ["offset", "index"])
@pytest.mark.parametrize("E,T,Rr,S,k", CHUNK_SHAPES)
def test_rnn_chunk_setup(lib, E, T, Rr, S, k, mode, traj):
    """keep_tm and h0, exact: offset mode (offset = k * R, fewer chunks than the dataset has) and index mode (chunk
    starts shuffled, expanded by sf_minibatch_expand), states read from flat rows or from the slab [E, T+1, S] whose row
    T is NaN; the chunks include the last one of a trajectory and the first one of the next, and the done / invalid
    patterns of learner_refs.chunk_case"""
    N, nchunks = E * T, E * T // Rr
    dones, valids, states = R.chunk_case(E, T, Rr, S, k, seed=E + S)
    layout = R.obs_slab(states, E, T, S, False) if traj else states
    st = dev(layout).view(E, T + 1, S) if traj else dev(layout)
    if mode == "offset":
        Cn, offset, index, idx_dev = nchunks - k - 1, k * Rr, None, None
        first = np.arange(k, k + Cn)
    else:
        starts = np.random.default_rng(S).permutation(np.arange(0, N, Rr))
        idx_dev = torch.full((N + 64,), -1, dtype=torch.int32, device="cuda")
        lib.minibatch_expand(dev(starts, torch.int32), idx_dev, N, Rr)
        index = host(idx_dev)[:N]
        np.testing.assert_array_equal(index, R.minibatch_expand(starts, Rr))
        Cn, offset, first = nchunks, 0, starts // Rr
    per_traj = T // Rr
    assert any(c % per_traj == per_traj - 1 and c + 1 in first for c in first)   # a trajectory's last chunk and the next one's first
    assert all(c in first for c in range(k, k + 4))                              # the chunks that carry the patterns
    keep_ref, h0_ref = R.chunk_setup(dones, valids, layout, Rr, Cn, index, offset, T if traj else 0)
    assert np.isfinite(h0_ref).all() and (keep_ref == 0).any() and (keep_ref == 1).any()
    keep, h0 = torch.full((Rr, Cn), -7.0, device="cuda"), torch.full((Cn, S), -7.0, device="cuda")
    lib.rnn_chunk_setup(dev(dones, torch.bool), dev(valids, torch.bool), st, idx_dev, offset, Cn, Rr, keep, h0,
                        traj_T=T if traj else 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(keep), keep_ref)
    np.testing.assert_array_equal(host(h0), h0_ref)


def test_rnn_chunk_setup_rejections(lib):
    E, T, Rr, S, Cn = 3, 8, 4, 5, 4
    d, v = torch.zeros(E * T, dtype=torch.bool, device="cuda"), torch.ones(E * T, dtype=torch.bool, device="cuda")
    flat, slab = torch.zeros((E * T, S), device="cuda"), torch.zeros((E, T + 1, S), device="cuda")
    keep, h0 = torch.zeros((Rr, Cn), device="cuda"), torch.zeros((Cn, S), device="cuda")
    lib.rnn_chunk_setup(d, v, flat, None, 0, Cn, Rr, keep, h0)
    lib.rnn_chunk_setup(d, v, slab, None, 0, Cn, Rr, keep, h0, traj_T=T)
    wide = torch.zeros((E * T, S + 3), device="cuda")
    for bad in [dict(keep_tm=torch.zeros((Cn, Rr + 1), device="cuda")),           # wrong keep_tm shape
                dict(h0=torch.zeros((Cn, S + 1), device="cuda")),                 # wrong h0 shape
                dict(rnn_states=wide[:, :S]),                                     # non-contiguous rnn_states
                dict(rnn_states=slab, traj_T=T + 1),                              # traj_T that is not the slab's
                dict(rnn_states=flat, traj_T=T)]:                                 # ... or no slab at all
        a = dict(rnn_states=flat, keep_tm=keep, h0=h0, traj_T=0)
        a.update(bad)
        with pytest.raises(lib.SfHipError):
            lib.rnn_chunk_setup(d, v, a["rnn_states"], None, 0, Cn, Rr, a["keep_tm"], a["h0"], traj_T=a["traj_T"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_chunks,rec", [(1, 64), (70, 3), (64, 1), (129, 32), (200, 33)])
def test_minibatch_expand(lib, n_chunks, rec):
    """out[j * rec + r] == starts[j] + r, exactly; nothing past experience_size is written"""
    N = n_chunks * rec
    starts = np.random.default_rng(n_chunks).permutation(np.arange(0, N, rec))
    out = torch.full((N + 4096,), -12345, dtype=torch.int32, device="cuda")
    lib.minibatch_expand(dev(starts, torch.int32), out, N, rec)
    torch.cuda.synchronize()
    got = host(out)
    np.testing.assert_array_equal(got[:N].reshape(n_chunks, rec), starts[:, None] + np.arange(rec)[None, :])
    assert np.all(got[N:] == -12345)


# ================================================================================================ batch preparation
def run_mask(lib, pid, pver, actions, logp, my_pid, train_step, max_lag):
    E, T = pid.shape
    na = actions.size // (E * T)
    valids = torch.full((E, T + 1), 7, dtype=torch.uint8, device="cuda")
    flat = torch.full((E * T,), 7, dtype=torch.uint8, device="cuda")
    a, lp = dev(actions, torch.float32), dev(logp, torch.float32)
    ninv = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    lib.valid_mask(dev(pid, torch.int32), dev(pver, torch.float32), valids, a, na, lp, my_pid, train_step, max_lag, ninv,
                   valids_flat=flat)
    torch.cuda.synchronize()
    return valids, flat, a, lp, int(ninv.item())


@pytest.mark.parametrize("norm,boot", R.PREP_FLAGS)
@pytest.mark.parametrize("E,T", R.PREP_SHAPES)
def test_prepare_batch_vs_oracle(lib, E, T, norm, boot):
    """sf_valid_mask -> sf_gae_returns -> sf_moments -> sf_rms_update -> sf_rms_apply chained as Learner._prepare_batch
    chains them, against oracle.prepare_batch (f32, the original's operation order) at the bounds of
    test_prepare_batch_golden, and the advantages against the float64 recursion at twice the oracle's own distance
    from it.  With both flags on the bootstrap term takes the de-normalised value"""
    c = R.prepare_case(E, T)
    o = oracle.prepare_batch(c["rewards"], c["dones"], c["time_outs"], c["values"], c["policy_id"], c["policy_version"],
                             c["actions"], c["log_prob_actions"], my_policy_id=R.PREP_PID, train_step=R.PREP_TRAIN_STEP,
                             max_policy_lag=R.PREP_MAX_LAG, normalize_returns=norm, value_bootstrap=boot, rms=R.PREP_RMS)
    valids, vflat, actions, logp, ninv = run_mask(lib, c["policy_id"], c["policy_version"], c["actions"],
                                                  c["log_prob_actions"], R.PREP_PID, R.PREP_TRAIN_STEP, R.PREP_MAX_LAG)
    assert ninv == o["num_invalids"]
    np.testing.assert_array_equal(host(valids).astype(bool), o["valids"])
    np.testing.assert_array_equal(host(vflat).astype(bool).reshape(E, T), o["valids"][:, :T])
    np.testing.assert_array_equal(host(actions), o["actions"])
    np.testing.assert_array_equal(host(logp), o["log_prob_actions"])
    r, d, to, v = dev(c["rewards"]), dev(c["dones"], torch.bool), dev(c["time_outs"], torch.bool), dev(c["values"])
    st = dev(R.PREP_RMS, torch.float64) if norm else None
    adv, ret = torch.full((E, T), float("nan"), device="cuda"), torch.full((E, T), float("nan"), device="cuda")
    lib.gae_returns(r, d, to, v, valids, st, 0.99, 0.95, boot, adv, ret)
    torch.cuda.synchronize()
    adv64, ret64, rew64 = R.gae(c["rewards"], c["dones"], c["time_outs"], c["values"], o["valids"], 0.99, 0.95,
                                rms=R.PREP_RMS if norm else None, bootstrap=boot)
    e_or, e_64 = np.abs(host(adv) - o["advantages"]).max(), np.abs(host(adv) - adv64).max()
    print(f"E={E} T={T} norm={norm} boot={boot}: adv vs oracle {e_or:.3e}, vs f64 {e_64:.3e} (bound {R.ADV_F64_BOUND:.3e})")
    np.testing.assert_allclose(host(r), o["rewards"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(host(adv), o["advantages"], rtol=0, atol=1e-5)
    assert e_64 <= R.ADV_F64_BOUND
    if norm:
        flat = ret.view(-1)
        mom, new = torch.full((3,), 5.0, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
        lib.moments(flat, None, None, flat.numel(), mom)
        lib.rms_update(st, mom, new)
        lib.rms_apply(flat, new, False)
        torch.cuda.synchronize()
        np.testing.assert_allclose(host(new), o["rms"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(host(ret), o["returns"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("na", [1, 3])
@pytest.mark.parametrize("E,T", [(1, 1), (9, 7), (5, 13), (257, 3)])
def test_valid_mask(lib, E, T, na):
    """E * T = 1, 63, 65 and 771 (partial waves for the ballot count), my_policy_id = 2, versions exactly at the lag
    boundary (invalid: the comparison is strict), one below and one above it"""
    N, my_pid, train_step, max_lag = E * T, 2, 5000, 100
    i = np.arange(N)
    lag = np.array([max_lag, max_lag - 1, max_lag + 1, 0, 17])[i % 5]
    pid = np.where(i % 7 == 3, 0, np.where(i % 11 == 5, 1, my_pid)).astype(np.int32).reshape(E, T)
    pver = (train_step - lag).astype(np.float32).reshape(E, T)
    rng = np.random.default_rng(N)
    actions = rng.standard_normal((N, na)).astype(np.float32)
    logp = (-rng.random(N) - 0.1).astype(np.float32)
    want = R.valid_mask(pid, pver, my_pid, train_step, max_lag)
    ok = want[:, :T].reshape(-1)
    np.testing.assert_array_equal(ok, ((pid == my_pid).reshape(-1)) & (lag < max_lag))
    assert not ok[0] and (N < 5 or (ok[1] and not ok[2] and not ok[3] and ok[4]))
    valids, flat, a, lp, ninv = run_mask(lib, pid, pver, actions, logp, my_pid, train_step, max_lag)
    assert ninv == int((~ok).sum())
    np.testing.assert_array_equal(host(valids), want.astype(np.uint8))          # column T copies column T - 1
    np.testing.assert_array_equal(host(flat), ok.astype(np.uint8))
    got_a, got_lp = host(a), host(lp)
    assert np.all(got_a[~ok] == 0.0) and np.all(got_lp[~ok] == -1.0)
    assert np.array_equal(got_a[ok].view(np.uint32), actions[ok].view(np.uint32))   # kept rows: bit for bit
    assert np.array_equal(got_lp[ok].view(np.uint32), logp[ok].view(np.uint32))


def test_rms_apply_and_moments_above_the_caps(lib):
    """n = 2048 * 256 + 77: the grid-stride loops of k_rms_apply and k_moments take a second trip for 77 elements"""
    n = 2048 * 256 + 77
    rng = np.random.default_rng(11)
    stats = np.array([0.7, 2.5, 1000.0])
    st = dev(stats, torch.float64)
    x = (rng.standard_normal(n) * 4 + 0.5).astype(np.float32)
    t = dev(x)
    lib.rms_apply(t, st, False)
    np.testing.assert_allclose(host(t), R.rms_apply(stats, x), rtol=0, atol=2e-6)
    assert (host(t) == 5.0).any() and (host(t) == -5.0).any()
    z = (rng.standard_normal(n) * 3).astype(np.float32)
    t = dev(z)
    lib.rms_apply(t, st, True)
    np.testing.assert_allclose(host(t), R.rms_apply(stats, z, True), rtol=0, atol=1e-5)
    # moments through an index into a larger dataset, with a validity mask
    N = n + 1000
    data = (rng.standard_normal(N) + 1.0).astype(np.float32)
    valids = rng.random(N) > 0.1
    index = rng.permutation(N)[:n]
    mom = torch.full((3,), 5.0, dtype=torch.float64, device="cuda")
    lib.moments(dev(data), dev(valids, torch.bool), dev(index, torch.int32), n, mom)
    want = R.moments(data[index], valids[index])
    assert host(mom)[2] == want[2]
    np.testing.assert_allclose(host(mom)[:2], want[:2], rtol=1e-12, atol=0)
    # ... and dense, by offset, without a mask
    lib.moments(dev(data), None, None, n, mom, offset=1000)
    want = R.moments(data[1000:])
    assert host(mom)[2] == n
    np.testing.assert_allclose(host(mom)[:2], want[:2], rtol=1e-12, atol=0)


# ================================================================================================ optimiser
P_CAP = 2048 * 256 * 4 + 4 * 256 * 3 + 5   # a second trip of k_adam's grid-stride loop (3 blocks' worth) and a 1-element tail
ADAM = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-6, max_norm=4.0)


def check_adam_step(tp, tm, tv, ref, what):
    """norm, second moment and weights at test_clip_and_adam_vs_oracle's tolerances, against one float64 step from the
    state the device held; the first moment at the reference's operand-magnitude bound"""
    p64, m64, v64, total, coef, m_bound = ref
    em = np.abs(host(tm) - m64)
    print(f"{what}: coef {coef:.4g}, m err/bound {float((em / np.maximum(m_bound, 1e-300)).max()):.3f}, "
          f"p err {np.abs(host(tp) - p64).max():.2e}")
    assert np.all(em <= m_bound)
    np.testing.assert_allclose(host(tv), v64, rtol=4e-5, atol=1e-14)
    np.testing.assert_allclose(host(tp), p64, rtol=2e-7, atol=2e-7)


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("P", [1, 5, 7, 1003, P_CAP])
def test_adam_unpadded_vs_f64_and_oracle(lib, P, clip):
    """P not a multiple of 4 (tail only, tail after vectors) and above the 2048-block cap, grad_scale 0.5, three steps:
    the clip binds on the second (scaled norm 40 against 4) and not on the others; sumsq = None is the no-clip path.
    Each step against the float64 reference AND, as test_clip_and_adam_vs_oracle, against the oracle.  The oracle's first
    moment is held to a tolerance relative to the result, which says nothing where 0.9 m and 0.1 g cancel, so the scaled
    norms 1 / 40 / 0.39 keep the two an order of magnitude apart at every step, as that test's 0.001 / 10 / 0.001 do; the
    float64 check's operand-magnitude bound needs no such care (k_adam forms 1 - beta from the f32 betas of its C
    signature: 1 - beta1 is 2.4e-7 and 1 - beta2 1.3e-5 off the oracle's, relatively, inside these tolerances)"""
    rng = np.random.default_rng(P)
    gs = 0.5
    p = rng.standard_normal(P).astype(np.float32)
    m, v = np.zeros(P, np.float32), np.zeros(P, np.float32)
    tp, tm, tv = dev(p), dev(m), dev(v)
    assert all(t.data_ptr() % 16 == 0 for t in (tp, tm, tv))
    sumsq = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
    for step, norm in ((1, 1.0), (2, 40.0), (3, 0.39)):
        g = R.adam_grad(rng, P, norm, gs)
        tg = dev(g)
        assert tg.data_ptr() % 16 == 0
        before = (host(tp), host(tm), host(tv))
        lib.grad_sumsq(tg, sumsq)
        lib.adam_step(tp, tg, tm, tv, step, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["max_norm"],
                      sumsq if clip else None, grad_scale=gs)
        torch.cuda.synchronize()
        ref = R.adam_step(*before[:1], g, *before[1:], step, ADAM["lr"], max_norm=ADAM["max_norm"], grad_scale=gs, clip=clip)
        total = ref[3]
        assert abs(float(sumsq.sqrt().item()) * gs - total) < 1e-5 * max(1.0, total)
        assert (ref[4] < gs) == (clip and step == 2)
        check_adam_step(tp, tm, tv, ref, f"P={P} clip={clip} step={step}")
        # the oracle's f32 steps, carried in f32 (grad_scale 0.5 is an exact factor on the gradient)
        gc, tot_o = oracle.clip_grad_norm(g * np.float32(gs), ADAM["max_norm"] if clip else 0.0)
        assert abs(float(sumsq.sqrt().item()) * gs - tot_o) < 1e-5 * max(1.0, tot_o)
        p, m, v = oracle.adam_step(p, gc, m, v, step, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"])
        np.testing.assert_allclose(host(tm), m, rtol=2e-5, atol=1e-10)
        np.testing.assert_allclose(host(tv), v, rtol=4e-5, atol=1e-14)
        np.testing.assert_allclose(host(tp), p, rtol=2e-7, atol=2e-7)


@pytest.mark.parametrize("P", [7, 1003])
def test_adam_step_dlr(lib, P):
    """lr read from the device: lr_dev = [3e-4], lr_scale = 0.8 equals sf_adam_step with lr = f32(3e-4) * 0.8; a non-zero
    skip flag leaves weights and moments bit-identical"""
    rng = np.random.default_rng(P)
    p0 = rng.standard_normal(P).astype(np.float32)
    m0, v0 = (rng.standard_normal(P) * 0.01).astype(np.float32), (rng.random(P) * 1e-4).astype(np.float32)
    g = R.adam_grad(rng, P, 40.0, 1.0)
    lr = float(np.float32(3e-4)) * 0.8
    lr_dev = dev([3e-4], torch.float32)
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    tg = dev(g)
    lib.grad_sumsq(tg, sumsq)
    a, b = [dev(x) for x in (p0, m0, v0)], [dev(x) for x in (p0, m0, v0)]
    lib.adam_step_dlr(a[0], tg, a[1], a[2], 3, lr_dev, 0.8, ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["max_norm"], sumsq)
    lib.adam_step(b[0], tg, b[1], b[2], 3, lr, ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["max_norm"], sumsq)
    torch.cuda.synchronize()
    ref = R.adam_step(p0, g, m0, v0, 3, lr, max_norm=ADAM["max_norm"])
    assert ref[4] < 1.0
    check_adam_step(*a, ref, f"dlr P={P}")
    check_adam_step(*b, ref, f"plain P={P}")
    np.testing.assert_allclose(host(a[1]), host(b[1]), rtol=2e-5, atol=1e-10)
    np.testing.assert_allclose(host(a[2]), host(b[2]), rtol=4e-5, atol=1e-14)
    np.testing.assert_allclose(host(a[0]), host(b[0]), rtol=2e-7, atol=2e-7)
    assert not np.array_equal(host(a[0]), p0) and float(lr_dev.item()) == float(np.float32(3e-4))
    for fn in ("dlr", "plain"):
        s = [dev(x) for x in (p0, m0, v0)]
        skip = dev([3], torch.int32)
        if fn == "dlr":
            lib.adam_step_dlr(s[0], tg, s[1], s[2], 3, lr_dev, 0.8, ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["max_norm"],
                              sumsq, skip_flag=skip)
        else:
            lib.adam_step(s[0], tg, s[1], s[2], 3, lr, ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["max_norm"], sumsq,
                          skip_flag=skip)
        torch.cuda.synchronize()
        for got, want in zip(s, (p0, m0, v0)):
            assert np.array_equal(host(got).view(np.uint32), want.view(np.uint32))
        skip.zero_()   # ... and a zero flag lets the step through
        lib.adam_step(s[0], tg, s[1], s[2], 3, lr, ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["max_norm"], sumsq, skip_flag=skip)
        assert np.array_equal(host(s[0]), host(b[0]))


def test_lr_kl_adaptive(lib):
    """KlAdaptiveScheduler.update on the device: expected values in f64, rounded to f32, compared exactly"""
    thr, lr_min, lr_max = np.float32(0.01), np.float32(1e-6), np.float32(1e-2)
    table = [(0.03, 3e-4, "divide"), (0.001, 3e-4, "multiply"), (0.01, 3e-4, "same"), (0.5, 1.2e-6, "floor"),
             (0.0, 9e-3, "cap"), (np.float32(2) * thr, 3e-4, "same"), (np.float32(0.5) * thr, 3e-4, "same"),
             (0.0200001, 3e-4, "divide"), (0.0049999, 3e-4, "multiply")]
    for kl, lr, kind in table:
        want = R.lr_kl_adaptive(kl, lr, thr, lr_min, lr_max)
        lr32 = np.float32(lr)
        assert {"divide": want < lr32 and want > lr_min, "multiply": want > lr32 and want < lr_max, "same": want == lr32,
                "floor": want == lr_min, "cap": want == lr_max}[kind], (kl, lr, kind, want)
        for with_out in (True, False):
            kl_dev, lr_dev = dev([kl], torch.float32), dev([lr], torch.float32)
            out = dev([-1.0], torch.float32) if with_out else None
            lib.lr_kl_adaptive(kl_dev, lr_dev, float(thr), float(lr_min), float(lr_max), out)
            torch.cuda.synchronize()
            assert host(lr_dev)[0] == want, (kl, lr, kind, host(lr_dev)[0], want)
            assert out is None or host(out)[0] == want
            assert host(kl_dev)[0] == np.float32(kl)


def test_tanh_scale_above_the_grid_cap(lib):
    """n * ncols = 1 048 608 > 4096 blocks of 256: 32 elements go round the grid-stride loop a second time.  Against
    float64 at test_tanh_scale_fwd_bwd_vs_torch's tolerances; the other columns of the ld = 8 matrix stay bit-identical"""
    n, ld, col0, D, s = 4096 * 256 // 3 + 11, 8, 1, 3, 2.0
    assert n * D > 4096 * 256
    g = torch.Generator().manual_seed(7)
    x = torch.randn((n, ld), generator=g) * 3
    gy = torch.randn((n, ld), generator=g)
    xr = x.double().requires_grad_(True)
    yr = torch.tanh(xr[:, col0:col0 + D] / s) * s
    yr.backward(gy.double()[:, col0:col0 + D])
    y = x.cuda()
    lib.tanh_scale_fwd(y, ld, n, col0, D, s)
    assert (y.cpu().double()[:, col0:col0 + D] - yr.detach()).abs().max().item() < 1e-6
    assert torch.equal(y.cpu()[:, :col0], x[:, :col0]) and torch.equal(y.cpu()[:, col0 + D:], x[:, col0 + D:])
    gx = gy.cuda()
    lib.tanh_scale_bwd(gx, y, ld, n, col0, D, s)
    assert (gx.cpu().double()[:, col0:col0 + D] - xr.grad[:, col0:col0 + D]).abs().max().item() < 1e-5
    assert torch.equal(gx.cpu()[:, :col0], gy[:, :col0]) and torch.equal(gx.cpu()[:, col0 + D:], gy[:, col0 + D:])
