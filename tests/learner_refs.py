"""Plain numpy float64 references, and the seeded inputs, for the learner-side kernels of sf_rl.hip: the observation
normaliser, the recurrent minibatch setup, batch preparation and the optimiser step.  tests/test_learner_refs_cpu.py
holds them to the CPU oracle and the `rms` golden; tests/test_gpu_learner_kernels.py holds the kernels to them.
Nothing here imports the package under test or touches a GPU."""
import numpy as np

EPS = 1e-5   # running_mean_std.py's _NORM_EPS
CLIP = 5.0   # ... and its clip
U = 2.0 ** -23  # one f32 rounding, relative (the per-element apply bound is written in these)
OBS_SCALE = {True: (50.0, 0.3), False: (0.25, 0.7)}  # (obs_subtract_mean, 1 / obs_scale) of the u8 and the f32 cases

# max |oracle.prepare_batch advantages - gae() below| over every case of PREP_SHAPES x PREP_FLAGS, measured on the host
# by test_learner_refs_cpu.py::test_gae_f64_vs_oracle_prepare_batch (it prints each case): 2.737e-06, at (130, 64) with
# de-normalised values and the time-out bootstrap, where |advantage| reaches 14.5 (f32 spacing 9.5e-07 there: about three
# roundings' worth, accumulated over the 64-step recursion).  The GPU is allowed twice that against the f64 recursion.
ADV_ORACLE_VS_F64 = 2.74e-06
ADV_F64_BOUND = 2 * ADV_ORACLE_VS_F64

PREP_SHAPES = [(1, 1), (63, 31), (65, 33), (70, 37), (130, 64)]
PREP_FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # (normalize_returns, value_bootstrap)
PREP_RMS = (0.7, 2.5, 1000.0)
PREP_TRAIN_STEP, PREP_MAX_LAG, PREP_PID = 5000, 100, 0


# ------------------------------------------------------------------------------------------------ sample addressing
def sample_rows(n, index=None, offset=0, traj_T=0):
    """row of logical sample i: index[i] or offset + i, then dataset row e*T+t -> slab row e*(T+1)+t when traj_T > 0"""
    d = np.asarray(index[:n], np.int64) if index is not None else offset + np.arange(n, dtype=np.int64)
    if traj_T > 0:
        d = (d // traj_T) * (traj_T + 1) + d % traj_T
    return d


# ------------------------------------------------------------------------------------------------ observation normaliser
def obs_prescale(buf, rows, D, sub_mean, inv_scale):
    """x' = (float32(raw) - sub_mean) * inv_scale in f32, promoted to f64.  buf: [rows_total, stride] u8 or f32"""
    raw = buf[rows, :D].astype(np.float32)
    return ((raw - np.float32(sub_mean)) * np.float32(inv_scale)).astype(np.float64)


def obsnorm_update(mean, var, count, xp):
    """Chan merge of the batch xp [n, D] (f64) into (mean[D], var[D], count); batch mean and unbiased variance are
    formed in f64 and rounded to f32 (they are f32 tensors in the original), the merge itself is f64.  n == 0: unchanged"""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    n = 0 if xp is None else xp.shape[0]
    if n == 0:
        return mean.copy(), var.copy(), float(count)
    bm64 = xp.mean(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        bv64 = ((xp - bm64) ** 2).sum(0) / (n - 1.0)
    bm, bv = bm64.astype(np.float32).astype(np.float64), bv64.astype(np.float32).astype(np.float64)
    delta, tot = bm - mean, count + n
    m2 = var * count + bv * n + (delta * delta) * count * n / tot
    return mean + delta * n / tot, m2 / tot, float(tot)


def obsnorm_tables(mean, var):
    """mu = f32(mean), rstd = 1 / sqrt(f32(var) + 1e-5), both returned as f64"""
    mu = np.asarray(mean).astype(np.float32).astype(np.float64)
    rstd = 1.0 / np.sqrt(np.asarray(var).astype(np.float32).astype(np.float64) + EPS)
    return mu, rstd


def obsnorm_apply(xp, mu, rstd, C=0, HW=0):
    """(y, bound, clamped, near): y = clamp((x' - mu) * rstd, +-5) in f64, images (C > 0) written channels-last at
    pos = p * C + c; bound = 2^-23 (2 (|x'| + |mu|) rstd + 2 |y|) per element (four f32 roundings, those of x' and of the
    subtraction amplified by rstd); clamped: the reference clamps the element; near: its unclamped value lies within
    `bound` of +-5, so that f32 may land on either side of the clamp"""
    mu, rstd = np.asarray(mu, np.float64), np.asarray(rstd, np.float64)
    pre = (xp - mu) * rstd
    y = np.clip(pre, -CLIP, CLIP)
    bound = U * (2.0 * (np.abs(xp) + np.abs(mu)) * rstd + 2.0 * np.abs(y))
    clamped = np.abs(pre) >= CLIP
    near = np.abs(np.abs(pre) - CLIP) <= bound
    out = [y, bound, clamped, near]
    if C > 0:
        n = xp.shape[0]
        out = [a.reshape(n, C, HW).transpose(0, 2, 1).reshape(n, C * HW) for a in out]
    return tuple(out)


def obs_data(u8, D, rows, seed, const_value=None):
    """[rows, D] observations: seeded normal columns of different location and scale (u8: integers <= 100); column 0 is
    constant when D >= 2 (batch variance 0), column D - 1 is the outlier column (tight around its centre, see
    obs_outlier_rows)"""
    rng = np.random.default_rng(seed)
    if u8:
        loc, scale = rng.uniform(30, 70, D), rng.uniform(2, 9, D)
        x = np.clip(np.rint(loc + scale * rng.standard_normal((rows, D))), 0, 100)
        x[:, D - 1] = np.clip(np.rint(50 + 2 * rng.standard_normal(rows)), 40, 60)
        if D >= 2:
            x[:, 0] = 42 if const_value is None else const_value
        return x.astype(np.uint8)
    loc, scale = rng.uniform(-2, 2, D), rng.uniform(0.2, 3, D)
    x = loc + scale * rng.standard_normal((rows, D))
    x[:, D - 1] = 0.5 + 0.25 * rng.standard_normal(rows)
    if D >= 2:
        x[:, 0] = 0.3 if const_value is None else const_value
    return x.astype(np.float32)


def obs_outlier_rows(u8, D, seed):
    """two more rows whose outlier column lies far above / far below anything the statistics were built from, so that the
    normalised value leaves +-5 on either side whatever the batch size was"""
    x = obs_data(u8, D, 2, seed)
    x[:, D - 1] = (100, 0) if u8 else (1.0e4, -1.0e4)
    return x


def obs_pad(x, stride, u8):
    """rows of `stride` elements: the observation, then padding no kernel may read (255 among values <= 100, or NaN)"""
    buf = np.full((x.shape[0], stride), 255 if u8 else np.nan, np.uint8 if u8 else np.float32)
    buf[:, :x.shape[1]] = x
    return buf


def obs_slab(x, E, T, stride, u8):
    """the dataset rows x [E*T, D] laid out as the slab [E, T+1, stride]; row T of every trajectory is the sentinel"""
    slab = np.full((E, T + 1, stride), 255 if u8 else np.nan, np.uint8 if u8 else np.float32)
    slab[:, :T, :x.shape[1]] = x.reshape(E, T, -1)
    return slab.reshape(E * (T + 1), stride)


# ------------------------------------------------------------------------------------------------ recurrent minibatch
def minibatch_expand(starts, rec):
    starts = np.asarray(starts, np.int64)
    return (starts[:, None] + np.arange(rec, dtype=np.int64)[None, :]).reshape(-1)


def chunk_setup(dones, valids, states, R, Cn, index=None, offset=0, traj_T=0):
    """keep[t][c] = !(dones[r0 + t] | !valids[r0 + t]), h0[c] = states[r0] with r0 = index[c * R] or offset + c * R;
    dones / valids by flat dataset row, states [rows, S] by dataset row or, with traj_T, by slab row"""
    c = np.arange(Cn, dtype=np.int64)
    if index is not None:
        rows = np.asarray(index, np.int64)[: Cn * R].reshape(Cn, R)
    else:
        rows = offset + c[:, None] * R + np.arange(R, dtype=np.int64)[None, :]
    d, v = np.asarray(dones).astype(bool), np.asarray(valids).astype(bool)
    keep = (~(d[rows] | ~v[rows])).astype(np.float32).T.copy()
    r0 = rows[:, 0]
    if traj_T > 0:
        r0 = (r0 // traj_T) * (traj_T + 1) + r0 % traj_T
    return keep, states[r0].copy()


def chunk_case(E, T, R, S, k, seed):
    """dones, valids [E*T], states [E*T, S]; chunks k .. k+3 carry, in turn, a done at the chunk's first step, a done at
    its last step, an invalid-only step and a step that is both done and invalid"""
    rng = np.random.default_rng(seed)
    N = E * T
    dones, valids = rng.random(N) < 0.1, rng.random(N) > 0.1
    for j in range(4):
        dones[(k + j) * R:(k + j + 1) * R], valids[(k + j) * R:(k + j + 1) * R] = False, True
    dones[k * R] = True
    dones[(k + 1) * R + R - 1] = True
    valids[(k + 2) * R + R // 2] = False
    dones[(k + 3) * R + R // 2], valids[(k + 3) * R + R // 2] = True, False
    states = rng.standard_normal((N, S)).astype(np.float32)
    return dones, valids, states


# ------------------------------------------------------------------------------------------------ batch preparation
def valid_mask(policy_id, policy_version, my_pid, train_step, max_lag):
    """[E, T+1] mask: own policy and (float(train_step) - version) < float(max_lag), strictly; column T copies T-1"""
    pid, ver = np.asarray(policy_id), np.asarray(policy_version, np.float32)
    lag = (np.float32(train_step) - ver).astype(np.float32)
    m = (pid == my_pid) & (lag < np.float32(max_lag))
    return np.concatenate([m, m[:, -1:]], 1)


def gae(rewards, dones, time_outs, values, valids, gamma, lam, rms=None, bootstrap=False):
    """(advantages, returns, rewards) in float64 from f32 inputs, every intermediate f64 (so no rounding is shared with
    the f32 oracle): values de-normalised first when rms is given (clamp +-5, * sqrt(var + 1e-5), + mean), the time-out
    bootstrap r += gamma * v[t] * time_out * done taken from that de-normalised value, then the backward recursion"""
    r = np.asarray(rewards, np.float64).copy()
    d, va = np.asarray(dones, np.float64), np.asarray(valids, np.float64)
    v = np.asarray(values, np.float64)
    g = float(np.float32(gamma))
    gl = float(np.float32(float(gamma) * float(lam)))
    if rms is not None:
        mu, sigma = float(np.float32(rms[0])), np.sqrt(float(np.float32(rms[1])) + EPS)
        v = np.clip(v, -CLIP, CLIP) * sigma + mu
    E, T = r.shape
    if bootstrap:
        r = r + g * v[:, :T] * np.asarray(time_outs, np.float64) * d
    adv = np.zeros((E, T))
    cum = np.zeros(E)
    for t in range(T - 1, -1, -1):
        delta = (r[:, t] - v[:, t]) * va[:, t] + (1.0 - d[:, t]) * g * v[:, t + 1] * va[:, t + 1]
        cum = delta + (gl * va[:, t] + (1.0 - va[:, t])) * cum * (1.0 - d[:, t])
        adv[:, t] = cum
    return adv, adv + va[:, :T] * v[:, :T], r


def moments(x, valids=None):
    x = np.asarray(x, np.float64).reshape(-1)
    if valids is not None:
        x = x[np.asarray(valids).reshape(-1).astype(bool)]
    return np.array([x.sum(), (x * x).sum(), float(x.size)])


def rms_update(stats, x):
    """scalar statistics: obsnorm_update with D = 1"""
    m, v, c = obsnorm_update([stats[0]], [stats[1]], stats[2], np.asarray(x, np.float64).reshape(-1, 1))
    return np.array([m[0], v[0], c])


def rms_apply(stats, x, denormalize=False):
    mu, sigma = float(np.float32(stats[0])), np.sqrt(float(np.float32(stats[1])) + EPS)
    x = np.asarray(x, np.float64)
    return np.clip(x, -CLIP, CLIP) * sigma + mu if denormalize else np.clip((x - mu) / sigma, -CLIP, CLIP)


def prepare_case(E, T, num_actions=2):
    """seeded learner batch: ~5 % dones, a time-out on half of them, ~10 % steps another policy's or too old (the mask
    kernel turns them into invalids), values of scale 2 with entries beyond +-5 so the de-normalisation clamp works"""
    rng = np.random.default_rng(E * 1000 + T)
    c = dict(rewards=rng.standard_normal((E, T)).astype(np.float32), dones=rng.random((E, T)) < 0.05)
    c["time_outs"] = c["dones"] & (rng.random((E, T)) < 0.5)
    c["values"] = (2.0 * rng.standard_normal((E, T + 1))).astype(np.float32)
    c["values"][0, 0], c["values"][-1, -1] = 7.5, -6.25
    c["policy_id"] = np.where(rng.random((E, T)) < 0.05, 1, PREP_PID).astype(np.int32)
    lag = np.where(rng.random((E, T)) < 0.05, PREP_MAX_LAG + rng.integers(0, 3, (E, T)), rng.integers(0, PREP_MAX_LAG, (E, T)))
    c["policy_version"] = (PREP_TRAIN_STEP - lag).astype(np.float32)
    c["actions"] = rng.integers(0, 5, (E, T, num_actions)).astype(np.float32)
    c["log_prob_actions"] = (-rng.random((E, T)) - 0.1).astype(np.float32)
    return c


# ------------------------------------------------------------------------------------------------ optimiser
def adam_step(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-6, max_norm=0.0, grad_scale=1.0, clip=True):
    """(p, m, v, total_norm, coef, m_bound) in float64: ONE step of torch.optim.Adam (no weight decay, no amsgrad) from
    the f32 state handed in, on the gradient g * grad_scale, clipped to max_norm by its global norm when clip
    (coef = min(1, max_norm / (total + 1e-6))).  m_bound = 4 * 2^-23 (|g coef| (1 - b1) + |m|) is what an f32 step may differ
    by in the first moment: g * coef, g - m, * (1 - b1) and the final sum round once each, coef carries the f32 roundings
    of the norm and the division — where (g - m)(1 - b1) cancels m, no bound relative to the result exists"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    total = float(np.sqrt((g * g).sum())) * abs(grad_scale)
    coef = grad_scale * min(max_norm / (total + 1e-6), 1.0) if clip and max_norm > 0 else grad_scale
    g = g * coef
    b1, b2, eps = float(np.float32(b1)), float(np.float32(b2)), float(np.float32(eps))
    m_bound = 4 * U * (np.abs(g) * (1.0 - b1) + np.abs(m))
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + g * g * (1.0 - b2)
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - lr / (1.0 - b1 ** step) * (m / denom), m, v, total, coef, m_bound


def adam_grad(rng, P, scaled_norm, grad_scale):
    """a seeded gradient whose norm after grad_scale is exactly scaled_norm (up to f32 rounding)"""
    g = rng.standard_normal(P)
    return (g * (scaled_norm / (np.sqrt((g * g).sum()) * abs(grad_scale)))).astype(np.float32)


def lr_kl_adaptive(kl, lr, threshold, lr_min, lr_max):
    """KlAdaptiveScheduler.update on f32 operands, in f64, rounded to f32; both comparisons are strict"""
    k, lr, thr = float(np.float32(kl)), float(np.float32(lr)), float(np.float32(threshold))
    if k > 2.0 * thr:
        lr = max(lr / 1.5, float(np.float32(lr_min)))
    if k < 0.5 * thr:
        lr = min(lr * 1.5, float(np.float32(lr_max)))
    return np.float32(lr)
