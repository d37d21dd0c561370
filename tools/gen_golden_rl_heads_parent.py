"""Fixture of the action-head kernels of csrc/sf_rl.hip (PPO loss, V-trace ratio, the four samplers):
    python tools/gen_golden_rl_heads_parent.py [out.npz]
draws every input on the HOST from numpy.random.default_rng(seed) (identical on every machine), runs the entry points
and stores their OUTPUTS per case.  The committed tests/golden/rl_heads_parent.npz was written by commit PARENT, the one
before the kernels' repeated arithmetic was folded into shared helpers: tests/test_gpu_rl_heads_parent_bits.py asks for
bit equality with it (sf_rl.hip is compiled with -ffp-contract=off, so an expression moved into an inlined helper with
its operation order unchanged gives the same bits).  Needs a GPU.

The double sums of the loss are atomics, one per block and slot.  Lane-per-row cases have n <= 256 rows (one block);
wave-per-row cases have n = 7 (two blocks of four rows, the second partial: 0 + a + b is the same in either order).

    python tools/gen_golden_rl_heads_parent.py --second [out.npz]
writes the second fixture, tests/golden/rl_heads_parent2.npz, from the case lists MASKED_LOSS_CASES, MASKED_VTRACE_CASES
and CONSISTENCY_CASES: the entry points that came after the first fixture (sf_ppo_loss_masked, sf_vtrace_masked,
sf_consistency_loss).  Commit PARENT2 wrote it; tests/test_gpu_rl_heads_parent2_bits.py asks for bit equality with it, so
that a later rewrite of these kernels that keeps the operation order can be held to their bits as well."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARENT = "dea0c8f"  # "Sample Tuple action spaces under an action mask on native samplers"
PARENT2 = "5652c55"  # "Report env-defined episode statistics: true_objective and extra stats"
SENT = -7.0         # what a sampler's slab holds before the launch: every step but t must still hold it after
CLIP_RATIO, CLIP_VALUE = 0.1, 0.5


def n_params(heads):
    return sum(h if h > 0 else -2 * h for h in heads)


def n_cols(heads):
    return sum(1 if h > 0 else -h for h in heads)


def logp64(params, actions, heads, mask=None):
    """float64 log-prob of the recorded actions (places the ratios; not a reference for the outputs); mask: -1e9 on the
    masked-out columns of a Discrete member, rounded to f32 as the kernels add it (an all-masked member is uniform)"""
    p, a = params.astype(np.float64), actions.astype(np.float64)
    lp = np.zeros(len(p))
    off = col = 0
    for h in heads:
        if h > 0:
            z = p[:, off:off + h]
            if mask is not None:
                z = np.where(mask[:, off:off + h] != 0, z, (z - 1e9).astype(np.float32).astype(np.float64))
            z = z - z.max(1, keepdims=True)
            ls = z - np.log(np.exp(z).sum(1, keepdims=True))
            lp += ls[np.arange(len(p)), a[:, col].astype(np.int64)]
            off, col = off + h, col + 1
        else:
            D = -h
            mu, sd = p[:, off:off + D], np.clip(np.exp(p[:, off + D:off + 2 * D]), 1e-4, 1e4)
            d = a[:, col:col + D] - mu
            lp += (-(d * d) / (2 * sd * sd) - np.log(sd) - 0.5 * math.log(2 * math.pi)).sum(1)
            off, col = off + 2 * D, col + D
    return lp


def draw_dists(rng, heads, N, n):
    """(params [n, A], old_params [N, A], actions [N, cols]): gaps > 100 in some logits, log_std beyond both clamp ends"""
    A = n_params(heads)
    old_params = rng.standard_normal((N, A))
    params = rng.standard_normal((n, A)) * 1.5
    actions = np.zeros((N, n_cols(heads)))
    off = col = 0
    for h in heads:
        if h > 0:
            actions[:, col] = rng.integers(0, h, N)
            if h > 1:
                params[rng.random(n) < 0.125, off + rng.integers(0, h)] -= 120.0
            off, col = off + h, col + 1
        else:
            D = -h
            actions[:, col:col + D] = rng.standard_normal((N, D)) * 1.3
            params[:, off + D:off + 2 * D] = rng.uniform(-1.5, 1.0, (n, D))
            old_params[:, off + D:off + 2 * D] = rng.uniform(-1.5, 1.0, (N, D))
            r = rng.random((n, D)) < 0.08
            r[:6] = False  # (the rows whose ratio and value step the loss cases place: |log-prob| stays small there)
            params[:, off + D:off + 2 * D][r] = rng.choice([-1, 1], r.sum()) * rng.uniform(9.5, 12.0, r.sum())
            off, col = off + 2 * D, col + D
    return params.astype(np.float32), old_params.astype(np.float32), actions.astype(np.float32)


def dev(x, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------------- PPO loss
# (name, entry point, heads, n, exploration kind, kl_coeff, read through, dense_adv, old_values_T)
LOSS_CASES = [
    ("loss_d7_e0", "cfg", [7], 70, 0, 0.0, "index", 0, 0),
    ("loss_d7_e1", "cfg", [7], 70, 1, 0.2, "offset", 0, 0),
    ("loss_d32_e2", "cfg", [32], 70, 2, 0.3, "index", 1, 0),
    ("loss_d128_e1", "cfg", [128], 20, 1, 0.1, "offset", 0, 5),
    ("loss_d128_e2", "cfg", [128], 20, 2, 0.0, "index", 0, 0),
    ("loss_box3_e1", "cfg", [-3], 70, 1, 0.2, "index", 0, 0),
    ("loss_box3_e0", "cfg", [-3], 70, 0, 0.0, "offset", 1, 5),
    ("loss_box70_wide", "cfg", [-70], 7, 1, 0.2, "index", 0, 0),
    ("loss_cfg_3_b2_5", "cfg", [3, -2, 5], 70, 1, 0.0, "offset", 0, 5),
    ("loss_heads_3_b2_5", "heads", [3, -2, 5], 70, 1, 0.1, "index", 0, 0),
    ("loss_heads_7_4_2_symkl", "heads", [7, 4, 2], 70, 2, 0.2, "index", 0, 0),
    ("loss_heads_11", "heads", [3] * 9 + [-2, 4], 70, 1, 0.1, "offset", 0, 0),
    ("loss_heads_11_symkl", "heads", [3] * 11, 70, 2, 0.0, "index", 1, 0),
    ("loss_heads_129", "heads", [129], 7, 2, 0.1, "index", 0, 0),
    ("loss_heads_100_100", "heads", [100, 100], 7, 1, 0.2, "offset", 0, 0),
    ("loss_heads_10_wide", "heads", [3] * 9 + [130], 7, 2, 0.1, "index", 0, 0),
    ("loss_heads_130_b2_3", "heads", [130, -2, 3], 7, 1, 0.1, "index", 0, 5),
]
# the same fields and mask_T: sf_ppo_loss_masked (k_masked_ppo_loss_md / _mh / _wide); the datasets have 2 n + 3 rows, so
# draw_mask's all-masked member rows are among the minibatch's
MASKED_LOSS_CASES = [
    ("mloss_d7_flat", "masked", [7], 70, 1, 0.2, "index", 0, 0, 0),
    ("mloss_d7_slab", "masked", [7], 70, 0, 0.0, "offset", 0, 5, 5),
    ("mloss_3_b2_5_flat", "masked", [3, -2, 5], 70, 1, 0.1, "offset", 1, 0, 0),
    ("mloss_3_b2_5_slab", "masked", [3, -2, 5], 70, 1, 0.0, "index", 0, 5, 5),
    ("mloss_11_flat", "masked", [3] * 9 + [-2, 4], 70, 1, 0.1, "index", 0, 0, 0),
    ("mloss_11_slab", "masked", [3] * 9 + [-2, 4], 70, 0, 0.2, "offset", 0, 0, 5),
    ("mloss_130_b2_3_flat", "masked", [130, -2, 3], 7, 1, 0.1, "offset", 0, 0, 0),
    ("mloss_130_b2_3_slab", "masked", [130, -2, 3], 7, 1, 0.2, "index", 0, 5, 5),
]


def allowed_actions(mask, heads, actions):
    """in place: a recorded action of a Discrete member that its mask slice rules out becomes the slice's first allowed
    one, as a sampler under that mask would never have drawn it (an all-masked slice keeps what was drawn)"""
    off = col = 0
    for h in heads:
        if h > 0:
            sl = mask[:, off:off + h]
            a = actions[:, col].astype(np.int64)
            bad = (sl[np.arange(len(sl)), a] == 0) & sl.any(1)
            actions[bad, col] = sl[bad].argmax(1)
        off, col = off + (h if h > 0 else -2 * h), col + (1 if h > 0 else -h)


def all_masked_member(mask_row, heads):
    """whether a Discrete member's whole slice of the mask row is zero"""
    off, hit = 0, False
    for h in heads:
        hit = hit or (h > 0 and not mask_row[off:off + h].any())
        off += h if h > 0 else -2 * h
    return hit


def slab_mask(mask, mask_T):
    """the device mask of dataset rows [N, A]: flat (mask_T = 0), or inside the slab's [E, mask_T + 1, A] array whose
    last step of every env holds ones the kernels must never read for these rows"""
    if not mask_T:
        return dev(mask)
    E = -(-len(mask) // mask_T)
    rows = np.arange(len(mask))
    slab = np.ones((E * (mask_T + 1), mask.shape[1]), np.uint8)
    slab[rows + rows // mask_T] = mask  # dataset row e * T + t -> e * (T + 1) + t
    return dev(slab.reshape(E, mask_T + 1, -1))


def run_loss_case(lib, case):
    """a case of LOSS_CASES, or of MASKED_LOSS_CASES (one more field, mask_T: sf_ppo_loss_masked under draw_mask's rows,
    flat [N, A] with mask_T = 0 or the slab's [E, mask_T + 1, A] read in place)"""
    import ctypes as C
    import torch
    name, entry, heads, n, expl_kind, kl_coeff, read, dense_adv, ov_T = case[:9]
    mask_T = case[9] if len(case) > 9 else None
    rng = np.random.default_rng(hash_name(name))
    A = n_params(heads)
    E = -(-(2 * n + 3) // ov_T) if ov_T else 0
    N = E * ov_T if ov_T else 2 * n + 3  # a dataset about twice the minibatch
    params, old_params, actions = draw_dists(rng, heads, N, n)
    if read == "index":
        index, offset = rng.permutation(N)[:n].astype(np.int32), 0
        rows = index.astype(np.int64)
    else:
        index, offset = None, 3
        rows = np.arange(offset, offset + n)
    # ratio placement: row 0 raw ratio 60 (> 20), row 1 1/60 (< 0.05), rows 2 / 3 outside the clip range but inside
    # [0.05, 20], the others around 1
    shift = rng.standard_normal(n) * 0.05
    shift[:4] = [-math.log(60.0), math.log(60.0), -0.3, 0.3]
    mask = None
    if mask_T is not None:  # (its own generator: the draws below stay those of an unmasked case of the same name)
        mask = draw_mask(np.random.default_rng(hash_name(name + "/mask")), heads, N)
        first = next(i for i, h in enumerate(heads) if h > 0)  # minibatch row 2 (valid below): an all-masked member
        mask[rows[2], n_params(heads[:first]):n_params(heads[:first + 1])] = 0
        allowed_actions(mask, heads, actions)
    old_logp = np.zeros(N, np.float32)
    old_logp[rows] = (logp64(params, actions[rows], heads, None if mask is None else mask[rows]) + shift).astype(np.float32)
    valids = rng.random(N) > 0.15
    valids[rows[:6]] = True
    valids[rows[6]] = False
    old_values = rng.standard_normal(N).astype(np.float32)
    dv = rng.standard_normal(n) * 1.5 * CLIP_VALUE
    dv[4], dv[5] = 3 * CLIP_VALUE, -3 * CLIP_VALUE  # v - v_old outside clip_value, both sides
    values = (old_values[rows] + dv).astype(np.float32)
    nadv = n if dense_adv else N  # dense_adv: adv / targets are indexed by the minibatch row
    adv = (rng.standard_normal(nadv) * 2 + 0.3).astype(np.float32)
    targets = rng.standard_normal(nadv).astype(np.float32)
    if ov_T:  # the slab's [E, T + 1] array read in place: dataset row e * T + t -> e * (T + 1) + t
        ov = np.full((E, ov_T + 1), 1e30, np.float32)
        ov[:, :ov_T] = old_values.reshape(E, ov_T)
        old_values = ov.reshape(-1)
    kind = 1 if len(heads) == 1 and heads[0] < 0 else 0
    cfg = lib.sf_loss_cfg(clip_ratio=CLIP_RATIO, clip_value=CLIP_VALUE, value_loss_coeff=0.5,
                          exploration_coeff=0.01 if expl_kind else 0.0, kl_coeff=kl_coeff, exploration_kind=expl_kind,
                          action_kind=kind, dense_adv=dense_adv, old_values_T=ov_T)
    if entry == "cfg" and len(heads) > 1:
        cfg.num_heads = len(heads)
        for i, h in enumerate(heads):
            cfg.head_n[i] = int(h)
    m = torch.cat([dev(values)[:, None], dev(params)], 1).contiguous()
    g = torch.full_like(m, SENT)
    ratio = torch.full((n,), SENT, device="cuda")
    idx = dev(index) if index is not None else None
    d_valids, d_adv = dev(valids), dev(adv)
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    out = torch.zeros(16, device="cuda")
    lib.moments(d_adv, d_valids, idx, n, mom, offset=offset, dense_x=bool(dense_adv))
    args = (m[:, 1:], 1 + A, m[:, 0], 1 + A, dev(actions), dev(old_logp), dev(old_params), dev(old_values), d_adv,
            dev(targets), d_valids, idx, offset, n, A, cfg, mom, sums, g[:, 1:], g[:, 0], ratio)
    if entry == "masked":
        lib.ppo_loss(*args, head_sizes=heads, mask=slab_mask(mask, mask_T), mask_T=mask_T)
    elif entry == "cfg":
        lib.ppo_loss(*args)
    else:  # sf_ppo_loss_heads with the list as its argument, whatever its length
        p, r = lib.ptr, lib._raw
        hn = (C.c_int32 * len(heads))(*heads)
        rc = lib.load().sf_ppo_loss_heads(
            r(args[0], "f32", "params"), 1 + A, r(args[2], "f32", "values"), 1 + A, p(args[4], "f32"), p(args[5], "f32"),
            p(args[6], "f32"), p(args[7], "f32"), p(args[8], "f32"), p(args[9], "f32"), p(args[10], "u8"), p(idx, "i32"),
            lib.i64(offset), lib.i64(n), A, C.byref(cfg), p(mom, "f64"), p(sums, "f64"), r(args[18], "f32", "g_params"),
            r(args[19], "f32", "g_values"), p(ratio, "f32"), hn, len(heads), lib.stream())
        lib._check(rc, "sf_ppo_loss_heads")
    lib.loss_scalars(sums, mom, cfg, out)
    torch.cuda.synchronize()
    o = dict(sums=sums.cpu().numpy(), moments=mom.cpu().numpy(), grads=g.cpu().numpy(), ratio=ratio.cpu().numpy(),
             scalars=out.cpu().numpy())
    if mask is not None:  # valid minibatch rows with an all-masked Discrete member (what the case is there for)
        o["all_masked_rows"] = np.int32(sum(valids[r] and all_masked_member(mask[r], heads) for r in rows))
    return o


def hash_name(name):
    """a seed from the case's name that does not depend on the interpreter (hash() of a str is salted)"""
    import zlib
    return zlib.crc32(name.encode())


# ---------------------------------------------------------------------------------------------------- V-trace
# (name, heads, recurrence, trajectories, rho_hat, c_hat, read through)
VTRACE_CASES = [
    ("vtrace_d8", [8], 7, 10, 1.0, 1.0, "index"),
    ("vtrace_d32", [32], 5, 14, 2.0, 0.5, "offset"),
    ("vtrace_box16", [-16], 5, 14, 0.5, 2.0, "offset"),
    ("vtrace_3_b2_5", [3, -2, 5], 7, 10, 2.0, 0.5, "index"),
    ("vtrace_11", [3] * 9 + [-2, 4], 1, 70, 1.0, 1.0, "index"),
    ("vtrace_100_b3_7", [100, -3, 7, 5, 1, -1, 3], 7, 10, 1.0, 1.0, "offset"),
    ("vtrace_d129", [129], 7, 10, 0.5, 2.0, "index"),
    ("vtrace_box70_wide", [-70], 5, 14, 1.0, 1.0, "offset"),
    ("vtrace_5_130_b2_7", [5, 130, -2, 7], 7, 10, 2.0, 0.5, "index"),
]
# the same fields and mask_T: sf_vtrace_masked (k_masked_vtrace_ratio / _wide)
MASKED_VTRACE_CASES = [
    ("mvtrace_d9", [9], 7, 10, 1.0, 1.0, "index", 0),
    ("mvtrace_3_b2_5", [3, -2, 5], 5, 14, 2.0, 0.5, "offset", 5),
    ("mvtrace_130_4", [130, 4], 7, 10, 0.5, 2.0, "index", 7),
]


def run_vtrace_case(lib, case):
    import torch
    name, heads, rec, ntraj, rho_hat, c_hat, read = case[:7]
    mask_T = case[7] if len(case) > 7 else None
    rng = np.random.default_rng(hash_name(name))
    A, n = n_params(heads), rec * ntraj
    N = 2 * n
    params, _, actions = draw_dists(rng, heads, N, n)
    if read == "index":
        index, offset = rng.permutation(N)[:n].astype(np.int32), 0
        rows = index.astype(np.int64)
    else:
        index, offset = None, rec * 2
        rows = np.arange(offset, offset + n)
    shift = rng.standard_normal(n) * 0.5
    shift[0], shift[1] = -90.0, 4.0  # logp - old_logp = 90 (f32 exp overflows), ratio e^-4 < 0.05
    mask = None
    if mask_T is not None:
        mask = draw_mask(np.random.default_rng(hash_name(name + "/mask")), heads, N)
        allowed_actions(mask, heads, actions)
    old_logp = np.zeros(N, np.float32)
    old_logp[rows] = (logp64(params, actions[rows], heads, None if mask is None else mask[rows]) + shift).astype(np.float32)
    values = rng.standard_normal(n).astype(np.float32)
    rewards = rng.standard_normal(N).astype(np.float32)
    dones = rng.random(N) < 0.1
    kind = 1 if len(heads) == 1 and heads[0] < 0 else 0
    m = torch.cat([dev(values)[:, None], dev(params)], 1).contiguous()
    vs, adv = torch.full((n,), SENT, device="cuda"), torch.full((n,), SENT, device="cuda")
    lib.vtrace(m[:, 1:], 1 + A, m[:, 0], 1 + A, dev(actions), dev(old_logp), dev(rewards), dev(dones),
               dev(index) if index is not None else None, offset, n, A, kind, rec, 0.99, rho_hat, c_hat, vs, adv,
               head_sizes=heads, **({} if mask is None else dict(mask=slab_mask(mask, mask_T), mask_T=mask_T)))
    torch.cuda.synchronize()
    return dict(vs=vs.cpu().numpy(), adv=adv.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- consistency loss
# (name, heads, n, read through): k_consistency_loss up to 128 parameters (at most 256 rows), k_consistency_loss_wide
# beyond (7 rows)
CONSISTENCY_CASES = [
    (f"cons_{tag}_{read}", heads, n, read)
    for tag, heads, n in (("d7", [7], 70), ("box3", [-3], 70), ("3_b2_5", [3, -2, 5], 70), ("d129", [129], 7),
                          ("130_b2_3", [130, -2, 3], 7))
    for read in ("index", "offset")
]


def run_consistency_case(lib, case):
    """target rows and student rows are the two halves of one [2 n, 1 + A] heads matrix, as the learner holds them; some
    student rows equal their target's bits (KL and gradient exactly 0), some log_std sit beyond both clamp ends"""
    import torch
    name, heads, n, read = case
    rng = np.random.default_rng(hash_name(name))
    A, N = n_params(heads), 2 * n + 3
    params_s, _, _ = draw_dists(rng, heads, N, n)
    params_t = (params_s + rng.standard_normal((n, A)) * 0.3).astype(np.float32)
    params_t[2::5] = params_s[2::5]
    values = rng.standard_normal((2 * n, 1)).astype(np.float32)
    values[2] = values[n + 2]
    if read == "index":
        index, offset = rng.permutation(N)[:n].astype(np.int32), 0
        rows = index.astype(np.int64)
    else:
        index, offset = None, 3
        rows = np.arange(offset, offset + n)
    valids = rng.random(N) > 0.15
    valids[rows[:3]] = True
    valids[rows[3]] = False
    m = dev(np.concatenate([values, np.concatenate([params_t, params_s])], 1))
    g = torch.full_like(m, SENT)
    mom = dev(np.array([0.0, 0.0, valids[rows].sum()]))
    sums = torch.full((4,), SENT, dtype=torch.float64, device="cuda")
    kind = 1 if len(heads) == 1 and heads[0] < 0 else 0
    lib.consistency_loss(m[:n, 1:], m[n:, 1:], 1 + A, m[:n, 0], m[n:, 0], 1 + A, dev(valids),
                         dev(index) if index is not None else None, offset, n, A, kind, 0.7, 0.3, mom, sums, g[n:, 1:],
                         g[n:, 0], head_sizes=heads)
    torch.cuda.synchronize()
    return dict(sums=sums.cpu().numpy(), grads=g.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- samplers
B = 70
# (name, entry point, heads); every case runs sampling and deterministic
SAMPLER_CASES = [
    ("sample_d7", "single", [7]), ("sample_d32", "single", [32]), ("sample_d128", "single", [128]),
    ("sample_box3", "single", [-3]), ("sample_d129", "single", [129]), ("sample_box70_wide", "single", [-70]),
    ("masked_d9", "masked", [9]), ("masked_d129", "masked", [129]),
    ("tuple_3_b2_5", "tuple", [3, -2, 5]), ("tuple_11", "tuple", [3] * 9 + [-2, 4]), ("tuple_3_4_5", "tuple", [3, 4, 5]),
    ("tuple_129_3", "tuple", [129, 3]), ("tuple_5_130_b2_7", "tuple", [5, 130, -2, 7]),
    ("mtuple_3_4_5", "tuple_masked", [3, 4, 5]), ("mtuple_3_b2_5", "tuple_masked", [3, -2, 5]),
    ("mtuple_11", "tuple_masked", [3] * 9 + [-2, 4]),
    ("mtuple_129_3", "tuple_masked", [129, 3]), ("mtuple_5_130_b2_7", "tuple_masked", [5, 130, -2, 7]),
]


def draw_mask(rng, heads, nrows):
    """u8 [nrows, A]: rows cycle through an all-zero member, a member with a single allowed action, a random mask with
    one action allowed per member, and everything allowed"""
    A = n_params(heads)
    mask = np.ones((nrows, A), np.uint8)
    kind = np.arange(nrows) % 4
    off = 0
    for i, h in enumerate(heads):
        w = h if h > 0 else -2 * h
        if h > 0:
            hit = (np.arange(nrows) // 4 + i) % 2 == 0  # which members of the row get the row's treatment
            sl = mask[:, off:off + h]
            sl[(kind == 0) & hit] = 0
            one = (kind == 1) & hit
            sl[one] = 0
            sl[one, rng.integers(0, h, one.sum())] = 1
            rnd = kind == 2
            sl[rnd] = rng.random((rnd.sum(), h)) < 0.5
            sl[rnd, rng.integers(0, h, rnd.sum())] = 1
        off += w
    return mask


def run_sampler_case(lib, case, deterministic):
    import torch
    name, entry, heads = case
    rng = np.random.default_rng(hash_name(name))
    A, nact, T, t = n_params(heads), n_cols(heads), 2, 1
    seed, step, row0 = 1234 + A, 77, 100003 + 17 * A
    logits = (rng.standard_normal((B, A)) * 3.0).astype(np.float32)
    logits[::9] *= 12.0  # rows whose tail probabilities underflow in f32
    if deterministic:
        logits[1::5] = np.round(logits[1::5])  # ties: the first maximum
    off = 0
    for h in heads:
        if h < 0:
            logits[:, off - h:off - 2 * h] = rng.uniform(-12, 12, (B, -h))
        off += h if h > 0 else -2 * h
    values = rng.standard_normal(B).astype(np.float32)
    heads_m = dev(np.concatenate([values[:, None], logits, np.zeros((B, 3), np.float32)], 1))
    ld = heads_m.shape[1]
    s = lambda *sh: torch.full(sh, SENT, device="cuda")
    tr = dict(actions=s(B, T, nact), logits=s(B, T, A), logp=s(B, T), values=s(B, T + 1), ver=s(B, T))
    all_discrete = all(h > 0 for h in heads)
    env_a = torch.full((B, len(heads)), -5, dtype=torch.int32, device="cuda") if all_discrete else None
    slab = (tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], env_a)
    if entry in ("masked", "tuple_masked"):
        slab_mask = torch.zeros((B, T + 1, A), dtype=torch.uint8, device="cuda")
        slab_mask[:, t] = dev(draw_mask(rng, heads, B))
        mview = slab_mask[:, t]
    if entry == "single":
        lib.sample_write_step(heads_m[:, 1:], ld, heads_m[:, 0], ld, B, A, T, t, seed, step, row0, 42.0, deterministic,
                              *slab, action_kind=1 if heads[0] < 0 else 0)
    elif entry == "masked":
        lib.sample_write_step_masked(heads_m[:, 1:], ld, heads_m[:, 0], ld, mview, mview.stride(0), B, A, T, t, seed, step,
                                     row0, 42.0, deterministic, *slab)
    elif entry == "tuple":
        lib.sample_write_step_tuple(heads_m[:, 1:], ld, heads_m[:, 0], ld, B, heads, T, t, seed, step, row0, 42.0,
                                    deterministic, *slab)
    else:
        lib.sample_write_step_tuple_masked(heads_m[:, 1:], ld, heads_m[:, 0], ld, mview, mview.stride(0), B, heads, T, t,
                                           seed, step, row0, 42.0, deterministic, *slab)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in tr.items()}
    # the recorded logits are an exact copy of the input: checked here, not stored (they would be most of the fixture)
    rec = o.pop("logits")
    o["logits_ok"] = np.uint8(np.array_equal(rec[:, t], logits) and np.all(rec[:, 1 - t] == SENT))
    if env_a is not None:
        o["env_a"] = env_a.cpu().numpy()
    return o


def run_all(lib):
    """{"<case>/<array>": host array} of every case, in a fixed order"""
    rec = {}
    for case in LOSS_CASES:
        rec.update({f"{case[0]}/{k}": v for k, v in run_loss_case(lib, case).items()})
    for case in VTRACE_CASES:
        rec.update({f"{case[0]}/{k}": v for k, v in run_vtrace_case(lib, case).items()})
    for case in SAMPLER_CASES:
        for det in (False, True):
            rec.update({f"{case[0]}_{'det' if det else 'draw'}/{k}": v
                        for k, v in run_sampler_case(lib, case, det).items()})
    return rec


def run_all_second(lib):
    """the second fixture's {"<case>/<array>": host array}"""
    rec = {}
    for cases, run in ((MASKED_LOSS_CASES, run_loss_case), (MASKED_VTRACE_CASES, run_vtrace_case),
                       (CONSISTENCY_CASES, run_consistency_case)):
        for case in cases:
            rec.update({f"{case[0]}/{k}": v for k, v in run(lib, case).items()})
    return rec


def main():
    from sample_factory_amd import lib
    lib.load()
    argv = [a for a in sys.argv[1:] if a != "--second"]
    second = len(argv) < len(sys.argv) - 1
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", "rl_heads_parent2.npz" if second else "rl_heads_parent.npz")
    rec = run_all_second(lib) if second else run_all(lib)
    rec["parent"] = np.array(PARENT2 if second else PARENT)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: {len(rec) - 1} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
