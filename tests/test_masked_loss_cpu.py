"""Training under the action mask, the parts that need no GPU: the float64 yardstick that judges the
masked loss and V-trace kernels (masked_dist_terms, masked_ref_loss) held to the action-distribution objects, the two
additive entry points (exported, declared, refusing bad arguments on the host), and the engine flag."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from sample_factory_amd.envs import spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS, VTRACE = "sf_ppo_loss_masked", "sf_vtrace_masked"
LN2PI_2 = 0.5 * math.log(2.0 * math.pi)


def n_params(heads):
    return sum(h if h > 0 else -2 * h for h in heads)


def _space(heads):
    sp = [spaces.Discrete(h) if h > 0 else spaces.Box(-1.0, 1.0, (-h,), np.float32) for h in heads]
    return sp[0] if len(sp) == 1 else spaces.Tuple(sp)


def _masked_member(z, m):
    """log-probs and probabilities of one Discrete member under its mask slice (bool), float64 torch.  A slice that
    allows something: log_softmax of z - 1e9 on the masked-out columns, p = softmax * mask / (sum + 1e-13).  An all-zero
    slice follows the f32 rule: z - 1e9 absorbs |z| < 32, so the member behaves as n equal logits (log-prob -log n with
    d/dz_k = delta_ak - 1 / n) and p = 0."""
    none = ~m.any(1, keepdim=True)
    y = torch.where(none, z - z.detach(), z + (~m).to(z.dtype) * -1e9)
    l = torch.log_softmax(y, 1)
    s = l.exp() * m
    return l, s / (s.sum(1, keepdim=True) + 1e-13)


def masked_dist_terms(params, old_params, actions, heads, mask):
    """float64 torch: per-sample log-prob of `actions`, entropy and KL(new || old) under `mask` ([n, A], non-zero =
    allowed, column c belonging to parameter column c).  Per Discrete member: log-prob logp_a, entropy -sum p logp,
    KL sum p (logp - logp_old) with the old distribution under the same mask slice; a Box(D) member never reads its 2 D
    mask columns and its terms are the unmasked ones; row quantities are sums over the members."""
    z, zo, act = params, old_params, actions
    m_all = torch.as_tensor(np.asarray(mask) != 0)
    lp = ent = kl = 0.0
    off = col = 0
    for h in heads:
        if h > 0:
            m = m_all[:, off:off + h]
            l, p = _masked_member(z[:, off:off + h], m)
            lo, _ = _masked_member(zo[:, off:off + h], m)
            lp = lp + l.gather(1, act[:, col].long()[:, None])[:, 0]
            ent = ent - (p * l).sum(1)
            kl = kl + (p * (l - lo)).sum(1)
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
    return lp, ent, kl


def masked_ref_loss(params, values, actions, old_logp, old_params, old_values, adv, targets, valids, heads, c, mask):
    """float64 autograd of the learner's total loss under the mask (rows already gathered): ref_loss of
    tests/test_gpu_action_heads.py with masked_dist_terms for the distribution terms (exploration: none or entropy).
    mask=None: the unmasked dist_terms, the yardstick of the all-ones test."""
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    z = t(params).requires_grad_(True)
    v = t(values).requires_grad_(True)
    m = torch.tensor(np.asarray(valids, bool))
    act = t(actions).reshape(len(values), -1)
    if mask is None:
        from test_gpu_action_heads import dist_terms
        lp, ent, kl, _ = dist_terms(z, t(old_params), act, heads)
    else:
        lp, ent, kl = masked_dist_terms(z, t(old_params), act, heads, mask)
    ratio = torch.clamp(torch.exp(lp - t(old_logp)), 0.05, 20.0)
    a = t(adv)
    mean, n = a[m].mean(), int(m.sum())
    std = a[m].std()
    advn = (a - mean) / torch.clamp_min(std, 1e-7)
    hi = 1.0 + c["clip_ratio"]
    lo = 1.0 / hi
    policy = -torch.min(ratio * advn, torch.clamp(ratio, lo, hi) * advn)[m].mean()
    assert c["expl_kind"] in (0, 1)
    expl = -c["expl_coeff"] * ent[m].mean() if c["expl_kind"] == 1 else torch.zeros((), dtype=torch.float64)
    kl_loss = c["kl_coeff"] * kl[m].mean()
    vo, R = t(old_values), t(targets)
    vclip = vo + torch.clamp(v - vo, -c["clip_value"], c["clip_value"])
    value = c["value_coeff"] * torch.max((v - R) ** 2, (vclip - R) ** 2)[m].mean()
    (policy + expl + kl_loss + value).backward()
    out = dict(policy_loss=policy.item(), exploration_loss=expl.item(), kl_loss=kl_loss.item(), value_loss=value.item(),
               kl_mean=kl[m].mean().item(), kl_max=kl[m].max().item(), adv_mean=mean.item(), adv_std=std.item(),
               n_valid=float(n))
    with torch.no_grad():  # distance of every sample to the nearest kink of the loss, as ref_loss measures it
        raw = torch.exp(lp - t(old_logp))
        d = torch.stack([(raw - 0.05).abs() / 0.05, (raw - 20).abs() / 20, (ratio - lo).abs(), (ratio - hi).abs(),
                         ((v - vo).abs() - c["clip_value"]).abs(),
                         torch.where(vclip != v, ((v - R) ** 2 - (vclip - R) ** 2).abs() / (1e-3 + (v - R) ** 2), 1.0)],
                        1).min(1).values
        off = 0
        for h in heads:
            if h < 0:
                e = torch.exp(z[:, off - h:off - 2 * h])
                d = torch.minimum(d, torch.minimum((e / 1e-4).log().abs(), (e / 1e4).log().abs()).min(1).values)
            off += h if h > 0 else -2 * h
    out["grad_params"], out["grad_values"] = z.grad.numpy(), v.grad.numpy()
    out["kink"] = d.numpy() < 1e-4
    out["logp"], out["kl"] = lp.detach().numpy(), kl.detach().numpy()
    return out


def make_mask(rng, heads, actions, p_allow=0.5):
    """[N, A] u8: every column allowed with probability p_allow, the taken action always, at least one column per
    Discrete member; the columns under a Box member are random too (nobody may read them)"""
    N, A = len(actions), n_params(heads)
    mask = (rng.random((N, A)) < p_allow).astype(np.uint8)
    off = col = 0
    for h in heads:
        if h > 0:
            mask[np.arange(N), off + actions[:, col].astype(np.int64)] = 1
            off, col = off + h, col + 1
        else:
            off, col = off - 2 * h, col - h
    return mask


# the cases of tests/test_gpu_masked_loss.py::test_masked_loss_vs_float64_autograd: (heads, exploration kind, kl_coeff,
# slab layout); built here so that the kink fraction of every case is confirmed without a GPU
MASKED_LOSS_CASES = [
    ([2], 1, 0.0, True), ([6], 0, 0.2, False), ([33], 1, 0.2, True), ([128], 0, 0.0, False),
    ([4, 3], 1, 0.2, True), ([5] * 8, 0, 0.2, False), ([3] * 12, 1, 0.0, True),
    ([3, -2, 5], 1, 0.2, False), ([100, -3, 7, 5, 1, -1, 3], 0, 0.2, True),
    ([300], 1, 0.2, False), ([21] * 8, 1, 0.0, True), ([150, 5], 0, 0.2, False),
]
MASK_T = 8
N_ROWS = 1024


def build_masked_case(heads, expl_kind, kl_coeff):
    """the data of one case, generated as test_ppo_loss_vs_float64_autograd generates it (make_loss_data /
    finish_loss_data) plus the mask; old log-probs are placed around the MASKED float64 log-prob, so that the ratios
    visit the same regions.  Returns (c, ds, index, values, gathered rows, mask [N, A], gathered mask)"""
    from test_gpu_action_heads import _cfg, finish_loss_data, make_loss_data
    c = _cfg(expl_kind, kl_coeff)
    rng = np.random.default_rng(abs(sum(heads)) * 31 + expl_kind)
    N, n = 3 * N_ROWS, N_ROWS
    ds = make_loss_data(rng, heads, N, n)
    index = rng.permutation(N)[:n].astype(np.int32)
    values, _ = finish_loss_data(rng, ds, heads, index, c)   # (moves actions under a clamped Box sd; old_logp redone below)
    mask = make_mask(rng, heads, ds["actions"])
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    lp, _, _ = masked_dist_terms(t(ds["params"]), t(ds["old_params"][index]), t(ds["actions"][index]), heads, mask[index])
    shift = rng.standard_normal(n) * 0.15
    k = rng.random(n)
    shift[k < 0.05] = -math.log(60.0)
    shift[(k >= 0.05) & (k < 0.1)] = math.log(60.0)
    ds["old_logp"][index] = (lp.numpy() + shift).astype(np.float32)
    g = {k2: ds[k2][index] for k2 in ("actions", "old_logp", "old_params", "old_values", "adv", "targets", "valids")}
    return c, ds, index, values, g, mask, mask[index]


_REFS = {}


def masked_case_ref(heads, expl_kind, kl_coeff):
    """(case data, float64 reference), computed once per case and shared by the tests that need it"""
    key = (tuple(heads), expl_kind, kl_coeff)
    if key not in _REFS:
        case = build_masked_case(heads, expl_kind, kl_coeff)
        c, ds, index, values, g, mask, gm = case
        _REFS[key] = (case, masked_ref_loss(ds["params"], values, g["actions"], g["old_logp"], g["old_params"],
                                            g["old_values"], g["adv"], g["targets"], g["valids"], heads, c, gm))
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("heads", [[6], [4, 3], [5] * 8, [3, -2, 5]], ids=str)
def test_yardstick_equals_the_distribution_objects(heads):
    """masked_dist_terms against get_action_distribution(space, z, mask) in float64, values and autograd gradients, on
    rows whose every Discrete slice allows something (1e-12: two float64 evaluations of the same formulas)"""
    from sample_factory_amd.algo.utils.action_distributions import get_action_distribution
    n, A = 96, n_params(heads)
    rng = np.random.default_rng(A)
    z = torch.tensor(rng.standard_normal((n, A)) * 2, requires_grad=True)
    zo = torch.tensor(rng.standard_normal((n, A)))
    off = 0
    for h in heads:  # keep a Box member's log_std inside the clamp
        if h < 0:
            with torch.no_grad():
                z[:, off - h:off - 2 * h].clamp_(-1.5, 1.0)
                zo[:, off - h:off - 2 * h].clamp_(-1.5, 1.0)
        off += h if h > 0 else -2 * h
    nact = sum(1 if h > 0 else -h for h in heads)
    act = np.zeros((n, nact))
    col = 0
    for h in heads:
        if h > 0:
            act[:, col] = rng.integers(0, h, n)
            col += 1
        else:
            act[:, col:col - h] = rng.standard_normal((n, -h))
            col += -h
    mask = make_mask(rng, heads, act)
    a = torch.tensor(act)
    lp, ent, kl = masked_dist_terms(z, zo, a, heads, mask)
    w = torch.tensor(rng.standard_normal((3, n)))
    g_mine, = torch.autograd.grad((w[0] * lp + w[1] * ent + w[2] * kl).sum(), z)
    space, mk = _space(heads), torch.tensor(mask).double()
    z2 = z.detach().clone().requires_grad_(True)
    dist, old = get_action_distribution(space, z2, mk), get_action_distribution(space, zo, mk)
    lp2, ent2, kl2 = dist.log_prob(a), dist.entropy(), dist.kl_divergence(old)
    g_obj, = torch.autograd.grad((w[0] * lp2 + w[1] * ent2 + w[2] * kl2).sum(), z2)
    for got, want in ((lp, lp2), (ent, ent2), (kl, kl2), (g_mine, g_obj)):
        np.testing.assert_allclose(got.detach().numpy(), want.detach().numpy(), rtol=1e-12, atol=1e-12)
    # the gradient of the log-prob is exactly zero on a masked-out column of a Discrete member
    g_lp, = torch.autograd.grad(masked_dist_terms(z, zo, a, heads, mask)[0].sum(), z)
    off = 0
    for h in heads:
        if h > 0:
            assert np.all(g_lp[:, off:off + h].numpy()[mask[:, off:off + h] == 0] == 0.0)
        off += h if h > 0 else -2 * h


def test_yardstick_all_zero_slice_is_n_equal_logits():
    """an all-zero slice: log-prob -log n whatever the logits, entropy 0, KL 0, d logp / dz_k = delta_ak - 1 / n and no
    entropy / KL gradient; the other member of the row is untouched by it"""
    heads, n = [5, 3], 16
    rng = np.random.default_rng(3)
    z = torch.tensor(rng.uniform(-30, 30, (n, 8)), requires_grad=True)
    zo = torch.tensor(rng.uniform(-30, 30, (n, 8)))
    act = np.stack([rng.integers(0, 5, n), rng.integers(0, 3, n)], 1).astype(np.float64)
    mask = make_mask(rng, heads, act)
    mask[:, :5] = 0
    lp, ent, kl = masked_dist_terms(z, zo, torch.tensor(act), heads, mask)
    lp1, ent1, kl1 = masked_dist_terms(z[:, 5:], zo[:, 5:], torch.tensor(act[:, 1:]), [3], mask[:, 5:])
    np.testing.assert_allclose((lp - lp1).detach().numpy(), -math.log(5.0), rtol=1e-14)
    np.testing.assert_array_equal((ent - ent1).detach().numpy(), 0.0)
    np.testing.assert_array_equal((kl - kl1).detach().numpy(), 0.0)
    g, = torch.autograd.grad(lp.sum(), z, retain_graph=True)
    want = -np.full((n, 5), 0.2)
    want[np.arange(n), act[:, 0].astype(int)] += 1.0
    np.testing.assert_allclose(g[:, :5].numpy(), want, rtol=1e-14)
    g2, = torch.autograd.grad((ent + kl).sum(), z)
    assert np.all(g2[:, :5].numpy() == 0.0)


@pytest.mark.parametrize("heads,expl_kind,kl_coeff,slab", MASKED_LOSS_CASES, ids=str)
def test_gpu_cases_keep_their_samples_off_the_kinks(heads, expl_kind, kl_coeff, slab):
    """check_loss asks that more than 0.98 of the samples lie off a kink of the loss: confirmed here, from the float64
    yardstick alone, for every case the GPU test runs (and that the mask is what the issue describes)"""
    (c, ds, index, values, g, mask, gm), ref = masked_case_ref(heads, expl_kind, kl_coeff)
    assert (~ref["kink"]).mean() > 0.98, (heads, (~ref["kink"]).mean())
    assert np.isfinite(ref["grad_params"]).all() and all(np.isfinite(ref[k]) for k in ("policy_loss", "kl_mean"))
    off = col = 0
    for h in heads:
        if h > 0:
            sl = gm[:, off:off + h]
            assert sl.any(1).all() and sl[np.arange(len(gm)), g["actions"][:, col].astype(int)].all()
            if h > 2:
                assert 0.4 < sl.mean() < 0.8
            off, col = off + h, col + 1
        else:
            off, col = off - 2 * h, col - h


# ------------------------------------------------------------------------------------------------ the entry points
def test_library_exports_the_masked_entry_points_and_keeps_the_abi():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    for e in (LOSS, VTRACE):
        assert e in lib.SYMBOLS and re.search(r"\bint\s+" + e + r"\s*\(", text) and hasattr(L, e)
    assert L.sf_abi_version() == 19
    import inspect
    for fn in (lib.ppo_loss, lib.vtrace):
        sig = inspect.signature(fn).parameters
        assert sig["mask"].default is None and sig["mask_T"].default == 0


def _loss_cfg(lib, action_kind=0, expl_kind=1, expl_coeff=0.01):
    return lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.5, value_loss_coeff=0.5, exploration_coeff=expl_coeff,
                           kl_coeff=0.0, exploration_kind=expl_kind, action_kind=action_kind, dense_adv=0)


def test_masked_loss_refuses_bad_arguments_on_the_host():
    """made-up non-null addresses: every refusal comes before the memset and the launch, so this returns -1 on a machine
    with no GPU, and every message names the entry point"""
    from sample_factory_amd import lib
    L = lib.load()
    p = C.c_void_p(4096)
    arr = lambda hs: (C.c_int32 * len(hs))(*hs)
    err = lambda: L.sf_last_error().decode()

    def loss(hs, A, cfg=None, mask=p, ld_mask=None, mask_T=0, n_heads=None):
        cfg = cfg if cfg is not None else _loss_cfg(lib)
        return getattr(L, LOSS)(p, 1 << 20, p, 1, p, p, p, p, p, p, p, None, C.c_int64(0), C.c_int64(64), A, C.byref(cfg),
                                p, p, p, p, None, arr(hs), len(hs) if n_heads is None else n_heads, mask,
                                C.c_int64(A if ld_mask is None else ld_mask), mask_T, None)

    assert loss([4, 3], 7, mask=None) == -1 and LOSS in err() and "null mask" in err()
    assert loss([4, 3], 7, ld_mask=6) == -1 and LOSS in err() and "ld_mask=6" in err() and "A=7" in err()
    assert loss([4, 3], 7, mask_T=-1) == -1 and LOSS in err() and "mask_T=-1" in err()
    assert loss([-2], 4, cfg=_loss_cfg(lib, action_kind=1)) == -1 and LOSS in err() and "pure Box" in err()
    assert loss([-2, -1], 6) == -1 and LOSS in err() and "pure Box" in err()
    assert loss([2] * 65, 130) == -1 and LOSS in err() and "limit is 64" in err()
    assert loss([4, 3], 7, n_heads=0) == -1 and LOSS in err() and "limit is 64" in err()
    assert loss([3] * 8 + [0], 24) == -1 and LOSS in err() and "empty action head" in err()
    assert loss([4, 3], 8) == -1 and LOSS in err() and "sum to 7" in err()
    assert loss([5], 6) == -1 and LOSS in err() and "one-member list" in err()
    for hs, A in (([6], 6), ([4, 3], 7), ([300], 300)):
        assert loss(hs, A, cfg=_loss_cfg(lib, expl_kind=2)) == -1 and LOSS in err() and "symmetric_kl" in err()
    assert loss([4, -2, 3], 11, cfg=_loss_cfg(lib, expl_kind=2)) == -1 and LOSS in err()


def test_masked_vtrace_refuses_bad_arguments_on_the_host():
    from sample_factory_amd import lib
    L = lib.load()
    p, f = C.c_void_p(4096), C.c_float
    arr = lambda hs: (C.c_int32 * len(hs))(*hs)
    err = lambda: L.sf_last_error().decode()

    def vt(hs, A, kind=0, mask=p, ld_mask=None, mask_T=0, n=64, rec=8):
        return getattr(L, VTRACE)(p, 1 << 20, p, 1, p, p, p, p, None, C.c_int64(0), C.c_int64(n), A, kind, rec, f(0.99),
                                  f(1.0), f(1.0), p, p, arr(hs) if len(hs) > 1 else None, len(hs) if len(hs) > 1 else 0,
                                  mask, C.c_int64(A if ld_mask is None else ld_mask), mask_T, None)

    assert vt([6], 6, mask=None) == -1 and VTRACE in err() and "null mask" in err()
    assert vt([4, 3], 7, ld_mask=5) == -1 and VTRACE in err() and "ld_mask=5" in err() and "A=7" in err()
    assert vt([6], 6, mask_T=-3) == -1 and VTRACE in err() and "mask_T=-3" in err()
    assert vt([-2], 4, kind=1) == -1 and VTRACE in err() and "pure Box" in err()
    assert vt([-2, -1], 6) == -1 and VTRACE in err() and "pure Box" in err()
    assert vt([2] * 65, 130) == -1 and VTRACE in err() and "limit is 64" in err()
    assert vt([3, 0, 2], 5) == -1 and VTRACE in err() and "empty action head" in err()
    assert vt([4, 3], 8) == -1 and VTRACE in err() and "sum to 7" in err()
    assert vt([6], 6, n=63) == -1 and VTRACE in err() and "multiple of recurrence" in err()


def test_bindings_refuse_a_mask_of_the_wrong_kind():
    from sample_factory_amd import lib
    t = torch.zeros(4, 7)
    with pytest.raises(lib.SfHipError, match="action mask: expected dtype u8"):
        lib.ppo_loss(t, 7, t, 1, t, t, t, t, t, t, t, None, 0, 4, 7, _loss_cfg(lib), t, t, t, t, head_sizes=[4, 3],
                     mask=torch.zeros(4, 7))
    with pytest.raises(lib.SfHipError, match="action mask lives on cpu"):
        lib.vtrace(t, 7, t, 1, t, t, t, t, None, 0, 4, 7, 0, 1, 0.99, 1.0, 1.0, t, t, head_sizes=[4, 3],
                   mask=torch.zeros(4, 7, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_defaults_to_off_and_parses():
    from sample_factory_amd.cfg.arguments import ENGINE_FLAGS, default_cfg, parse_full_cfg, parse_sf_args
    assert ("mask_actions_in_loss", False) in [(f[0], f[2]) for f in ENGINE_FLAGS]
    assert default_cfg(env="x").mask_actions_in_loss is False
    assert default_cfg(env="x", mask_actions_in_loss=True).mask_actions_in_loss is True
    parser, _ = parse_sf_args(["--env=x", "--mask_actions_in_loss=True"])
    assert parse_full_cfg(parser, ["--env=x", "--mask_actions_in_loss=True"]).mask_actions_in_loss is True
    assert parse_full_cfg(parser, ["--env=x"]).mask_actions_in_loss is False


def _learner(with_mask, **kw):
    from sample_factory_amd.algo.learning.learner import Learner
    from sample_factory_amd.cfg.arguments import default_cfg
    obs = {"obs": spaces.Box(-1.0, 1.0, (3,), np.float32)}
    if with_mask:
        obs["action_mask"] = spaces.Box(0, 1, (6,), np.uint8)
    info = types.SimpleNamespace(obs_space=spaces.Dict(obs), action_space=spaces.Discrete(6))
    cfg = default_cfg(env="x", optimizer="not_an_optimizer", **kw)  # init() stops at the optimizer check or before it
    return Learner(cfg, info, torch.zeros(1), 0, None)


def test_learner_init_refuses_symmetric_kl_under_a_mask_only():
    """Learner.init with stubbed env info: the symmetric-KL refusal names the flag and is reached only when the flag is
    on AND the env has a mask (the stub's unknown optimizer is the error that follows it, before any GPU work)"""
    with pytest.raises(ValueError, match="mask_actions_in_loss.*symmetric_kl"):
        _learner(True, mask_actions_in_loss=True, exploration_loss="symmetric_kl").init()
    for with_mask, kw in ((False, dict(mask_actions_in_loss=True, exploration_loss="symmetric_kl")),
                          (True, dict(mask_actions_in_loss=False, exploration_loss="symmetric_kl")),
                          (True, dict(mask_actions_in_loss=True, exploration_loss="entropy"))):
        with pytest.raises(RuntimeError, match="Unknown optimizer"):
            _learner(with_mask, **kw).init()
    from sample_factory_amd.algo.learning.learner import Learner
    from sample_factory_amd.cfg.arguments import default_cfg
    on = default_cfg(env="x", mask_actions_in_loss=True)
    assert Learner._mask_in_loss(on, _learner(True).env_info) is True
    assert Learner._mask_in_loss(on, _learner(False).env_info) is False      # logged, the plain path
    assert Learner._mask_in_loss(default_cfg(env="x"), _learner(True).env_info) is False


# ------------------------------------------------------------------------------------------------ the recorded ISA
def _isa(path):
    """{kernel: (vgpr, agpr, lds, scratch)} of a recorded tools/isa_stats.py output"""
    lines = open(os.path.join(ROOT, "profiles", path)).read().splitlines()
    out = {}
    for name, stats in zip(lines[0::2], lines[1::2]):
        m = re.search(r"vgpr (\d+) agpr (\d+) sgpr \? lds (\d+) scratch (\d+)", stats)
        out[name.strip()] = tuple(int(x) for x in m.groups())
    return out


def test_recorded_isa_keeps_every_earlier_kernel_and_the_new_ones_have_no_scratch():
    """profiles/masked_loss_isa_{parent,new}.txt (tools/isa_stats.py on sf_rl.hip at the parent commit and at this build):
    every kernel of the parent shows the same VGPR / AGPR / LDS / scratch numbers, and the kernels that were added are
    the five masked ones, without scratch"""
    parent, new = _isa("masked_loss_isa_parent.txt"), _isa("masked_loss_isa_new.txt")
    assert len(parent) > 50 and all(new.get(k) == v for k, v in parent.items()), \
        [(k, v, new.get(k)) for k, v in parent.items() if new.get(k) != v]
    added = sorted(set(new) - set(parent))
    assert len(added) == 5 and all("k_masked_" in k for k in added), added
    assert all(new[k][3] == 0 for k in added), {k: new[k] for k in added}
