"""The consistency loss of DrAC (--augment_consistency_coeff, sf_consistency_loss) as far as it can be
checked without a GPU: the entry point's place in the C ABI, its argument refusals (all of them come before any launch or
memset), the engine flag and its refusals, and the float64 yardstick (tests/consistency_refs.py) against
torch.distributions.kl_divergence."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from tests import consistency_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sf_consistency_loss"
FLAG = "augment_consistency_coeff"


def test_entry_point_is_declared_listed_exported_and_callable_and_the_abi_stays():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert ENTRY in lib.SYMBOLS and re.search(r"\bint\s+" + ENTRY + r"\s*\(", text) and hasattr(L, ENTRY)
    assert callable(lib.consistency_loss)
    assert len(lib.SYMBOLS) == len(set(lib.SYMBOLS))
    assert L.sf_abi_version() == 19
    assert C.sizeof(lib.sf_loss_cfg) == (8 + 1 + 8 + 1) * 4   # the loss struct did not grow: the coefficients are arguments


def _p(a):
    return None if a is None else C.c_void_p(a)


def _heads(h):
    return None if h is None else (C.c_int32 * len(h))(*h)


def _call(L, pt=1 << 20, ps=1 << 21, ldp=8, vt=1 << 22, vs=1 << 23, ldv=8, valids=1 << 24, index=None, offset=0, n=16, A=6,
          kind=0, heads=None, nh=None, cp=0.1, cv=0.1, mom=1 << 25, sums=1 << 26, gp=1 << 27, gv=1 << 28):
    nh = (len(heads) if heads is not None else 0) if nh is None else nh
    return getattr(L, ENTRY)(_p(pt), _p(ps), ldp, _p(vt), _p(vs), ldv, _p(valids), _p(index), C.c_int64(offset), C.c_int64(n),
                             A, kind, _heads(heads), nh, C.c_float(cp), C.c_float(cv), _p(mom), _p(sums), _p(gp), _p(gv),
                             None)


REFUSED = [dict(pt=None), dict(ps=None), dict(vt=None), dict(vs=None), dict(valids=None), dict(mom=None), dict(sums=None),
           dict(gp=None), dict(gv=None),
           dict(n=-1), dict(A=0), dict(A=-3), dict(ldp=5), dict(ldv=0), dict(offset=-1),
           dict(kind=2), dict(kind=-1), dict(kind=1, A=5, ldp=8),                     # Box needs [means | log_std]
           dict(heads=[3, 2]),                                                         # sums to 5, A = 6
           dict(heads=[3, 0, 3]),                                                      # an empty member
           dict(heads=[1] * 65, A=65, ldp=68),                                         # more than SF_MAX_ACTION_HEADS
           dict(heads=[3, 3], nh=0), dict(heads=[3, 3], nh=-1),                        # a list of no members
           dict(heads=None, nh=2),                                                     # a length without a list
           dict(heads=[5]), dict(heads=[-3], kind=0), dict(heads=[6], kind=1),        # a one-member list is the single space
           dict(heads=[2, -2], kind=1),                                                # a head list needs action_kind 0
           dict(cp=-0.1), dict(cv=-1.0), dict(cp=float("nan")), dict(cv=float("inf")), dict(cp=float("-inf"))]


@pytest.mark.parametrize("kw", REFUSED, ids=[",".join(f"{k}={v if not isinstance(v, list) or len(v) < 9 else len(v)}"
                                                      for k, v in kw.items()) for kw in REFUSED])
def test_refusals_come_before_any_launch_and_name_the_entry_point(kw):
    """made-up non-null addresses: each call must return -1 on a machine with no GPU"""
    from sample_factory_amd import lib
    L = lib.load()
    assert _call(L, **kw) == -1, kw
    assert ENTRY in L.sf_last_error().decode(), (kw, L.sf_last_error().decode())


def test_n_zero_is_ok_and_launches_nothing():
    from sample_factory_amd import lib
    L = lib.load()
    assert _call(L, n=0) == 0
    assert _call(L, n=0, index=1 << 16, heads=[3, -1, 1]) == 0            # Discrete(3) + Box(1) + Discrete(1): 6 parameters
    assert _call(L, n=0, kind=1, heads=[-3]) == 0 and _call(L, n=0, heads=[6]) == 0
    assert _call(L, n=0, A=200, ldp=204, cp=0.0, cv=0.0) == 0             # the wide path; zero coefficients are served


# ------------------------------------------------------------------------------------------------ the flag
def _cfg_ok(**kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    return default_cfg(env="x", num_workers=1, num_envs_per_worker=2, rollout=4, batch_size=8, num_batches_per_epoch=1,
                       use_rnn=False, recurrence=1, **kw)


def test_flag_defaults_to_off_parses_and_round_trips_through_config_json(tmp_path):
    from sample_factory_amd.cfg.arguments import (ENGINE_FLAGS, FLAGS, cfg_dict, default_cfg, load_from_checkpoint,
                                                   parse_full_cfg, parse_sf_args)
    specs = {f[0]: f for f in ENGINE_FLAGS}
    assert specs[FLAG][1:] == (float, 0.0)
    assert FLAG not in {f[0] for f in FLAGS}    # it shadows no reference flag
    assert default_cfg(env="x").augment_consistency_coeff == 0.0
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=drac", "--augment_random_shift=4", f"--{FLAG}=0.1"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    assert cfg.augment_consistency_coeff == 0.1 and cfg.cli_args[FLAG] == 0.1
    off = parse_full_cfg(parser, ["--env=x"])
    assert off.augment_consistency_coeff == 0.0 and FLAG not in off.cli_args
    os.makedirs(tmp_path / "drac")
    with open(tmp_path / "drac" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    assert json.load(open(tmp_path / "drac" / "config.json"))[FLAG] == 0.1
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=drac"]  # enjoy: the flag is not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    loaded = load_from_checkpoint(parse_full_cfg(parser, argv))
    assert loaded.augment_consistency_coeff == 0.1 and loaded.augment_random_shift == 4
    argv += [f"--{FLAG}=0.5"]  # ... and the command line still overrides the file
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).augment_consistency_coeff == 0.5


def test_verify_cfg_refusals():
    from sample_factory_amd.cfg.arguments import augment_consistency_coeff, verify_cfg
    info = type("I", (), dict(num_agents=1))()
    assert verify_cfg(_cfg_ok(), info)
    assert verify_cfg(_cfg_ok(augment_random_shift=4), info)                                   # RAD alone
    assert verify_cfg(_cfg_ok(augment_random_shift=4, augment_consistency_coeff=0.1), info)    # DrAC
    assert verify_cfg(_cfg_ok(mask_actions_in_loss=True), info)                                # alpha = 0: nothing changes
    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        assert not verify_cfg(_cfg_ok(augment_random_shift=4, augment_consistency_coeff=bad), info), bad
        with pytest.raises(ValueError, match=FLAG):
            augment_consistency_coeff(_cfg_ok(augment_random_shift=4, augment_consistency_coeff=bad))
    assert not verify_cfg(_cfg_ok(augment_consistency_coeff=0.1), info)                        # no shift to be consistent with
    with pytest.raises(ValueError) as e:
        augment_consistency_coeff(_cfg_ok(augment_consistency_coeff=0.1))
    assert FLAG in str(e.value) and "augment_random_shift" in str(e.value)                     # the message names both flags
    with pytest.raises(NotImplementedError, match="mask_actions_in_loss"):
        verify_cfg(_cfg_ok(augment_random_shift=4, augment_consistency_coeff=0.1, mask_actions_in_loss=True), info)
    assert augment_consistency_coeff(_cfg_ok()) == 0.0
    assert augment_consistency_coeff(_cfg_ok(augment_random_shift=4, augment_consistency_coeff=0.25)) == 0.25


def test_learner_init_refuses_before_it_touches_the_device():
    """Learner.init checks the flag right after the exploration loss: no GPU is needed to be refused"""
    from sample_factory_amd.algo.learning.learner import Learner
    for kw, exc in [(dict(augment_consistency_coeff=-1.0, augment_random_shift=4), ValueError),
                    (dict(augment_consistency_coeff=float("nan"), augment_random_shift=4), ValueError),
                    (dict(augment_consistency_coeff=0.1), ValueError),
                    (dict(augment_consistency_coeff=0.1, augment_random_shift=4, mask_actions_in_loss=True),
                     NotImplementedError)]:
        learner = Learner.__new__(Learner)
        learner.cfg = _cfg_ok(**kw)
        learner.env_info = type("I", (), dict(obs_space=None))()
        with pytest.raises(exc, match=FLAG):
            learner.init()


# ------------------------------------------------------------------------------------------------ the yardstick
def _rows(head_sizes, rows, seed):
    g = torch.Generator().manual_seed(seed)
    A = R.num_params(head_sizes)
    out = []
    for _ in range(2):
        h = torch.randn(rows, 1 + A, generator=g, dtype=torch.float64) * 2.0
        for kind, off, size in R.member_slices(head_sizes):
            if kind == "box":
                h[:, 1 + off + size:1 + off + 2 * size] = torch.rand(rows, size, generator=g, dtype=torch.float64) * 4.0 - 2.0
        out.append(h)
    return out


@pytest.mark.parametrize("head_sizes", [[5], [-3], [3, -2, 5], [130, 3]])
def test_yardstick_equals_torch_distributions(head_sizes):
    from torch.distributions import Categorical, Independent, Normal, kl_divergence
    ht, hs = _rows(head_sizes, 7, 11 + len(head_sizes))
    kl = R.row_kl(ht[:, 1:], hs[:, 1:], head_sizes)
    want = torch.zeros(7, dtype=torch.float64)
    for kind, off, size in R.member_slices(head_sizes):
        t, s = ht[:, 1 + off:], hs[:, 1 + off:]
        if kind == "cat":
            want += kl_divergence(Categorical(logits=t[:, :size]), Categorical(logits=s[:, :size]))
        else:
            want += kl_divergence(Independent(Normal(t[:, :size], t[:, size:2 * size].exp()), 1),
                                  Independent(Normal(s[:, :size], s[:, size:2 * size].exp()), 1))
    assert torch.allclose(kl, want, rtol=1e-12, atol=1e-13), (kl - want).abs().max()
    assert (kl > 0).all()


def test_yardstick_means_over_valid_rows_detaches_the_target_and_has_the_stated_gradients():
    head_sizes = [4, -2]
    ht, hs = _rows(head_sizes, 9, 5)
    valid = torch.tensor([1, 1, 0, 1, 1, 1, 0, 1, 1], dtype=torch.bool)
    ref = R.consistency_reference(ht, hs, valid, head_sizes, 0.3, 0.7)
    kl = R.row_kl(ht[:, 1:], hs[:, 1:], head_sizes)
    dv2 = (hs[:, 0] - ht[:, 0]) ** 2
    assert ref["n_valid"] == 7.0
    assert abs(ref["kl_sum"] - float(kl[valid].sum())) < 1e-12 and abs(ref["dv2_sum"] - float(dv2[valid].sum())) < 1e-12
    assert abs(ref["loss"] - (0.3 * float(kl[valid].sum()) + 0.7 * float(dv2[valid].sum())) / 7.0) < 1e-12
    assert ref["kl_max"] == float(kl[valid].max())
    g = ref["g"]
    assert g.shape == (9, 1 + 8) and not g[~valid].any() and g[valid].abs().min() > 0
    # the closed forms the header states: p_s - p_t; (mu_s - mu_t) / sd_s^2; 1 - vr - dl^2; 2 (v_s - v_t)
    pt, ps = torch.softmax(ht[:, 1:5], -1), torch.softmax(hs[:, 1:5], -1)
    sdt, sds = ht[:, 7:9].exp(), hs[:, 7:9].exp()
    dl = (ht[:, 5:7] - hs[:, 5:7]) / sds
    want = torch.cat([(0.7 / 7.0 * 2.0 * (hs[:, 0] - ht[:, 0]))[:, None], 0.3 / 7.0 * (ps - pt),
                      0.3 / 7.0 * (hs[:, 5:7] - ht[:, 5:7]) / sds ** 2, 0.3 / 7.0 * (1.0 - (sdt / sds) ** 2 - dl ** 2)], dim=1)
    assert torch.allclose(g[valid], want[valid], rtol=1e-10, atol=1e-14)
    # an explicit divisor (the learner's global valid count) scales loss and gradient alike
    half = R.consistency_reference(ht, hs, valid, head_sizes, 0.3, 0.7, n_valid=14)
    assert abs(half["loss"] - ref["loss"] / 2) < 1e-15 and torch.allclose(half["g"], g / 2, rtol=1e-14, atol=0)
    # equal rows: nothing, up to float64 rounding of the softmax gradient (the kernel's own zero is exact by construction)
    same = R.consistency_reference(ht, ht.clone(), valid, head_sizes, 0.3, 0.7)
    assert abs(same["kl_sum"]) < 1e-15 and same["dv2_sum"] == 0.0 and same["g"].abs().max() < 1e-15


def test_yardstick_clamps_the_standard_deviation_as_the_loss_does():
    ht = torch.tensor([[0.0, 0.5, 0.0]], dtype=torch.float64)
    hs = torch.tensor([[0.0, 0.0, -12.0]], dtype=torch.float64)   # exp(-12) < 1e-4: the student's sd sits at the clamp
    ref = R.consistency_reference(ht, hs, torch.ones(1, dtype=torch.bool), [-1], 1.0, 1.0)
    sd = 1e-4
    assert abs(ref["kl_sum"] - (torch.log(torch.tensor(sd, dtype=torch.float64)).item() + (1 + 0.25) / (2 * sd * sd) - 0.5)) \
        < 1e-6 * ref["kl_sum"]
    assert ref["g"][0, 2] == 0.0 and ref["g"][0, 1] < 0                 # log_std does not move beyond the clamp; the mean does
