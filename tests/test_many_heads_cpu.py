"""Tuple action spaces of more than eight members, the parts that need no GPU: the head list action_head_sizes hands to
the sampler, the learner and the env workers (up to SF_MAX_ACTION_HEADS = 64 members, a refusal that names the limit
above it), the library's additive entry point for such lists, and the float64 restatement that judges the GPU kernels
(dist_terms of tests/test_gpu_action_heads.py) held to numbers the reference itself produced for 17- and 11-member
Tuples (tests/golden/action_dist_many_heads.npz, written by tools/gen_golden_many_heads.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sample_factory_amd.envs import spaces
from test_gpu_action_heads import dist_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tuple(heads):
    return spaces.Tuple([spaces.Discrete(h) if h > 0 else spaces.Box(-1.0, 1.0, (-h,), np.float32) for h in heads])


@pytest.mark.parametrize("heads", [(3,) * 9, (5,) * 17, (2,) * 64, (3,) * 9 + (-2, 4), (-1, 2) * 32], ids=len)
def test_action_head_sizes_takes_up_to_64_members(heads):
    from sample_factory_amd.envs.spaces import (MAX_ACTION_HEADS, action_head_sizes, calc_num_action_parameters,
                                                calc_num_actions, heads_action_cols)
    assert MAX_ACTION_HEADS == 64
    sp = _tuple(heads)
    assert action_head_sizes(sp) == list(heads)
    assert calc_num_action_parameters(sp) == sum(h if h > 0 else -2 * h for h in heads)
    assert calc_num_actions(sp) == heads_action_cols(list(heads)) == sum(1 if h > 0 else -h for h in heads)


def test_action_head_sizes_refuses_65_members_and_names_the_limit():
    from sample_factory_amd.envs.spaces import action_head_sizes
    with pytest.raises(NotImplementedError, match=r"at most 64 action heads"):
        action_head_sizes(_tuple((2,) * 65))


def test_header_binding_and_spaces_agree_on_the_limit():
    from sample_factory_amd import lib
    from sample_factory_amd.envs.spaces import MAX_ACTION_HEADS
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert int(re.search(r"#define\s+SF_MAX_ACTION_HEADS\s+(\d+)", text).group(1)) == MAX_ACTION_HEADS == lib.MAX_ACTION_HEADS
    assert "sf_ppo_loss_heads" in lib.SYMBOLS and re.search(r"\bint\s+sf_ppo_loss_heads\s*\(", text)


def test_library_exports_the_head_list_entry_point_and_keeps_the_abi():
    """additive: the new symbol next to sf_ppo_loss, sf_loss_cfg and the ABI number as they were"""
    from sample_factory_amd import lib
    L = lib.load()
    assert hasattr(L, "sf_ppo_loss_heads") and hasattr(L, "sf_ppo_loss")
    assert L.sf_abi_version() == 19
    assert len(lib.sf_loss_cfg().head_n) == 8


def _loss_call(L, fn, A, cfg, tail):
    """a loss entry point on made-up non-null addresses: a head list that is refused is refused before anything is read
    or launched, so this returns -1 on a machine with no GPU"""
    p = C.c_void_p(4096)
    return getattr(L, fn)(p, A, p, 1, p, p, p, p, p, p, p, None, C.c_int64(0), C.c_int64(16), A, C.byref(cfg), p, p, p,
                          p, None, *tail, None)


def test_bad_head_lists_are_refused_on_the_host():
    """more than 64 members, an empty member, sizes that do not sum to A, a Box member with symmetric-KL exploration or
    with int32 env_actions: -1 and a message that names the entry point (and the limit), from every entry point"""
    from sample_factory_amd import lib
    L = lib.load()
    cfg = lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.5, value_loss_coeff=0.5, exploration_coeff=0.01,
                          exploration_kind=1, action_kind=0)
    arr = lambda hs: (C.c_int32 * len(hs))(*hs)
    err = lambda: L.sf_last_error().decode()
    assert _loss_call(L, "sf_ppo_loss_heads", 130, cfg, (arr([2] * 65), 65)) == -1
    assert "sf_ppo_loss_heads" in err() and "limit is 64" in err()
    assert _loss_call(L, "sf_ppo_loss_heads", 27, cfg, (arr([3] * 9), 0)) == -1 and "limit is 64" in err()
    assert _loss_call(L, "sf_ppo_loss_heads", 27, cfg, (None, 9)) == -1 and "sf_ppo_loss_heads" in err()
    assert _loss_call(L, "sf_ppo_loss_heads", 28, cfg, (arr([3] * 9), 9)) == -1 and "sum to 27, A = 28" in err()
    assert _loss_call(L, "sf_ppo_loss_heads", 24, cfg, (arr([3] * 8 + [0]), 9)) == -1 and "empty action head" in err()
    sym = lib.sf_loss_cfg(exploration_coeff=0.01, exploration_kind=2, action_kind=0)
    assert _loss_call(L, "sf_ppo_loss_heads", 31, sym, (arr([3] * 9 + [-2]), 10)) == -1 and "categorical heads only" in err()
    # sf_ppo_loss reads the struct, which holds eight members: nine are refused as before
    cfg.num_heads = 9
    assert _loss_call(L, "sf_ppo_loss", 27, cfg, ()) == -1 and "sf_ppo_loss:" in err() and "limit is 8" in err()
    p, f = C.c_void_p(4096), C.c_float
    vt = lambda A, hs, n: L.sf_vtrace(p, A, p, 1, p, p, p, p, None, C.c_int64(0), C.c_int64(16), A, 0, 8, f(0.99), f(1.0),
                                      f(1.0), p, p, arr(hs), n, None)
    assert vt(130, [2] * 65, 65) == -1 and "sf_vtrace" in err() and "limit is 64" in err()
    assert vt(28, [3] * 9, 9) == -1 and "sum to 27, A = 28" in err()
    assert vt(24, [3] * 8 + [0], 9) == -1 and "empty action head" in err()
    sw = lambda hs, n, env_a: L.sf_sample_write_step_tuple(p, 1 << 20, p, 1, 16, n, arr(hs), 2, 0, 1, 1, 0, f(0.0), 0, p, p, p,
                                                           p, p, env_a, None)
    assert sw([2] * 65, 65, None) == -1 and "sf_sample_write_step_tuple" in err() and "limit is 64" in err()
    assert sw([3] * 9, 0, None) == -1 and "limit is 64" in err()
    assert sw([3] * 8 + [0], 9, None) == -1 and "empty action head" in err()
    assert sw([3] * 9 + [-2], 10, p) == -1 and "Box member" in err()


def test_head_arrays_are_sized_by_the_list():
    from sample_factory_amd import lib
    for n in (1, 8, 9, 64):
        a = lib._head_array([3] * (n - 1) + [-2])
        assert len(a) == n and a[n - 1] == -2 and C.sizeof(a) == 4 * n


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "action_dist_many_heads.npz"))


@pytest.mark.parametrize("tag,n_heads", [("h17x5", 17), ("h17x11", 17), ("h9x3_box2_4", 11)])
def test_float64_restatement_equals_the_reference_beyond_eight_members(golden, tag, n_heads):
    """log-prob, entropy, KL and symmetric KL per row: two float64 evaluations of the same sums, which differ in the order
    of up to ~200 additions and, for a Box member's KL, in the algebraic form (log(sd_o / sd) + ... against
    0.5 (ratio + ... - log ratio)) — 1e-10 relative leaves five digits over 200 * 2^-53 times a cancellation of 1e3"""
    heads = [int(h) for h in golden[f"{tag}.heads"]]
    assert len(heads) == n_heads > 8
    t = lambda k: torch.tensor(golden[f"{tag}.{k}"].astype(np.float64))
    lp, ent, kl, sym = dist_terms(t("logits"), t("old_logits"), t("actions"), heads)
    assert golden[f"{tag}.log_prob"].dtype == np.float64 and len(lp) == 16
    for got, key in ((lp, "log_prob"), (ent, "entropy"), (kl, "kl")):
        np.testing.assert_allclose(got.numpy(), golden[f"{tag}.{key}"], rtol=1e-10, atol=1e-10, err_msg=key)
    if all(h > 0 for h in heads):
        np.testing.assert_allclose(sym.numpy(), golden[f"{tag}.symmetric_kl"], rtol=1e-10, atol=1e-10)
    else:
        assert f"{tag}.symmetric_kl" not in golden.files
