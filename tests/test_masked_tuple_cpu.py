"""Tuple action spaces under an action mask, the parts that need no GPU: the additive entry point
sf_sample_write_step_tuple_masked (exported, declared, refusing bad arguments on the host), the float64 per-member
composition that judges the GPU kernels (masked_tuple_ref) held to the TupleActionDistribution object, and the rollout
runner's check of the mask's width."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from sample_factory_amd.envs import spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sf_sample_write_step_tuple_masked"


def n_params(heads):
    return sum(h if h > 0 else -2 * h for h in heads)


def masked_tuple_ref(logits, mask, heads):
    """float64, per Discrete member on the mask columns under its own logits (a Box member's columns are not read):
    p = softmax over the allowed actions (an all-zero slice: uniform over all of them), log p = log_softmax of
    z + (mask == 0) * -1e9.  Returns [(probabilities [B, n], log-probabilities [B, n], allowed [B, n]) | None (Box)]"""
    out, off = [], 0
    for h in heads:
        if h < 0:
            out.append(None)
            off += -2 * h
            continue
        z = np.asarray(logits[:, off:off + h], np.float64)
        m = np.asarray(mask[:, off:off + h]) != 0
        none = ~m.any(1)
        zm = np.where(none[:, None], 0.0, np.where(m, z, -np.inf))
        zm = zm - zm.max(1, keepdims=True)
        p = np.exp(zm)
        p /= p.sum(1, keepdims=True)
        zp = z + np.where(m, 0.0, -1e9)
        zp = zp - zp.max(1, keepdims=True)
        logp = zp - np.log(np.exp(zp).sum(1, keepdims=True))
        out.append((p, logp, np.where(none[:, None], True, m)))
        off += h
    return out


def _tuple(heads):
    return spaces.Tuple([spaces.Discrete(h) if h > 0 else spaces.Box(-1.0, 1.0, (-h,), np.float32) for h in heads])


def test_library_exports_the_masked_tuple_sampler_and_keeps_the_abi():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert ENTRY in lib.SYMBOLS and re.search(r"\bint\s+" + ENTRY + r"\s*\(", text)
    assert hasattr(L, ENTRY) and hasattr(L, "sf_sample_write_step_tuple") and hasattr(L, "sf_sample_write_step_masked")
    assert L.sf_abi_version() == 19
    assert callable(lib.sample_write_step_tuple_masked)


def test_bad_arguments_are_refused_on_the_host():
    """made-up non-null addresses: a refusal comes before anything is read or launched, so this returns -1 on a machine
    with no GPU.  A null mask, ld_mask < A, and the head-list refusals of sf_sample_write_step_tuple; every message names
    the entry point"""
    from sample_factory_amd import lib
    L = lib.load()
    p, f = C.c_void_p(4096), C.c_float
    arr = lambda hs: (C.c_int32 * len(hs))(*hs)
    err = lambda: L.sf_last_error().decode()

    def sw(hs, n, env_a, mask=p, ld_mask=1 << 20):
        return getattr(L, ENTRY)(p, 1 << 20, p, 1, mask, C.c_int64(ld_mask), 16, n, arr(hs), 2, 0, 1, 1, 0, f(0.0), 0, p,
                                 p, p, p, p, env_a, None)

    assert sw([4, 3], 2, p, mask=None) == -1 and ENTRY in err() and "mask" in err()
    assert sw([4, 3], 2, p, ld_mask=6) == -1 and ENTRY in err() and "ld_mask=6" in err() and "A=7" in err()
    assert sw([5, -2, 7], 3, None, ld_mask=15) == -1 and ENTRY in err() and "A=16" in err()  # Box columns count
    assert sw([129, 3], 2, p, ld_mask=131) == -1 and ENTRY in err() and "A=132" in err()     # wave-per-row width
    assert sw([2] * 65, 65, None) == -1 and ENTRY in err() and "limit is 64" in err()
    assert sw([3] * 9, 0, None) == -1 and ENTRY in err() and "limit is 64" in err()
    assert sw([3] * 8 + [0], 9, None) == -1 and ENTRY in err() and "empty action head" in err()
    assert sw([3] * 9 + [-2], 10, p) == -1 and ENTRY in err() and "Box member" in err()


def test_binding_refuses_a_mask_that_is_not_a_u8_device_tensor():
    from sample_factory_amd import lib
    t = torch.zeros(4, 7)
    with pytest.raises(lib.SfHipError, match="u8/bool CUDA tensor"):
        lib.sample_write_step_tuple_masked(t, 7, t, 1, torch.zeros(4, 7), 7, 4, [4, 3], 2, 0, 1, 1, 0, 0.0, False, t, t, t,
                                           t, t, None)


@pytest.mark.parametrize("heads", [[2, 3], [6, 1, 5], [5, -2, 7], [3] * 12, [21] * 8], ids=str)
def test_tuple_distribution_object_equals_the_per_member_composition(heads):
    """TupleActionDistribution with a [B, A] mask, CPU float64: per Discrete member the probabilities and log-probabilities
    are those of masked_tuple_ref on the member's own mask columns (1e-12: two float64 evaluations of one softmax, the
    object's carrying the reference's + 1e-13 in the renormalisation), a member whose slice is all zero has probability
    zero everywhere and samples in range, a Box member ignores its columns, and the row's log-prob is the members' sum"""
    from sample_factory_amd.algo.utils.action_distributions import TupleActionDistribution
    B, A = 64, n_params(heads)
    rng = np.random.default_rng(A)
    logits = rng.standard_normal((B, A)) * 3
    mask = (rng.random((B, A)) < 0.5).astype(np.uint8)
    off = 0
    for h in heads:
        if h > 0:
            mask[0::4, off:off + h] = 0
            mask[0::4, off] = 1              # first only
            mask[1::4, off:off + h] = 0
            mask[1::4, off + h - 1] = 1      # last only
            mask[2::4, off:off + h] = 0      # none
            mask[3::4, off + h // 2] = 1     # a random half and one fixed column
        else:
            mask[:, off:off - 2 * h] = 0
        off += h if h > 0 else -2 * h
    ref = masked_tuple_ref(logits, mask, heads)
    dist = TupleActionDistribution(_tuple(heads), torch.tensor(logits), torch.tensor(mask).double())
    torch.manual_seed(0)
    actions = dist.sample()
    lp_want = np.zeros(B)
    col = 0
    for h, d, r in zip(heads, dist.distributions, ref):
        if h < 0:
            assert r is None and not hasattr(d, "action_mask")
            lp_want += d.log_prob(actions[:, col:col - h]).numpy()
            col += -h
            continue
        p, logp, allowed = r
        none = np.arange(B) % 4 == 2
        got_p = d.probs.numpy()
        np.testing.assert_allclose(got_p[~none], p[~none], rtol=1e-12, atol=1e-12)
        assert np.all(got_p[none] == 0)     # (the object's sample() then draws uniformly, as the kernel does)
        np.testing.assert_allclose(d.log_probs.numpy(), logp, rtol=1e-12, atol=1e-12 * 1e9)
        np.testing.assert_allclose(d.log_probs.numpy()[allowed & ~none[:, None]], logp[allowed & ~none[:, None]],
                                   rtol=1e-12, atol=1e-12)
        a = actions[:, col].numpy().astype(np.int64)
        assert np.all((a >= 0) & (a < h)) and np.all(allowed[np.arange(B), a])
        assert np.all(a[0::4] == 0) and np.all(a[1::4] == h - 1)
        lp_want += logp[np.arange(B), a]
        col += 1
    some = np.arange(B) % 4 != 2
    np.testing.assert_allclose(dist.log_prob(actions).numpy()[some], lp_want[some], rtol=1e-12, atol=1e-12)


def _runner_args(heads, mask_cols, n_params_model):
    B, T = 4, 2
    traj = {"rewards": torch.zeros(B, T), "obs": {"obs": torch.zeros(B, T + 1, 3),
                                                  "action_mask": torch.zeros(B, T + 1, mask_cols, dtype=torch.uint8)}}
    env = types.SimpleNamespace(num_agents=B)
    info = types.SimpleNamespace(action_space=_tuple(heads) if len(heads) > 1 else spaces.Box(-1.0, 1.0, (2,), np.float32))
    ac = types.SimpleNamespace(device=torch.device("cpu"), num_action_params=n_params_model)
    return types.SimpleNamespace(rollout=T), info, env, ac, traj


def test_runner_checks_the_width_of_the_mask():
    """one mask column per distribution parameter: Tuple(Discrete(4), Box(2), Discrete(3)) has 11, a mask of 7 columns
    (one per Discrete action) is refused with both numbers and the convention; a pure Box space stays refused"""
    from sample_factory_amd.algo.sampling.batched_sampling import BatchedVectorEnvRunner
    with pytest.raises(ValueError, match=r"7 columns.*11 distribution parameters.*one column per\s+distribution parameter"):
        BatchedVectorEnvRunner(*_runner_args([4, -2, 3], 7, 11))
    with pytest.raises(ValueError, match=r"8 columns.*7 distribution parameters"):
        BatchedVectorEnvRunner(*_runner_args([4, 3], 8, 7))
    with pytest.raises(NotImplementedError, match="pure Box"):
        BatchedVectorEnvRunner(*_runner_args([-2], 4, 4))
