"""sf_sample_write_step_tuple_masked (csrc/sf_rl.hip: k_sample_write_masked_tuple up to 128 distribution parameters,
k_sample_write_wide above) against float64 numpy: per Discrete member the masked softmax / log-softmax on the mask
columns under the member's own logits (masked_tuple_ref of tests/test_masked_tuple_cpu.py, whose single-head form
tests/golden/action_dist.npz pins to the reference), per Box member the float64 Box-Muller draw.  Never another GPU path.

4096 rows, logits of scale 3, the mask in a [B, T + 1, A] u8 slab (row stride (T + 1) * A > A; the other steps hold the
complement of the mask, so a launch that read another step's row would draw masked-out actions).  Per member a row's
mask is one of four kinds: only the first action allowed, only the last, none, a random half plus one fixed column.
Rows 0-3 of every eight give all members the same kind (so that rows 0, 1 and 3 have no all-zero member and their
log-prob is checked, and row 2 masks every member out); rows 4-7 rotate the kind with the member index, so neighbouring
members of one row carry different kinds and a member that read its neighbour's columns is caught.

Rows that differ from the float64 first crossing (cap: 0.5 % = 20 of 4096 per member): a numpy emulation of the
lane-per-row kernel's float32 arithmetic (sequential float32 sums, numpy's float32 exp and log) on exactly these
inputs, with the real Philox uniforms of uniforms_discrete, gives 0 differing rows of 4096 for every Discrete member of
every head list below (tools/masked_tuple_emulation.py prints the counts).  The kernels themselves, on one MI355X: 0 rows
of 4096 for every member of every list as well, and a largest log-prob error of 3.5e-6 ([3] * 40, sums of 40 terms)."""
import numpy as np
import pytest
import torch

from test_gpu_action_heads import (SENT, _read_slab, _slab, dev, log_softmax64, logp_tol, normal_logp64, normals,
                                   uniforms_discrete)
from test_gpu_wide_action_heads import check_wide_draw, tuple_logits
from test_masked_tuple_cpu import masked_tuple_ref, n_params

pytestmark = pytest.mark.gpu

B = 4096
NARROW = [[2, 3], [6, 1, 5], [5, -2, 7], [3] * 40, [64, 64]]              # A <= 128: one lane per row
WIDE = [[129, 3], [5, 300, -2, 7], [21] * 8, [63, 65, 64]]               # A >= 129: one wave per row
HEAD_LISTS = NARROW + WIDE


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def member_kinds(hs):
    """[B, members]: 0 first only, 1 last only, 2 none, 3 a random half plus one fixed column"""
    base = np.arange(B) % 8
    return np.stack([np.where(base < 4, base, (base + h_i) % 4) for h_i in range(len(hs))], 1)


def make_case(hs):
    """(logits, values, mask u8 [B, A], kinds [B, members]); the columns under a Box member are zero"""
    rng = np.random.default_rng(1000 * len(hs) + n_params(hs))
    logits = tuple_logits(rng, hs, B, 3.0)
    values = rng.standard_normal(B).astype(np.float32)
    mask = np.zeros((B, n_params(hs)), np.uint8)
    kinds = member_kinds(hs)
    off = 0
    for h_i, h in enumerate(hs):
        if h < 0:
            off += -2 * h
            continue
        m, k = mask[:, off:off + h], kinds[:, h_i]
        m[k == 0, 0] = 1
        m[k == 1, -1] = 1
        r3 = np.flatnonzero(k == 3)
        m[r3] = rng.random((len(r3), h)) < 0.5
        m[r3, h_i % h] = 1
        off += h
    return logits, values, mask, kinds


def run_masked_tuple(lib, logits, values, mask, hs, *, seed, step, row0, deterministic=False, T=2, t=1):
    """one launch on [values | logits | pad] heads with the mask at step t of a [B, T + 1, A] slab -> (actions, logp)"""
    A = logits.shape[1]
    nact = sum(1 if h > 0 else -h for h in hs)
    heads = dev(np.concatenate([values[:, None], logits, np.zeros((B, 1), np.float32)], 1))
    ld = heads.shape[1]
    slab_mask = (1 - dev(mask, torch.uint8))[:, None, :].repeat(1, T + 1, 1).contiguous()
    slab_mask[:, t] = dev(mask, torch.uint8)
    mview = slab_mask[:, t]
    assert mview.stride(0) == (T + 1) * A > A
    tr = _slab(B, T, nact, A)
    env_a = torch.full((B, len(hs)), -5, dtype=torch.int32, device="cuda") if all(h > 0 for h in hs) else None
    lib.sample_write_step_tuple_masked(heads[:, 1:], ld, heads[:, 0], ld, mview, mview.stride(0), B, hs, T, t, seed, step,
                                       row0, 6.0, deterministic, tr["actions"], tr["logits"], tr["logp"], tr["values"],
                                       tr["ver"], env_a)
    torch.cuda.synchronize()
    a, lp = _read_slab(tr, logits, values, t, 6.0)
    if env_a is not None:
        np.testing.assert_array_equal(env_a.cpu().numpy(), a.astype(np.int32))
    return a, lp


def run_unmasked_tuple(lib, logits, values, hs, *, seed, step, row0, T=2, t=1):
    nact = sum(1 if h > 0 else -h for h in hs)
    heads = dev(np.concatenate([values[:, None], logits, np.zeros((B, 1), np.float32)], 1))
    tr = _slab(B, T, nact, logits.shape[1])
    lib.sample_write_step_tuple(heads[:, 1:], heads.shape[1], heads[:, 0], heads.shape[1], B, hs, T, t, seed, step, row0,
                                6.0, False, tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], None)
    torch.cuda.synchronize()
    return _read_slab(tr, logits, values, t, 6.0)


@pytest.mark.parametrize("hs", HEAD_LISTS, ids=str)
def test_masked_tuple_sampler_vs_float64(lib, hs):
    """per Discrete member: the draw is in range, never masked out, never of zero probability, its float64 CDF interval
    within 1e-5 of its Philox uniform (counter (step, h, 2, 0)), and at most 0.5 % of the rows differ from the float64
    first crossing (emulation of the kernel's f32 arithmetic with the real uniforms: 0 rows, see the module docstring);
    first-only / last-only rows draw exactly that action; an all-zero slice draws uniformly.  Box members draw
    mu + sd * eps from counter (step, k / 2, 3, h) and ignore their (zero) mask columns.  The row's log-prob is the
    float64 sum of the members' masked log-softmax / Normal log-density at the recorded actions, within logp_tol (plus,
    per Box member, 2e-6 of the size of its terms, the bound of the unmasked Tuple tests), on rows with no all-zero
    member.  env_actions, recorded logits / values / version and the other steps' sentinels: run_masked_tuple."""
    seed, step, row0 = 31 + len(hs), 12, 70001 + n_params(hs)
    A = n_params(hs)
    logits, values, mask, kinds = make_case(hs)
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    a, lp = run_masked_tuple(lib, logits, values, mask, hs, seed=seed, step=step, row0=row0)
    ref = masked_tuple_ref(logits, mask, hs)
    r = np.arange(B)
    lp_want, box_size = np.zeros(B), np.zeros(B)
    off = col = 0
    for h_i, h in enumerate(hs):
        if h > 0:
            p, logp, allowed = ref[h_i]
            u = uniforms_discrete(seed, step, rows, head=h_i)
            diff = check_wide_draw(a[:, col], p, u, f"{hs} member {h_i}", allowed=allowed)
            print(f"{hs} member {h_i}: {int(diff.sum())} of {B} rows differ from the float64 first crossing")
            k = kinds[:, h_i]
            assert np.all(a[k == 0, col] == 0) and np.all(a[k == 1, col] == h - 1), (hs, h_i)
            lp_want += logp[r, a[:, col].astype(np.int64)]
            off, col = off + h, col + 1
        else:
            D = -h
            assert ref[h_i] is None and not mask[:, off:off + 2 * D].any()
            mu, ls_ = logits[:, off:off + D], logits[:, off + D:off + 2 * D]
            sd = np.clip(np.exp(ls_.astype(np.float64)), 1e-4, 1e4)
            want = mu + sd * normals(seed, step, rows, D, member=h_i)
            got = a[:, col:col + D]
            np.testing.assert_array_less(np.abs(got - want), 1e-5 * (1 + np.abs(want)) + 4e-6 * sd)
            t = normal_logp64(got, mu, ls_)
            lp_want += t.sum(1)
            box_size += D + np.abs(t).sum(1)
            off, col = off + 2 * D, col + D
    some = ~(kinds == 2)[:, [i for i, h in enumerate(hs) if h > 0]].any(1)
    assert some.sum() >= 3 * B // 8
    err = np.abs(lp - lp_want)
    print(f"{hs}: max |log-prob - float64| on {int(some.sum())} rows {err[some].max():.3e}")
    np.testing.assert_array_less(err[some], (logp_tol(lp_want, A) + 2e-6 * box_size)[some])


@pytest.mark.parametrize("hs", HEAD_LISTS, ids=str)
def test_masked_tuple_sampler_deterministic(lib, hs):
    """each Discrete member takes the first arg-max over its allowed actions, an all-zero member action 0, a Box member
    its means; the log-prob is the float64 sum at those actions"""
    seed, step, row0 = 5, 3, 900 + n_params(hs)
    logits, values, mask, kinds = make_case(hs)
    a, lp = run_masked_tuple(lib, logits, values, mask, hs, seed=seed, step=step, row0=row0, deterministic=True)
    ref = masked_tuple_ref(logits, mask, hs)
    r = np.arange(B)
    lp_want, box_size = np.zeros(B), np.zeros(B)
    off = col = 0
    for h_i, h in enumerate(hs):
        if h > 0:
            _, logp, _ = ref[h_i]
            m = mask[:, off:off + h] != 0
            want = np.where(m.any(1), np.argmax(np.where(m, logits[:, off:off + h].astype(np.float64), -np.inf), 1), 0)
            np.testing.assert_array_equal(a[:, col], want, err_msg=f"{hs} member {h_i}")
            lp_want += logp[r, want]
            off, col = off + h, col + 1
        else:
            D = -h
            mu, ls_ = logits[:, off:off + D], logits[:, off + D:off + 2 * D]
            np.testing.assert_array_equal(a[:, col:col + D], mu)
            t = normal_logp64(mu, mu, ls_)
            lp_want += t.sum(1)
            box_size += D + np.abs(t).sum(1)
            off, col = off + 2 * D, col + D
    some = ~(kinds == 2)[:, [i for i, h in enumerate(hs) if h > 0]].any(1)
    np.testing.assert_array_less(np.abs(lp - lp_want)[some], (logp_tol(lp_want, n_params(hs)) + 2e-6 * box_size)[some])


@pytest.mark.parametrize("hs", HEAD_LISTS, ids=str)
def test_all_ones_mask_is_the_unmasked_distribution(lib, hs):
    """a mask of ones changes nothing that is defined without it: every member's draw passes the float64 inverse-CDF check
    of the unmasked softmax, the row's log-prob is the float64 unmasked sum within logp_tol, and a Box member's actions
    are bit-equal to what sf_sample_write_step_tuple records for the same seed, step and rows"""
    seed, step, row0 = 77, 9, 12345
    A = n_params(hs)
    logits, values, _, _ = make_case(hs)
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    a, lp = run_masked_tuple(lib, logits, values, np.ones((B, A), np.uint8), hs, seed=seed, step=step, row0=row0)
    a_un, _ = run_unmasked_tuple(lib, logits, values, hs, seed=seed, step=step, row0=row0)
    r = np.arange(B)
    lp_want, box_size = np.zeros(B), np.zeros(B)
    off = col = 0
    for h_i, h in enumerate(hs):
        if h > 0:
            ls = log_softmax64(logits[:, off:off + h])
            check_wide_draw(a[:, col], np.exp(ls), uniforms_discrete(seed, step, rows, head=h_i), f"{hs} member {h_i}")
            lp_want += ls[r, a[:, col].astype(np.int64)]
            off, col = off + h, col + 1
        else:
            D = -h
            got = a[:, col:col + D]
            assert np.array_equal(got.view(np.uint32), a_un[:, col:col + D].view(np.uint32)), (hs, h_i)
            t = normal_logp64(got, logits[:, off:off + D], logits[:, off + D:off + 2 * D])
            lp_want += t.sum(1)
            box_size += D + np.abs(t).sum(1)
            off, col = off + 2 * D, col + D
    np.testing.assert_array_less(np.abs(lp - lp_want), logp_tol(lp_want, A) + 2e-6 * box_size)


def test_bool_mask_and_host_mask(lib):
    """a bool mask is read like a u8 one, and a mask that is not on the device is refused by the binding"""
    hs = [6, 1, 5]
    logits, values, mask, _ = make_case(hs)
    heads = dev(np.concatenate([values[:, None], logits], 1))
    A = n_params(hs)
    out = []
    for dt in (torch.uint8, torch.bool):
        tr = _slab(B, 1, 3, A)
        mk = dev(mask, dt)
        lib.sample_write_step_tuple_masked(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, mk, A, B, hs, 1, 0, 4, 4, 4, 1.0, False,
                                           tr["actions"], tr["logits"], tr["logp"], tr["values"], tr["ver"], None)
        torch.cuda.synchronize()
        out.append((tr["actions"].cpu().numpy(), tr["logp"].cpu().numpy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert not np.any(out[0][0] == SENT)
    with pytest.raises(lib.SfHipError, match="u8/bool CUDA tensor"):
        lib.sample_write_step_tuple_masked(heads[:, 1:], 1 + A, heads[:, 0], 1 + A, torch.ones(B, A, dtype=torch.uint8), A,
                                           B, hs, 1, 0, 4, 4, 4, 1.0, False, tr["actions"], tr["logits"], tr["logp"],
                                           tr["values"], tr["ver"], None)
