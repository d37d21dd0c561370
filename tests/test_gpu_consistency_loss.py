"""sf_consistency_loss (csrc/sf_rl.hip) against the float64 yardstick of tests/consistency_refs.py.

The launch sees two halves of ONE sentinel-filled heads-gradient matrix, as the learner hands them over: target rows
[0, n), student rows [n, 2n), a few rows behind them, and guard columns beyond 1 + A.  Tolerances are check_loss's of
tests/test_gpu_action_heads.py: scalars to 1e-6 + 2e-5 |ref|, the largest KL to 1e-4 relative, gradients to rtol 5e-4 with
atol 1e-5 of the largest reference gradient.  Logits ~ N(0, 2^2) and log_std uniform in [-2, 2]: no row is at the box_sd
clamp (asserted on the data), so no row is left out.

Which list reaches which kernel: up to 128 parameters k_consistency_loss (one lane per row; 259 rows = one full 256-thread
block and a partial wave of a second), above k_consistency_loss_wide (one wave per row, 67 rows = 17 blocks, the last with
three rows).  The 9-member list is longer than the 8 members sf_loss_cfg holds."""
import numpy as np
import pytest
import torch

from tests import consistency_refs as R

pytestmark = pytest.mark.gpu

SENT = -7.0
NINE = [3, 2, -2, 4, 2, 5, 3, 2, 6]            # 9 members, one of them Box(2): 31 parameters
NARROW = [[2], [8], [9], [33], [128], [-1], [-5], [-64], [3, -2, 5], NINE]
WIDE = [[200], [130, 3], [-70]]
CP, CV = 0.3, 0.7
EXTRA_ROWS, GUARD = 5, 3


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def _ident(heads):
    return "-".join(str(h) for h in heads) if len(heads) < 9 else f"{len(heads)}members"


def make_heads(g, heads, rows):
    """[rows, 1 + A] float32: value ~ N(0, 1), logits and means ~ N(0, 2^2), log_std uniform in [-2, 2]"""
    A = R.num_params(heads)
    h = torch.randn(rows, 1 + A, generator=g) * 2.0
    h[:, 0] *= 0.5
    for kind, off, size in R.member_slices(heads):
        if kind == "box":
            ls = torch.rand(rows, size, generator=g) * 4.0 - 2.0
            assert (ls.exp() > 1e-4).all() and (ls.exp() < 1e4).all()      # no row at the box_sd clamp
            h[:, 1 + off + size:1 + off + 2 * size] = ls
    return h


def run(lib, heads, n, *, use_index, same=False, seed=0):
    """one launch as the learner makes it; returns everything the checks need, on the host"""
    g = torch.Generator().manual_seed(1000 + 31 * abs(sum(heads)) + len(heads) + seed)
    A = R.num_params(heads)
    ld = 1 + A + GUARD
    N = 3 * n
    ht = make_heads(g, heads, n)
    hs = ht.clone() if same else make_heads(g, heads, n)
    valids = torch.rand(N, generator=g) > 0.15
    if use_index:
        index = torch.randperm(N, generator=g)[:n].to(torch.int32)
        offset, rows = 0, index.long()
    else:
        index, offset = None, n + 7
        rows = torch.arange(offset, offset + n)
    valid = valids[rows]
    assert 0 < int(valid.sum()) < n
    n_global = float(valid.sum()) + 17.0                                    # the GLOBAL count is the divisor, not the local one
    mat = torch.full((2 * n + EXTRA_ROWS, ld), SENT)
    mat[:n, :1 + A], mat[n:2 * n, :1 + A] = ht, hs
    d_heads = mat.cuda()
    d_g = torch.full_like(d_heads, SENT)
    before = d_heads.clone()
    mom = torch.tensor([0.3, 1.7, n_global], dtype=torch.float64, device="cuda")
    sums = torch.full((4,), 123.0, dtype=torch.float64, device="cuda")     # the call zeroes them
    kind = 1 if len(heads) == 1 and heads[0] < 0 else 0
    lib.consistency_loss(d_heads[:n, 1:], d_heads[n:2 * n, 1:], ld, d_heads[:n, 0], d_heads[n:2 * n, 0], ld, valids.cuda(),
                         None if index is None else index.cuda(), offset, n, A, kind, CP, CV, mom, sums,
                         d_g[n:2 * n, 1:], d_g[n:2 * n, 0], head_sizes=heads)
    torch.cuda.synchronize()
    assert torch.equal(d_heads, before)                                     # the heads are read only
    return dict(A=A, ht=ht, hs=hs, valid=valid, n_global=n_global, sums=sums.cpu().numpy(), g=d_g.cpu())


def check_untouched(out, n):
    A, g = out["A"], out["g"]
    assert (g[:n] == SENT).all(), "the target rows' gradient memory was written"
    assert (g[2 * n:] == SENT).all(), "rows behind the student half were written"
    assert (g[n:2 * n, 1 + A:] == SENT).all(), "guard columns beyond 1 + A were written"
    assert not (g[n:2 * n, :1 + A] == SENT).any()


def check_against_yardstick(out, heads, n, what):
    ref = R.consistency_reference(out["ht"], out["hs"], out["valid"], heads, CP, CV, n_valid=out["n_global"])
    s, A = out["sums"], out["A"]
    got = dict(kl_sum=s[0], dv2_sum=s[1], kl_mean=s[0] / s[3], dv2_mean=s[1] / s[3],
               loss=(CP * s[0] + CV * s[1]) / out["n_global"])
    want = dict(kl_sum=ref["kl_sum"], dv2_sum=ref["dv2_sum"], kl_mean=ref["kl_sum"] / ref["n_valid"],
                dv2_mean=ref["dv2_sum"] / ref["n_valid"], loss=ref["loss"])
    print(what, {k: (float(got[k]), want[k]) for k in got}, "kl_max", float(s[2]), ref["kl_max"])
    assert s[3] == ref["n_valid"], (what, s[3], ref["n_valid"])
    for k in got:
        assert abs(got[k] - want[k]) <= 1e-6 + 2e-5 * abs(want[k]), (what, k, got[k], want[k])
    assert abs(s[2] - ref["kl_max"]) <= 1e-4 * max(1.0, abs(ref["kl_max"])), (what, "kl_max", s[2], ref["kl_max"])
    g = out["g"][n:2 * n, :1 + A].double().numpy()
    gr = ref["g"].numpy()
    np.testing.assert_allclose(g[:, 1:], gr[:, 1:], rtol=5e-4, atol=1e-5 * np.abs(gr[:, 1:]).max(), err_msg=f"{what} g_params")
    np.testing.assert_allclose(g[:, 0], gr[:, 0], rtol=5e-4, atol=1e-5 * np.abs(gr[:, 0]).max(), err_msg=f"{what} g_values")
    invalid = ~out["valid"].numpy()
    assert invalid.any() and np.all(g[invalid] == 0.0), (what, "an invalid row has a gradient")
    assert np.all(np.abs(g[~invalid]).max(1) > 0.0)


@pytest.mark.parametrize("heads", NARROW, ids=_ident)
def test_lane_per_row_kernel_through_a_shuffled_index(lib, heads):
    n = 259
    out = run(lib, heads, n, use_index=True)
    check_untouched(out, n)
    check_against_yardstick(out, heads, n, f"narrow {heads}")


@pytest.mark.parametrize("heads", WIDE, ids=_ident)
def test_wave_per_row_kernel_through_a_shuffled_index(lib, heads):
    n = 67
    out = run(lib, heads, n, use_index=True)
    check_untouched(out, n)
    check_against_yardstick(out, heads, n, f"wide {heads}")


@pytest.mark.parametrize("heads,n", [([3, -2, 5], 259), ([130, 3], 67)], ids=["narrow", "wide"])
def test_rows_through_an_offset(lib, heads, n):
    out = run(lib, heads, n, use_index=False, seed=5)
    check_untouched(out, n)
    check_against_yardstick(out, heads, n, f"offset {heads}")


@pytest.mark.parametrize("heads,n", [([9], 259), ([-5], 259), (NINE, 259), ([200], 67), ([130, 3], 67), ([-70], 67)],
                         ids=lambda v: _ident(v) if isinstance(v, list) else str(v))
def test_identical_rows_give_exactly_nothing(lib, heads, n):
    out = run(lib, heads, n, use_index=True, same=True, seed=9)
    check_untouched(out, n)
    s = out["sums"]
    assert s[0] == 0.0 and s[1] == 0.0 and s[2] == 0.0 and s[3] == float(out["valid"].sum()), s
    assert (out["g"][n:2 * n, :1 + out["A"]] == 0.0).all()


def test_the_wrapper_takes_a_one_member_list_and_none_alike(lib):
    """head_sizes None, [A] and [-D] are the single space of action_kind; a wrong one-member list is refused by the library"""
    n, A = 64, 6
    g = torch.Generator().manual_seed(3)
    heads = torch.randn(2 * n, 1 + A, generator=g).cuda()
    valids = torch.ones(n, dtype=torch.bool, device="cuda")
    mom = torch.tensor([0.0, 0.0, float(n)], dtype=torch.float64, device="cuda")
    outs = []
    for kind, hs_ in ((0, None), (0, [A]), (1, None), (1, [-3])):
        gh = torch.zeros_like(heads)
        sums = torch.zeros(4, dtype=torch.float64, device="cuda")
        lib.consistency_loss(heads[:n, 1:], heads[n:, 1:], 1 + A, heads[:n, 0], heads[n:, 0], 1 + A, valids, None, 0, n, A, kind,
                             CP, CV, mom, sums, gh[n:, 1:], gh[n:, 0], head_sizes=hs_)
        outs.append((sums.cpu(), gh.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[2][0], outs[3][0]) and torch.equal(outs[2][1], outs[3][1])
    assert not torch.equal(outs[0][1], outs[2][1])
    with pytest.raises(lib.SfHipError, match="sf_consistency_loss"):
        lib.consistency_loss(heads[:n, 1:], heads[n:, 1:], 1 + A, heads[:n, 0], heads[n:, 0], 1 + A, valids, None, 0, n, A, 0,
                             CP, CV, mom, torch.zeros(4, dtype=torch.float64, device="cuda"), heads[n:, 1:], heads[n:, 0],
                             head_sizes=[4, 1])
