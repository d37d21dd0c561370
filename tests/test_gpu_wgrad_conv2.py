"""The conv2 weight gradient k_wgrad_img<32, 20, 20, 4, 2, 2> (sf_nn_wimg.h; selected for n >= 512, one 8-wave work-group per
CU) after its two wave sets were set half a sample apart:
  * bit equality with tests/golden/wgrad_conv2_parent.npz, written by the commit before that change from the same host-drawn
    inputs (tools/gen_golden_wgrad_conv2.py): every accumulator must still see the same operands in the same order;
  * the edges of the sample walk against a float64 torch conv2d weight gradient, with the tolerance
    test_gpu_nn.py::test_conv_fwd_wgrad_dgrad_vs_torch uses for this geometry, and determinism of two launches;
  * stage hygiene: large finite values in the LAST sample of every work-group in one launch must not show in the next launch
    on ordinary inputs in the same buffers (a stale-stage read, or a DMA piece that lands after its reader)."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_wgrad_conv2", os.path.join(ROOT, "tools", "gen_golden_wgrad_conv2.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_conv2_parent.npz")


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


_cache = {}


def inputs_and_f64(n):
    """host inputs of gen.make_inputs(n, gen.seed_of(n)) and the float64 torch conv2d gradients (dW k-major [512, 64], db [64],
    on the CPU); computed once per n and shared, never modified.  The float64 convolution itself runs on the GPU: its backward
    pass takes 7 - 11 s on host cores at these n."""
    if n not in _cache:
        x, dy = gen.make_inputs(n, gen.seed_of(n))
        w = torch.zeros((gen.COUT, gen.CIN, gen.KS, gen.KS), dtype=torch.float64, device="cuda", requires_grad=True)
        b = torch.zeros(gen.COUT, dtype=torch.float64, device="cuda", requires_grad=True)
        xt = torch.from_numpy(x).cuda().double().permute(0, 3, 1, 2).contiguous()     # NCHW copy of the NHWC draw
        dyt = torch.from_numpy(dy).cuda().double().permute(0, 3, 1, 2).contiguous()
        F.conv2d(xt, w, b, stride=gen.ST).backward(dyt)
        dw = w.grad.permute(2, 3, 1, 0).reshape(gen.KS * gen.KS * gen.CIN, gen.COUT).contiguous().cpu()  # (kh, kw, c) x out
        _cache[n] = (x, dy, dw, b.grad.cpu())
    return _cache[n]


def check_f64(dw, db, dw_ref, db_ref, what):
    # test_conv_fwd_wgrad_dgrad_vs_torch's bound for this geometry: 3e-5 of the largest element (fp32 accumulation)
    e_w = (dw.cpu().double() - dw_ref).abs().max().item()
    e_b = (db.cpu().double() - db_ref).abs().max().item()
    s_w, s_b = dw_ref.abs().max().item(), db_ref.abs().max().item()
    print(f"{what}: wgrad err {e_w:.3e} (bound {3e-5 * max(1.0, s_w):.3e}), bgrad err {e_b:.3e} (bound {3e-5 * max(1.0, s_b):.3e})")
    assert e_w < 3e-5 * max(1.0, s_w), f"{what}: wgrad"
    assert e_b < 3e-5 * max(1.0, s_b), f"{what}: bgrad"


@pytest.mark.parametrize("n", gen.NS)
def test_bit_equal_to_the_parent_commit(lib, n):
    g = np.load(GOLDEN)
    assert int(g[f"seed_{n}"]) == gen.seed_of(n)
    x, dy = gen.make_inputs(n, gen.seed_of(n))
    dw, db = gen.run_wgrad(lib, torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda(), n)
    assert torch.equal(dw.cpu(), torch.from_numpy(g[f"dw_{n}"])), "dW differs in bits from the parent commit's"
    assert torch.equal(db.cpu(), torch.from_numpy(g[f"db_{n}"])), "db differs in bits from the parent commit's"


# 769: per = 4 on 256 work-groups, 193 used, the last holds ONE sample, the rest write zero partials; 1279: per = 5, the last
# work-group holds 4
@pytest.mark.parametrize("n", [769, 1279])
def test_edges_of_the_sample_walk_vs_float64(lib, n):
    x, dy, dw_ref, db_ref = inputs_and_f64(n)
    xd, dyd = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    dw, db = gen.run_wgrad(lib, xd, dyd, n)
    check_f64(dw, db, dw_ref, db_ref, f"n={n}")
    dw2, db2 = gen.run_wgrad(lib, xd, dyd, n)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two launches on the same inputs differ"


def test_stage_hygiene_after_large_values_in_last_samples(lib):
    n = 1279
    x, dy, dw_ref, db_ref = inputs_and_f64(n)
    d = gen.conv2_desc(lib)
    ws = torch.empty(lib.conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    xd, dyd = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    # the last sample of every work-group (per = ceil(n / 256) consecutive samples each; the last one ends at n - 1)
    per = -(-n // 256)
    last = torch.tensor(sorted({min(s + per - 1, n - 1) for s in range(0, n, per)}), device="cuda")
    xd[last] = 3.0e18   # finite, and so is every product (9e36 < 3.4e38)
    dyd[last] = 3.0e18
    gen.run_wgrad(lib, xd, dyd, n, ws)
    xd.copy_(torch.from_numpy(x))
    dyd.copy_(torch.from_numpy(dy))
    dw, db = gen.run_wgrad(lib, xd, dyd, n, ws)
    check_f64(dw, db, dw_ref, db_ref, "after a launch with 3e18 in the last samples")
