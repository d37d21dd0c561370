"""The forwards that write with an OUTPUT sample stride (sf_conv_fwd_relu_mask_os, sf_conv_fwd_t_os): sample s, pixel p goes
to out + s * out_sample_stride + p * Cout.  A rollout step writes slot t of a kept [E, T, OH*OW, Cout] buffer this way and
the learner's first minibatch reads rows of that buffer instead of running conv1..conv3 again, so the
strided kernels must produce the BYTES of the dense kernels the training launch would run.

Per layer of the Nature CNN (conv1 on u8 frames, conv2, conv3), slot 1 of T = 3 slots, the buffer pre-filled with NaN:
  * n = 258 (conv1 also 259: an odd last sample pair; conv2: 20898 rows = 163 tiles of 128 and a ragged one; conv3: 49-row
    samples straddling the 16-row fragments), conv2 also at n = 1620 (1026 row tiles: the last round runs as 64-row tiles)
    and conv3 at n = 514;
  * slots 0 and 2 and the guard band behind the buffer still hold their fill, every element of slot 1 is written;
  * against float64 at the kernel ledger's bounds (tests/test_gpu_kernel_ledger.py);
  * conv1's sign-bit words equal those of sf_conv_fwd_relu_mask;
  * byte for byte equal to the dense entry point.  The dense dispatch runs conv2 / conv3 on k_fwd_glds_zt / k_fwd_img only from
    n = 1214 / 512 on, the strided twins run at any n: the n = 258 launches are compared with the first 258 samples of the
    dense launch on the larger batch the 258 samples are the head of (a sample's result does not depend on the launch).
  * kernel names: the strided twins of the dense kernels, the dense names unchanged.
Row independence: sample i inside a strided launch of n = 256 (samples 100 .. 355 of the batch) equals sample i of a launch
over n = 1024, strided and — where the dense dispatch runs the twin's kernel at n = 1024 — dense.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_kernel_ledger import (BAND, CONV2, CONV3, DEFAULT_SWITCHES, F32, NATURE1, U8, Case, _conv64,  # noqa: E402
                                          _elementwise, _maxnorm, _rows, make_desc)

T, SLOT = 3, 1
LAYERS = {  # name -> (format, geometry, dense name, strided name, n of the shared batch)
    "conv1": (U8, NATURE1, "k_conv1_u8_bf16_w<false>", "k_conv1_u8_bf16_w_os<false>", 1024),
    "conv2": (F32, CONV2, "k_fwd_glds_zt<128, 64, 2, 2>", "k_fwd_glds_zt_os<128, 64, 2, 2>", 1620),
    "conv3": (F32, CONV3, "k_fwd_img<64, 9, 9, 3, 1, 2, 1, 7>", "k_fwd_img_os<64, 9, 9, 3, 1, 2, 1, 7>", 1024),
}
DENSE_N = {"conv1": 258, "conv2": 1620, "conv3": 514}  # smallest tested n at which the dense entry point runs the dense name
CASES = [("conv1", 258), ("conv1", 259), ("conv2", 258), ("conv2", 1620), ("conv3", 258), ("conv3", 514)]


@functools.lru_cache(maxsize=1)
def _batch(layer):
    fmt, geom, _, _, nmax = LAYERS[layer]
    return Case(fmt, geom, nmax, 0.0, False)


def _desc(layer):
    fmt, geom = LAYERS[layer][:2]
    return make_desc(fmt, geom, 0.0, 1)


def _rowlen(layer):
    d = _desc(layer)
    return d.OH * d.OW * d.Cout, d.OH * d.OW


@functools.lru_cache(maxsize=8)
def _dense(layer, n):
    """the existing dense entry point on the first n samples of the batch -> (out [n, OHOW * Cout], mask [n, OHOW] | None)"""
    c, d = _batch(layer), _desc(layer)
    L, P = _rowlen(layer)
    out = torch.full((n, L), float("nan"), device="cuda")
    mask = None
    if layer == "conv1":
        mask = torch.full((n, P), -1, dtype=torch.int32, device="cuda")
        lib.conv_fwd_relu_mask(c.x_dev, c.stride, None, 0, c.wk, c.b_dev, out, mask.view(-1), n, d)
    else:
        lib.conv_fwd_t(c.x_dev, c.stride, c.wk.t().contiguous(), c.b_dev, out, n, d)
    torch.cuda.synchronize()
    return out, mask


def _strided(layer, n, first=0):
    """the strided entry point on samples [first, first + n) of the batch into slot SLOT of a NaN-filled [n, T, .] buffer with a
    guard band behind it -> (buffer [n, T, L], band, mask buffer [n, T, P] | None, mask band | None)"""
    c, d = _batch(layer), _desc(layer)
    L, P = _rowlen(layer)
    flat = torch.full((n * T * L + BAND,), float("nan"), device="cuda")
    buf = flat[:n * T * L].view(n, T, L)
    x = c.x_dev[first:]
    mbuf = mflat = None
    if layer == "conv1":
        mflat = torch.full((n * T * P + BAND,), -1, dtype=torch.int32, device="cuda")
        mbuf = mflat[:n * T * P].view(n, T, P)
        assert lib.conv_fwd_os_supported("fwd", n, d, c.stride, T * L)
        lib.conv_fwd_relu_mask_os(x, c.stride, None, 0, c.wk, c.b_dev, buf[:, SLOT], T * L, mbuf[:, SLOT], T * P, n, d)
    else:
        assert lib.conv_fwd_os_supported("fwd_t", n, d, c.stride, T * L)
        lib.conv_fwd_t_os(x, c.stride, c.wk.t().contiguous(), c.b_dev, buf[:, SLOT], T * L, n, d)
    torch.cuda.synchronize()
    return buf, flat[n * T * L:], mbuf, None if mflat is None else mflat[n * T * P:]


def test_kernel_names():
    """the strided twins are named after the dense kernels, whose names (and sizes) are what they were"""
    from sample_factory_amd.algo.learning.rollout_reuse import twin_name
    for layer, (fmt, geom, dense, strided, _) in LAYERS.items():
        d = _desc(layer)
        assert strided == twin_name(dense)
        if not DEFAULT_SWITCHES:  # a dispatch switch is under test: it may move a launch to another kernel, which is its business
            continue
        for n in (4096, 32768):  # the rollout-size and the training-size launch of the headline workload
            assert lib.conv_kernel_name(0 if layer == "conv1" else 3, n, d) == dense
        for n in (258, 4096):
            assert lib.conv_kernel_name(6 if layer == "conv1" else 7, n, d) == strided
        assert lib.conv_kernel_name(0 if layer == "conv1" else 3, DENSE_N[layer], d) == dense


@pytest.mark.parametrize("layer,n", CASES, ids=[f"{l}-n{n}" for l, n in CASES])
def test_strided_equals_dense(layer, n):
    c, d = _batch(layer), _desc(layer)
    fmt, geom = LAYERS[layer][:2]
    Cin, H, W, Cout, K, S = geom
    L, P = _rowlen(layer)
    buf, band, mbuf, mband = _strided(layer, n)
    assert bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, 2]).all()), "a neighbouring slot was written"
    assert bool(torch.isnan(band).all()), "the forward wrote behind its buffer"
    got = buf[:, SLOT]
    assert bool(torch.isfinite(got).all()), "an element of the slot was not written"
    # float64, the ledger's bounds for a forward row
    x64 = c.x[:n]
    w, b = c.w.double(), c.b.double()
    ref = torch.relu(_rows(_conv64(x64, w, b, S)))
    mag = _rows(_conv64(x64.abs(), w.abs(), b.abs(), S))
    g64 = got.cpu().double().reshape(-1, Cout)
    rel = _maxnorm(g64, ref, 3e-5, "forward")
    ratio = _elementwise(g64, ref, mag, (3 if layer == "conv1" else 1) * K * K * Cin, "forward")
    print(f"out-stride {layer} n={n}: max|err|/max|ref| {rel:.3g} max(err/bound) {ratio:.3g}")
    # the dense entry point, byte for byte
    nd = max(n, DENSE_N[layer])
    dense, dmask = _dense(layer, nd)
    assert torch.equal(got.contiguous().view(torch.int32), dense[:n].view(torch.int32)), "strided and dense bytes differ"
    if layer == "conv1":
        assert bool((mbuf[:, 0] == -1).all()) and bool((mbuf[:, 2] == -1).all()) and bool((mband == -1).all())
        assert torch.equal(mbuf[:, SLOT], dmask[:n]), "the sign-bit words differ from sf_conv_fwd_relu_mask's"
        bits = (got.view(n, P, Cout) > 0).to(torch.int64) << torch.arange(Cout, device="cuda")
        assert torch.equal(bits.sum(-1).to(torch.int32), mbuf[:, SLOT]), "sign bits do not match the activation"


@pytest.mark.parametrize("layer", list(LAYERS))
def test_row_independence(layer):
    """a sample's bytes do not depend on the launch it is computed in, nor on its position inside it"""
    d = _desc(layer)
    first, n_small, n_big = 100, 256, 1024
    small = _strided(layer, n_small, first)[0][:, SLOT]
    big = _strided(layer, n_big)[0][:, SLOT]
    assert torch.equal(small.contiguous().view(torch.int32), big[first:first + n_small].contiguous().view(torch.int32))
    if lib.conv_kernel_name(0 if layer == "conv1" else 3, n_big, d) == LAYERS[layer][2]:
        dense, _ = _dense(layer, n_big)
        assert torch.equal(small.contiguous().view(torch.int32), dense[first:first + n_small].view(torch.int32))
    else:  # conv2: the dense launch at n = 1024 is another kernel; the dense kernel itself is compared at n = 1620
        dense, _ = _dense(layer, LAYERS[layer][4])
        assert torch.equal(small.contiguous().view(torch.int32), dense[first:first + n_small].view(torch.int32))
