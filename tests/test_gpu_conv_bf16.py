"""--encoder_conv_bf16: the inner convs of convnet_simple / convnet_atari on bf16 MFMA (csrc/sf_conv_bf16.hip) against float64
torch on operands rounded like the kernel's; batch independence, determinism, the unmasked data gradient, the refusals."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_resnet import ACTS, _nchw, _nhwc, _w_native  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG  # noqa: E402

# derivative of the activation through its stored output y (sf_conv_dgrad's contract)
ACT_BWD = {0: lambda y: torch.ones_like(y), 1: lambda y: (y > 0).double(), 2: lambda y: 1 - y * y,
           3: lambda y: torch.where(y > 0, torch.ones_like(y), y + 1)}


def _bf(t):
    return t.float().bfloat16().double()


def _desc(cin, cout, k, s, h, w, act=0, **kw):
    f = dict(Cin=cin, H=h, W=w, Cout=cout, KH=k, KW=k, stride=s, OH=(h - k) // s + 1, OW=(w - k) // s + 1, in_u8=0, relu=act,
             traj_T=0, sub_mean=0.0, inv_scale=1.0)
    f.update(kw)
    return lib.sf_conv_desc(**f)


@functools.lru_cache(maxsize=None)
def _layer(cin, cout, k, s, h, w, n):
    """N(0,1) data, N(0, 1/(K*K*Cin)) weights, drawn in float32 so that the device and the reference round the same numbers;
    float64 references of the activation-free passes on rounded operands; the device operands"""
    g = torch.Generator().manual_seed(cin * 1000 + h * 10 + w + n)
    rnd = lambda *sh: torch.randn(*sh, generator=g).double()  # noqa: E731
    x, wt, b = rnd(n, cin, h, w), rnd(cout, cin, k, k).div((k * k * cin) ** 0.5).float().double(), rnd(cout)
    gy = rnd(n, cout, (h - k) // s + 1, (w - k) // s + 1)
    ref = dict(x=x, pre=F.conv2d(_bf(x), _bf(wt), b, stride=s),
               gx=torch.nn.grad.conv2d_input(x.shape, _bf(wt), _bf(gy), stride=s),
               gw=_w_native(torch.nn.grad.conv2d_weight(_bf(x), wt.shape, _bf(gy), stride=s)), gb=_bf(gy).sum((0, 2, 3)))
    dev = dict(x=_nhwc(x).float().cuda(), w=_w_native(wt).float().cuda(), b=b.float().cuda(), gy=_nhwc(gy).float().cuda())
    return dev, ref


def _wgrad(t, n, d):
    gw, gb = torch.empty(d.KH * d.KW * d.Cin, d.Cout, device="cuda"), torch.empty(d.Cout, device="cuda")
    ws = torch.empty(lib.conv_wgrad_bf16_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.conv_wgrad_bf16(t["x"], d.H * d.W * d.Cin, None, 0, t["gy"], gw, gb, n, d, ws)
    return gw, gb


GEOMS = [(32, 64, 4, 2, 4, 4, 5), (32, 64, 4, 2, 20, 20, 3), (64, 64, 3, 1, 9, 9, 5), (64, 128, 3, 2, 9, 9, 2),
         (32, 64, 4, 2, 17, 31, 2), (64, 128, 3, 2, 7, 14, 2), (32, 64, 4, 2, 31, 39, 2), (32, 64, 4, 2, 20, 20, 300)]
SMALL = [(32, 64, 4, 2, 4, 4, 5), (64, 128, 3, 2, 9, 9, 2)]  # the two smallest: every activation kind
CASES = [c + (a,) for c in SMALL for a in (0, 2, 3)] + [c + (1,) for c in GEOMS]


@pytest.mark.parametrize("cin,cout,k,s,h,w,n,act", CASES)
def test_conv_bf16_fwd_dgrad_wgrad(cin, cout, k, s, h, w, n, act):
    t, ref = _layer(cin, cout, k, s, h, w, n)
    d = _desc(cin, cout, k, s, h, w, act)
    y = torch.empty(n, d.OH, d.OW, cout, device="cuda")
    lib.conv_fwd_bf16(t["x"], h * w * cin, None, 0, t["w"], t["b"], y, n, d)
    np.testing.assert_allclose(_nchw(y).cpu().double(), ACTS[act](ref["pre"]), **FWD)
    gx = torch.full((n, h, w, cin), float("nan"), device="cuda")
    lib.conv_dgrad_bf16(t["gy"], t["w"], t["x"] if act else None, gx, n, d)  # in_act: the stored tensor itself
    np.testing.assert_allclose(_nchw(gx).cpu().double(), ref["gx"] * ACT_BWD[act](ref["x"]), **FWD)
    rows, cols = (d.OH - 1) * s + k, (d.OW - 1) * s + k  # input rows and columns a window covers
    assert (gx[:, rows:] == 0).all() and (gx[:, :, cols:] == 0).all()
    gw, gb = _wgrad(t, n, d)
    np.testing.assert_allclose(gw.cpu().double(), ref["gw"], **WG)
    np.testing.assert_allclose(gb.cpu().double(), ref["gb"], **WG)


@pytest.mark.parametrize("cin,cout,k,s,h,w", [(32, 64, 4, 2, 20, 20), (64, 64, 3, 1, 9, 9)])
def test_conv_bf16_forward_does_not_depend_on_the_batch(cin, cout, k, s, h, w):
    t, _ = _layer(cin, cout, k, s, h, w, 5)
    d = _desc(cin, cout, k, s, h, w, 3)
    full, one = torch.empty(5, d.OH, d.OW, cout, device="cuda"), torch.empty(1, d.OH, d.OW, cout, device="cuda")
    lib.conv_fwd_bf16(t["x"], h * w * cin, None, 0, t["w"], t["b"], full, 5, d)
    for i in range(5):
        lib.conv_fwd_bf16(t["x"][i:i + 1], h * w * cin, None, 0, t["w"], t["b"], one, 1, d)
        assert torch.equal(one[0], full[i]), i


def test_conv_bf16_wgrad_is_deterministic():
    t, _ = _layer(32, 64, 4, 2, 20, 20, 300)
    d = _desc(32, 64, 4, 2, 20, 20, 1)
    (gw0, gb0), (gw1, gb1) = _wgrad(t, 300, d), _wgrad(t, 300, d)
    assert torch.equal(gw0, gw1) and torch.equal(gb0, gb1)


def test_conv_bf16_dgrad_without_in_act_is_unmasked():
    t, ref = _layer(32, 64, 4, 2, 20, 20, 3)
    gx = torch.empty(3, 20, 20, 32, device="cuda")
    lib.conv_dgrad_bf16(t["gy"], t["w"], None, gx, 3, _desc(32, 64, 4, 2, 20, 20, 0))
    np.testing.assert_allclose(_nchw(gx).cpu().double(), ref["gx"], **FWD)


@pytest.mark.parametrize("cin,cout,k,s,kw", [(16, 32, 4, 2, {}), (32, 64, 5, 1, {}), (32, 64, 4, 2, dict(in_u8=1)),
                                            (32, 64, 4, 2, dict(index=True))])
def test_conv_bf16_refuses_what_it_does_not_serve(cin, cout, k, s, kw):
    index = torch.zeros(2, dtype=torch.int32, device="cuda") if kw.pop("index", False) else None
    d = _desc(cin, cout, k, s, 20, 20, 1, **kw)
    x = torch.zeros(2, 20, 20, cin, device="cuda", dtype=torch.uint8 if d.in_u8 else torch.float32)
    w, b = torch.zeros(k * k * cin, cout, device="cuda"), torch.zeros(cout, device="cuda")
    y = torch.full((2, d.OH, d.OW, cout), 7.0, device="cuda")
    gw, ws = torch.full_like(w, 7.0), torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    if index is None:
        assert not any(lib.conv_bf16_supported(op, 2, d) for op in ("fwd", "dgrad", "wgrad"))
        assert lib.conv_wgrad_bf16_workspace(2, d) == 0
    with pytest.raises(lib.SfHipError, match=r"\(-3\)"):  # SF_ERR_UNSUPPORTED
        lib.conv_fwd_bf16(x, x[0].numel(), index, 0, w, b, y, 2, d)
    with pytest.raises(lib.SfHipError, match=r"\(-3\)"):
        lib.conv_wgrad_bf16(x, x[0].numel(), index, 0, y, gw, b, 2, d, ws)
    if index is None:
        with pytest.raises(lib.SfHipError, match=r"\(-3\)"):
            lib.conv_dgrad_bf16(y, w, None, torch.empty(2, 20, 20, cin, device="cuda"), 2, d)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (gw == 7.0).all()  # nothing was launched
