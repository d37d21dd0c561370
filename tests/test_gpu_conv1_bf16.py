"""--encoder_conv1_bf16: the raw-frame conv layer on bf16 MFMA (csrc/sf_conv1_bf16.hip) against float64 torch on operands
rounded like the kernel's: x' formed in float32 with the contract's separate operations, then rounded once to bf16."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_resnet import ACTS, _nchw, _nhwc  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG  # noqa: E402

# kind -> (u8 frames, sub_mean, inv_scale, tables)
KINDS = {"u8": (True, 0.0, 1.0, False), "u8_norm": (True, 128.0, float(np.float32(1.0 / 255.0)), True),
         "f32": (False, 0.25, 2.0, False), "f32_norm": (False, 0.25, 2.0, True)}


def _bf(t):
    return t.float().bfloat16().double()


def _w_frame(w):  # OIHW -> [(c*KH + kh)*KW + kw, Cout]
    return w.reshape(w.shape[0], -1).t().contiguous()


def _desc(cin, h, w, cout, kind, act=1, **kw):
    u8, sub, inv, _ = KINDS[kind]
    f = dict(Cin=cin, H=h, W=w, Cout=cout, KH=8, KW=8, stride=4, OH=(h - 8) // 4 + 1, OW=(w - 8) // 4 + 1, in_u8=1 if u8 else 2,
             relu=act, traj_T=0, sub_mean=sub, inv_scale=inv)
    f.update(kw)
    return lib.sf_conv_desc(**f)


def x_prime(frames, sub, inv, mu=None, rstd=None):
    """the contract's input value: float32 on the CPU, one rounded operation after the other"""
    v = frames.cpu().float()
    v = v - sub
    v = v * inv
    if mu is not None:
        v = v - mu.cpu().view(v.shape[1:])
        v = v * rstd.cpu().view(v.shape[1:])
        v = v.clamp(-5.0, 5.0)
    return v


def _frames(kind, shape, g):
    if KINDS[kind][0]:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.rand(shape, generator=g)


def _tables(kind, elems, g):  # |mu * rstd| reaches a few units: part of every frame is clamped
    if not KINDS[kind][3]:
        return None, None
    return torch.rand(elems, generator=g) - 0.5, torch.rand(elems, generator=g) * 12.0 + 0.1


@functools.lru_cache(maxsize=None)
def _case(cin, h, w, cout, n, kind):
    """frames, N(0, 1/(64 Cin)) weights drawn in float32, N(0, 1) dout; float64 references of the activation-free passes.
    Un-scaled u8 pixels (kind "u8": x' up to 255, rms 147) get dout * 2^-7, an exact scaling: WG's atol of 5e-4 was set for
    products of unit variance, and with N(0, 1) dout the partial sums here reach 1e4, where one fp32 ulp is 1e-3 — no fp32
    accumulator meets the bound there (measured with N(0, 1) dout at 3x72x128: 2 of 6144 elements off by 1.4e-3 at most)."""
    g = torch.Generator().manual_seed(cin * 1000 + h * 10 + w + n)
    _, sub, inv, _ = KINDS[kind]
    x = _frames(kind, (n, cin, h, w), g)
    mu, rstd = _tables(kind, cin * h * w, g)
    wt = torch.randn(cout, cin, 8, 8, generator=g).div((64 * cin) ** 0.5).double()
    b = torch.randn(cout, generator=g).double()
    gy = torch.randn(n, cout, (h - 8) // 4 + 1, (w - 8) // 4 + 1, generator=g).double()
    if kind == "u8":
        gy = gy / 128
    xb = _bf(x_prime(x, sub, inv, mu, rstd))
    if mu is not None:
        assert (xb.abs() == 5).any() and (xb.abs() < 5).any()
    ref = dict(pre=F.conv2d(xb, _bf(wt), b, stride=4),
               gw=_w_frame(torch.nn.grad.conv2d_weight(xb, wt.shape, _bf(gy), stride=4)), gb=_bf(gy).sum((0, 2, 3)))
    dev = dict(x=x.cuda(), mu=None if mu is None else mu.cuda(), rstd=None if rstd is None else rstd.cuda(),
               w=_w_frame(wt).float().cuda(), b=b.float().cuda(), gy=_nhwc(gy).float().cuda())
    return dev, ref


def _guarded(*shape):
    """a tensor of `shape` with guard values behind it"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 64,), 7.0, device="cuda")
    return buf[:numel].view(*shape), buf[numel:]


def _fwd(t, d, n, x=None, stride=None, index=None, offset=0):
    y, guard = _guarded(n, d.OH, d.OW, d.Cout)
    x = t["x"] if x is None else x
    lib.conv1_fwd_bf16(x, stride or d.Cin * d.H * d.W, index, offset, t["mu"], t["rstd"], t["w"], t["b"], y, n, d)
    assert (guard == 7.0).all()
    return y


def _wgrad(t, d, n, x=None, stride=None, index=None, offset=0):
    (gw, g0), (gb, g1) = _guarded(d.Cin * 64, d.Cout), _guarded(d.Cout)
    ws = torch.empty(lib.conv1_wgrad_bf16_workspace(n, d), dtype=torch.uint8, device="cuda")
    x = t["x"] if x is None else x
    lib.conv1_wgrad_bf16(x, stride or d.Cin * d.H * d.W, index, offset, t["mu"], t["rstd"], t["gy"], gw, gb, n, d, ws)
    assert (g0 == 7.0).all() and (g1 == 7.0).all()
    return gw, gb


# (Cin, H, W, Cout, n): one output pixel; several samples a band; W % 4 != 0 with an uncovered row and column (scalar loader);
# the Nature layer at both widths; more than one band; weights of 12 and of 16 channels (the latter with the 128 KiB LDS
# budget); several weight-gradient parts
SHAPES = [(1, 8, 8, 16, 5), (4, 36, 36, 32, 3), (3, 27, 41, 16, 2), (4, 84, 84, 32, 2), (4, 84, 84, 16, 2), (3, 72, 128, 32, 2),
          (12, 20, 20, 32, 2), (16, 12, 12, 32, 2), (4, 36, 36, 32, 300)]
CASES = [s + (k, a) for s in SHAPES[:2] for k in KINDS for a in (0, 2, 3)] + [s + (k, 1) for s in SHAPES for k in KINDS]


@pytest.mark.parametrize("cin,h,w,cout,n,kind,act", CASES)
def test_conv1_bf16_fwd_wgrad(cin, h, w, cout, n, kind, act):
    t, ref = _case(cin, h, w, cout, n, kind)
    d = _desc(cin, h, w, cout, kind, act)
    assert lib.conv1_bf16_supported("fwd", n, d) and lib.conv1_bf16_supported("wgrad", n, d)
    np.testing.assert_allclose(_nchw(_fwd(t, d, n)).cpu().double(), ACTS[act](ref["pre"]), **FWD)
    gw, gb = _wgrad(t, d, n)
    np.testing.assert_allclose(gw.cpu().double(), ref["gw"], **WG)
    np.testing.assert_allclose(gb.cpu().double(), ref["gb"], **WG)


@pytest.mark.parametrize("mode,kind", [("index", "u8_norm"), ("traj", "u8_norm"), ("stride", "u8_norm"), ("byte_off", "u8_norm"),
                                       ("index", "f32_norm"), ("traj", "f32_norm"), ("stride", "f32_norm")])
def test_conv1_bf16_addressing_equals_the_dense_launch(mode, kind):
    cin, h, w, cout = 4, 36, 36, 32
    t, _ = _case(cin, h, w, cout, 3, kind)
    elems = cin * h * w
    store = _frames(kind, (12, elems), torch.Generator().manual_seed(5)).cuda()
    index, offset, stride, tT = None, 0, elems, 0
    if mode == "index":
        index = torch.tensor([5, 0, 9, 3, 3, 11], dtype=torch.int32, device="cuda")
        src, rows = store, index.long()
    elif mode == "traj":  # a slab [3, T + 1]: logical sample e*T + t is slab row e*(T + 1) + t
        tT, offset = 3, 2
        src, rows = store, torch.tensor([dd + dd // 3 for dd in range(2, 7)], device="cuda")
    elif mode == "stride":
        stride = elems + 8
        src, rows = torch.cat([store, store[:, :8]], 1).contiguous(), torch.arange(12, device="cuda")
    else:  # u8 frames one byte off the 4-byte grid
        src, rows = torch.cat([store.view(-1)[:1], store.view(-1)])[1:], torch.arange(12, device="cuda")
        assert src.data_ptr() % 4 == 1
    n = rows.numel()
    dense = store[rows].contiguous()
    t = dict(t, gy=torch.randn(n, 8, 8, cout, generator=torch.Generator().manual_seed(6)).cuda())
    d, dt = _desc(cin, h, w, cout, kind), _desc(cin, h, w, cout, kind, traj_T=tT)
    assert torch.equal(_fwd(t, dt, n, src, stride, index, offset), _fwd(t, d, n, dense))
    (gw0, gb0), (gw1, gb1) = _wgrad(t, dt, n, src, stride, index, offset), _wgrad(t, d, n, dense)
    assert torch.equal(gw0, gw1) and torch.equal(gb0, gb1)


@pytest.mark.parametrize("kind", ["u8_norm", "f32"])
def test_conv1_bf16_forward_does_not_depend_on_the_batch(kind):
    t, _ = _case(4, 36, 36, 32, 3, kind)
    d = _desc(4, 36, 36, 32, kind, 3)
    full = _fwd(t, d, 3)
    for i in range(3):
        assert torch.equal(_fwd(t, d, 1, t["x"][i:i + 1])[0], full[i]), i


def test_conv1_bf16_wgrad_is_deterministic():
    t, _ = _case(4, 36, 36, 32, 300, "u8_norm")
    d = _desc(4, 36, 36, 32, "u8_norm")
    assert lib.conv1_wgrad_bf16_workspace(300, d) > lib.conv1_wgrad_bf16_workspace(2, d)  # several parts
    (gw0, gb0), (gw1, gb1) = _wgrad(t, d, 300), _wgrad(t, d, 300)
    assert torch.equal(gw0, gw1) and torch.equal(gb0, gb1)


@pytest.mark.parametrize("what", ["in_u8", "kernel", "cout", "cin", "one_table", "workspace"])
def test_conv1_bf16_refuses_what_it_does_not_serve(what):
    cin, cout = (17 if what == "cin" else 4), (64 if what == "cout" else 32)
    kw = dict(in_u8=0) if what == "in_u8" else dict(KH=4, KW=4, stride=2, OH=17, OW=17) if what == "kernel" else {}
    d = _desc(cin, 36, 36, cout, "u8_norm", **kw)
    x = torch.zeros(2, cin, 36, 36, device="cuda", dtype=torch.float32 if d.in_u8 == 0 else torch.uint8)
    mu = rstd = torch.ones(cin * 36 * 36, device="cuda")
    if what == "one_table":
        rstd = None
    w, b = torch.zeros(d.KH * d.KW * cin, cout, device="cuda"), torch.zeros(cout, device="cuda")
    y = torch.full((2, d.OH, d.OW, cout), 7.0, device="cuda")
    gw, gb, ws = torch.full_like(w, 7.0), torch.full_like(b, 7.0), torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    if what == "workspace":
        ws = ws[:lib.conv1_wgrad_bf16_workspace(2, d) - 16]
    served = what in ("one_table", "workspace")
    if not served:
        assert not lib.conv1_bf16_supported("fwd", 2, d) and not lib.conv1_bf16_supported("wgrad", 2, d)
        assert lib.conv1_wgrad_bf16_workspace(2, d) == 0
    code = r"\(-1\)" if served else r"\(-3\)"  # SF_ERR_ARG / SF_ERR_UNSUPPORTED
    if what != "workspace":
        with pytest.raises(lib.SfHipError, match=code):
            lib.conv1_fwd_bf16(x, x[0].numel(), None, 0, mu, rstd, w, b, y, 2, d)
    with pytest.raises(lib.SfHipError, match=code):
        lib.conv1_wgrad_bf16(x, x[0].numel(), None, 0, mu, rstd, y, gw, gb, 2, d, ws)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (gw == 7.0).all() and (gb == 7.0).all()  # nothing was launched
