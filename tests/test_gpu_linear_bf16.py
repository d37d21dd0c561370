"""--mlp_bf16: the fully connected layers on bf16 MFMA (csrc/sf_linear_bf16.hip) against float64 torch on operands rounded like
the kernel's; guard elements, row independence, determinism, the refusals."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_conv_bf16 import ACT_BWD, _bf  # noqa: E402
from tests.test_gpu_resnet import ACTS  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG  # noqa: E402

GUARD = 64


@functools.lru_cache(maxsize=None)
def _layer(n, K, N):
    """N(0, 1) rows, N(0, 1/K) weights, drawn in float32; float64 references of the activation-free passes on rounded operands"""
    g = torch.Generator().manual_seed(n * 7 + K * 3 + N)
    x, w = torch.randn(n, K, generator=g), torch.randn(K, N, generator=g) / K ** 0.5
    b, gy = torch.randn(N, generator=g), torch.randn(n, N, generator=g)
    ref = dict(x=x.double(), pre=_bf(x) @ _bf(w) + b.double(), gx=_bf(gy) @ _bf(w).t(), gw=_bf(x).t() @ _bf(gy), gb=_bf(gy).sum(0))
    return dict(x=x.cuda(), w=w.cuda(), b=b.cuda(), gy=gy.cuda()), ref


def _guarded(*shape):
    """a tensor of `shape` with GUARD elements of 7.0 behind it"""
    flat = torch.full((int(np.prod(shape)) + GUARD,), 7.0, device="cuda")
    return flat[:-GUARD].view(*shape), flat[-GUARD:]


def _wgrad(t, n, K, N):
    (gw, g0), (gb, g1) = _guarded(K, N), _guarded(N)
    ws = torch.empty(lib.linear_wgrad_bf16_workspace(n, K, N), dtype=torch.uint8, device="cuda")
    lib.linear_wgrad_bf16(t["x"], t["gy"], gw, gb, n, K, N, ws)
    assert (g0 == 7.0).all() and (g1 == 7.0).all()
    return gw, gb


def _two_part_rows(K, N):
    """the smallest row count whose weight gradient is cut into more than one part (a part reduces chunks of 64 rows,
    include/sf_hip.h), plus one; read off the workspace query"""
    one = lib.linear_wgrad_bf16_workspace(1, K, N)
    assert lib.linear_wgrad_bf16_workspace(64, K, N) == one and lib.linear_wgrad_bf16_workspace(65, K, N) == 2 * one
    return 66


SHAPES = [(1, 8, 8), (5, 40, 72), (5, 3136, 512), (300, 64, 64), (300, 512, 256), ("P", 256, 64)]
CASES = [s + (a,) for s in SHAPES[:2] for a in (0, 2, 3)] + [s + (1,) for s in SHAPES]


@pytest.mark.parametrize("n,K,N,act", CASES)
def test_linear_bf16_fwd_dgrad_wgrad(n, K, N, act):
    if n == "P":
        n = _two_part_rows(K, N)
        if n > 20000:
            pytest.skip(f"two parts need {n} rows")
    t, ref = _layer(n, K, N)
    y, guard = _guarded(n, N)
    lib.linear_fwd_bf16(t["x"], t["w"], t["b"], y, n, K, N, act)
    np.testing.assert_allclose(y.cpu().double(), ACTS[act](ref["pre"]), **FWD)
    assert (guard == 7.0).all()
    gx = torch.full((n, K), float("nan"), device="cuda")
    lib.linear_dgrad_bf16(t["gy"], t["w"], t["x"] if act else None, gx, n, K, N, act)  # in_act: the stored tensor itself
    np.testing.assert_allclose(gx.cpu().double(), ref["gx"] * ACT_BWD[act](ref["x"]), **FWD)
    gw, gb = _wgrad(t, n, K, N)
    np.testing.assert_allclose(gw.cpu().double(), ref["gw"], **WG)
    np.testing.assert_allclose(gb.cpu().double(), ref["gb"], **WG)


def test_linear_bf16_forward_row_does_not_depend_on_the_launch():
    n, K, N = 5, 3136, 512
    t, _ = _layer(n, K, N)
    full, one = torch.empty(n, N, device="cuda"), torch.empty(1, N, device="cuda")
    lib.linear_fwd_bf16(t["x"], t["w"], t["b"], full, n, K, N, 1)
    for i in range(n):
        lib.linear_fwd_bf16(t["x"][i:i + 1], t["w"], t["b"], one, 1, K, N, 1)
        assert torch.equal(one[0], full[i]), i


def test_linear_bf16_wgrad_is_deterministic():
    t, _ = _layer(300, 512, 256)
    (gw0, gb0), (gw1, gb1) = _wgrad(t, 300, 512, 256), _wgrad(t, 300, 512, 256)
    assert torch.equal(gw0, gw1) and torch.equal(gb0, gb1)


@pytest.mark.parametrize("n,K,N", [(2, 12, 64), (2, 64, 12), (2, 4, 8)])
def test_linear_bf16_refuses_what_it_does_not_serve(n, K, N):
    assert not any(lib.linear_bf16_supported(op, n, K, N) for op in ("fwd", "dgrad", "wgrad"))
    assert lib.linear_wgrad_bf16_workspace(n, K, N) == 0
    x, w, b = torch.zeros(n, K, device="cuda"), torch.zeros(K, N, device="cuda"), torch.zeros(N, device="cuda")
    y, gx, gw, gb = (torch.full(s, 7.0, device="cuda") for s in ((n, N), (n, K), (K, N), (N,)))
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.SfHipError, match=r"\(-3\)"):  # SF_ERR_UNSUPPORTED
        lib.linear_fwd_bf16(x, w, b, y, n, K, N, 1)
    with pytest.raises(lib.SfHipError, match=r"\(-3\)"):
        lib.linear_dgrad_bf16(y, w, x, gx, n, K, N, 1)
    with pytest.raises(lib.SfHipError, match=r"\(-3\)"):
        lib.linear_wgrad_bf16(x, y, gw, gb, n, K, N, ws)
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in (y, gx, gw, gb))  # nothing was launched


def test_linear_bf16_wgrad_refuses_a_short_workspace():
    t, _ = _layer(300, 64, 64)
    gw, gb = torch.full((64, 64), 7.0, device="cuda"), torch.full((64,), 7.0, device="cuda")
    ws = torch.empty(lib.linear_wgrad_bf16_workspace(300, 64, 64) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.SfHipError, match="workspace"):
        lib.linear_wgrad_bf16(t["x"], t["gy"], gw, gb, 300, 64, 64, ws)
    torch.cuda.synchronize()
    assert (gw == 7.0).all() and (gb == 7.0).all()
