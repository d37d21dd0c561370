"""One row per network kernel the dispatcher can pick (sf_conv_fwd, sf_conv_fwd_t, sf_conv_wgrad, sf_conv_dgrad,
sf_conv_fwd_norm, sf_conv_wgrad_norm: about 70 compiled instantiations chosen by geometry, sample count, input format,
occupancy and row thresholds).  Every row pins the kernel by the name sf_conv_kernel_name reports, then checks the
operation against float64 on the CPU (max-norm AND an element-wise a-priori bound), guard bands around every output and
bit reproducibility.  The roster test sweeps a grid of launches through sf_conv_kernel_name and fails on a selectable
kernel that has neither a row nor a written reason; the next test repeats both under the A/B switch groups of
tests/test_gpu_switches.py, and the last checks that the reported name follows a switch the way the launch does.
DESIGN.md 4.1 holds the measured figures."""
import functools
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U8, F32F = lib.IN_F32_NHWC, lib.IN_U8_FRAME, lib.IN_F32_FRAME
INV = {F32: 1.0, U8: float(np.float32(1.0 / 255.0)), F32F: 0.5}  # sf_conv_desc.inv_scale per input format
FWD, WGRAD, DGRAD, FWD_T, FWD_NORM, WGRAD_NORM = range(6)        # op, as sf_conv_kernel_name numbers them
# switches that do not touch the dispatch; any other SF_* variable in the environment suspends the name asserts
NOT_DISPATCH = {"SF_HIP_LIB", "SF_FUZZ_SEED", "SF_FUZZ_CASES", "SF_LAUNCH_PROGRAMS"}
DEFAULT_SWITCHES = not any(k.startswith("SF_") and k not in NOT_DISPATCH for k in os.environ)

Row = namedtuple("Row", "id op fmt geom n mean act name")  # geom = (Cin, H, W, Cout, K, S); act: 0 none, 1 ReLU


def _r(op, fmt, geom, n, mean, act, name):
    tag = {F32: "f32", U8: "u8", F32F: "f32f"}[fmt]
    return Row(f"op{op}-{tag}-{'x'.join(map(str, geom))}-n{n}-m{mean:g}", op, fmt, geom, n, mean, act, name)


NATURE1, CONV2, CONV3 = (4, 84, 84, 32, 8, 4), (32, 20, 20, 64, 4, 2), (64, 9, 9, 64, 3, 1)

# The expected names are those of the default dispatch on the MI355X (256 CUs; the occupancy-dependent choices of
# plan_fwd_t / fwd_tail_split as the device reports them).  Shapes: the smallest n at which the kernel is still selected,
# n * OH * OW not a multiple of the row tile, Cout / K off the column tile / 32 where the kernel's contract allows it.
LEDGER = [
    # ---- sf_conv_fwd: register-staged k_conv_fwd<BM, BN, WM, WN, MODE> (MODE 0 f32 NHWC, 1 u8, 2 scalar, 3 f32 frames)
    _r(FWD, F32, (4, 9, 9, 8, 3, 1), 3, 0.0, 1, "k_conv_fwd<128, 32, 4, 1, 0>"),
    _r(FWD, U8, (4, 36, 36, 32, 8, 4), 37, 3.0, 1, "k_conv_fwd<128, 32, 4, 1, 1>"),
    _r(FWD, F32, (3, 9, 9, 5, 3, 1), 3, 0.0, 0, "k_conv_fwd<128, 32, 4, 1, 2>"),
    _r(FWD, F32F, (3, 36, 36, 16, 8, 4), 5, 1.5, 1, "k_conv_fwd<128, 32, 4, 1, 3>"),
    _r(FWD, F32, (4, 9, 9, 8, 3, 1), 10700, 0.0, 1, "k_conv_fwd<256, 32, 4, 1, 0>"),       # Mtot 524300 >= 256 * 2048
    _r(FWD, U8, (3, 36, 36, 16, 8, 4), 8193, 3.0, 1, "k_conv_fwd<256, 32, 4, 1, 1>"),
    _r(FWD, F32, (3, 9, 9, 5, 3, 1), 10700, 0.0, 1, "k_conv_fwd<256, 32, 4, 1, 2>"),
    _r(FWD, F32F, (3, 36, 36, 16, 8, 4), 8193, 0.0, 0, "k_conv_fwd<256, 32, 4, 1, 3>"),
    _r(FWD, F32, (16, 11, 13, 48, 3, 2), 37, 0.0, 1, "k_conv_fwd<128, 64, 2, 2, 0>"),
    _r(FWD, U8, (3, 36, 36, 48, 8, 4), 3, 3.0, 1, "k_conv_fwd<128, 64, 2, 2, 1>"),
    _r(FWD, F32, (3, 9, 9, 50, 3, 1), 3, 0.0, 1, "k_conv_fwd<128, 64, 2, 2, 2>"),
    _r(FWD, F32F, (3, 36, 36, 48, 8, 4), 3, 1.5, 0, "k_conv_fwd<128, 64, 2, 2, 3>"),
    _r(FWD, F32, (8, 6, 6, 128, 3, 1), 3, 0.0, 1, "k_conv_fwd<64, 64, 2, 2, 0>"),          # Mtot 48 <= 64
    _r(FWD, U8, (4, 36, 36, 48, 8, 4), 1, 0.0, 1, "k_conv_fwd<64, 64, 2, 2, 1>"),
    _r(FWD, F32, (3, 9, 9, 50, 3, 1), 1, 0.0, 0, "k_conv_fwd<64, 64, 2, 2, 2>"),
    _r(FWD, F32F, (4, 36, 36, 48, 8, 4), 1, 3.0, 1, "k_conv_fwd<64, 64, 2, 2, 3>"),
    _r(FWD, F32, (3136, 1, 1, 136, 1, 1), 130, 0.0, 1, "k_conv_fwd<128, 64, 2, 2, 0>"),    # split along K + k_splitk_finish
    # ---- sf_conv_fwd: Nature conv1 on raw u8 frames, n >= 256 (strip-image kernels)
    _r(FWD, U8, NATURE1, 257, 3.0, 1, "k_conv1_u8_bf16_w<true>"),
    _r(FWD, U8, NATURE1, 257, 0.0, 0, "k_conv1_u8_bf16_w<false>"),
    _r(FWD, U8, (4, 84, 84, 24, 8, 4), 257, 3.0, 1, "k_conv1_u8_bf16<true>"),
    _r(FWD, U8, (4, 84, 84, 24, 8, 4), 257, 0.0, 1, "k_conv1_u8_bf16<false>"),
    _r(FWD, U8, (4, 84, 84, 24, 8, 4), 257, 1.5, 1, "k_conv_u8_img<2, 4, 5, 16, true>"),   # non-integer mean: f32 image
    # ---- sf_conv_fwd_t: narrow heads, LDS-image conv3, LDS-DMA tiles
    _r(FWD_T, F32, (48, 1, 1, 7, 1, 1), 37, 0.0, 0, "k_linear_narrow<1>"),
    _r(FWD_T, F32, (48, 1, 1, 20, 1, 1), 37, 0.0, 1, "k_linear_narrow<2>"),
    _r(FWD_T, F32, CONV3, 513, 0.0, 1, "k_fwd_img<64, 9, 9, 3, 1, 2, 1, 7>"),
    _r(FWD_T, F32, CONV2, 513, 0.0, 1, "k_fwd_glds_z<64, 64, 2, 2>"),                      # small inference launch
    _r(FWD_T, F32, (3136, 1, 1, 136, 1, 1), 2049, 0.0, 1, "k_fwd_glds_z<64, 64, 2, 2>"),   # 64x64 tiles split along K
    _r(FWD_T, F32, (32, 11, 13, 96, 3, 2), 1641, 0.0, 1, "k_fwd_glds_z<128, 64, 2, 2>"),   # two column tiles
    _r(FWD_T, F32, (32, 12, 14, 64, 3, 2), 3277, 0.0, 1, "k_fwd_glds_zt<128, 64, 2, 2>"),  # one column tile: tail split
    _r(FWD_T, F32, (32, 1, 1, 160, 1, 1), 32769, 0.0, 1, "k_fwd_glds_z<128, 128, 2, 2>"),  # by the device's occupancy
    _r(FWD_T, F32, (32, 11, 13, 136, 3, 2), 2049, 0.0, 0, "k_fwd_glds_z<128, 128, 2, 2>"),  # spatial taps, ragged columns
    # ---- sf_conv_wgrad
    _r(WGRAD, F32, (4, 9, 9, 8, 3, 1), 3, 0.0, 0, "k_conv_wgrad<32, 4, 1, 0>"),
    _r(WGRAD, U8, (4, 36, 36, 32, 8, 4), 37, 3.0, 0, "k_conv_wgrad<32, 4, 1, 1>"),
    _r(WGRAD, F32, (3, 9, 9, 5, 3, 1), 3, 0.0, 0, "k_conv_wgrad<32, 4, 1, 2>"),
    _r(WGRAD, F32F, (3, 36, 36, 16, 8, 4), 5, 1.5, 0, "k_conv_wgrad<32, 4, 1, 3>"),
    _r(WGRAD, F32, (16, 11, 13, 48, 3, 2), 37, 0.0, 0, "k_conv_wgrad<64, 2, 2, 0>"),
    _r(WGRAD, U8, (3, 36, 36, 48, 8, 4), 3, 3.0, 0, "k_conv_wgrad<64, 2, 2, 1>"),
    _r(WGRAD, F32, (3, 9, 9, 48, 3, 1), 3, 0.0, 0, "k_conv_wgrad<64, 2, 2, 2>"),
    _r(WGRAD, F32F, (3, 36, 36, 48, 8, 4), 3, 1.5, 0, "k_conv_wgrad<64, 2, 2, 3>"),
    _r(WGRAD, F32, (27, 1, 1, 17, 1, 1), 1001, 0.0, 0, "k_linear_wgrad_small"),
    _r(WGRAD, U8, NATURE1, 257, 3.0, 0, "k_conv1_wgrad_bf16<true>"),
    _r(WGRAD, U8, NATURE1, 257, 0.0, 0, "k_conv1_wgrad_bf16<false>"),
    _r(WGRAD, U8, NATURE1, 257, 1.5, 0, "k_conv1_wgrad_img<2, 4, true>"),
    _r(WGRAD, F32, CONV3, 513, 0.0, 0, "k_wgrad_img<64, 9, 9, 3, 1, 1>"),
    _r(WGRAD, F32, CONV2, 513, 0.0, 0, "k_wgrad_img<32, 20, 20, 4, 2, 2>"),
    _r(WGRAD, F32, (4, 20, 20, 128, 4, 2), 810, 0.0, 0, "k_wgrad_glds<64, 128, 2, 2>"),     # K = 64 on a real conv
    _r(WGRAD, F32, (16, 9, 9, 68, 4, 1), 1821, 0.0, 0, "k_wgrad_glds<256, 64, 4, 1>"),     # K = 256
    _r(WGRAD, F32, (32, 11, 13, 136, 3, 2), 2185, 0.0, 0, "k_wgrad_glds<128, 128, 2, 2>"),
    _r(WGRAD, F32, (32, 11, 13, 96, 3, 2), 2185, 0.0, 0, "k_wgrad_glds<128, 64, 2, 2>"),   # K = 288: no 256-row tiles
    _r(WGRAD, F32, (64, 1, 1, 520, 1, 1), 16399, 0.0, 0, "k_wgrad_glds_z<64, 128, 2, 2>"),
    _r(WGRAD, F32, (512, 1, 1, 8, 1, 1), 70001, 0.0, 0, "k_wgrad_glds_z<256, 64, 4, 1>"),
    _r(WGRAD, F32, (96, 1, 1, 160, 1, 1), 70001, 0.0, 0, "k_wgrad_glds_z<128, 128, 2, 2>"),
    _r(WGRAD, F32, (96, 1, 1, 72, 1, 1), 70001, 0.0, 0, "k_wgrad_glds_z<128, 64, 2, 2>"),
    # ---- sf_conv_dgrad (each row with and without the producer's ReLU mask)
    _r(DGRAD, F32, (16, 11, 13, 48, 3, 2), 37, 0.0, 1, "k_conv_dgrad<128, 32, 4, 1, true>"),
    _r(DGRAD, F32, (16, 1, 1, 5, 1, 1), 37, 0.0, 1, "k_conv_dgrad<128, 32, 4, 1, false>"),
    _r(DGRAD, F32, (40, 6, 6, 48, 3, 1), 37, 0.0, 1, "k_conv_dgrad<64, 64, 2, 2, true>"),
    _r(DGRAD, F32, (40, 1, 1, 5, 1, 1), 37, 0.0, 1, "k_conv_dgrad<64, 64, 2, 2, false>"),
    _r(DGRAD, F32, (64, 1, 1, 8, 1, 1), 140001, 0.0, 1, "k_conv_dgrad<128, 64, 2, 2, true>"),
    _r(DGRAD, F32, (64, 1, 1, 5, 1, 1), 140001, 0.0, 1, "k_conv_dgrad<128, 64, 2, 2, false>"),
    _r(DGRAD, F32, (16, 9, 9, 32, 3, 1), 1025, 0.0, 1, "k_dgrad_pix<256, 32, 4, 1>"),      # Cout % 64 != 0: no _z form
    _r(DGRAD, F32, (16, 9, 9, 64, 3, 1), 1025, 0.0, 1, "k_dgrad_pix_z<256, 32, 4, 1>"),
    _r(DGRAD, F32, (40, 6, 6, 96, 3, 1), 1025, 0.0, 1, "k_dgrad_pix<128, 64, 2, 2>"),
    _r(DGRAD, F32, (40, 6, 6, 64, 3, 1), 1025, 0.0, 1, "k_dgrad_pix_z<128, 64, 2, 2>"),
    _r(DGRAD, F32, (20, 10, 14, 96, 4, 2), 1025, 0.0, 1, "k_dgrad_quadrow<128, 128, 2, 2>"),
    _r(DGRAD, F32, (20, 10, 14, 64, 4, 2), 1025, 0.0, 1, "k_dgrad_quadrow_z<128, 128, 2, 2>"),
    _r(DGRAD, F32, (136, 1, 1, 96, 1, 1), 32700, 0.0, 1, "k_fwd_glds_z<128, 128, 2, 2>"),  # linear: masked forward GEMM
    _r(DGRAD, F32, (64, 1, 1, 544, 1, 1), 8193, 0.0, 1, "k_fwd_glds_z<64, 64, 2, 2>"),
    # ---- sf_conv_fwd_norm / sf_conv_wgrad_norm (MODE 4 f32 frames + tables, 5 u8 + tables, 2 scalar)
    _r(FWD_NORM, U8, NATURE1, 77, 3.0, 1, "k_conv_u8_img_norm<2, 4, 5, 16>"),
    _r(FWD_NORM, U8, (3, 36, 36, 16, 8, 4), 5, 3.0, 1, "k_conv_fwd<128, 32, 4, 1, 5>"),
    _r(FWD_NORM, F32F, (3, 36, 36, 16, 8, 4), 5, 1.5, 0, "k_conv_fwd<128, 32, 4, 1, 4>"),
    _r(FWD_NORM, U8, (1, 45, 53, 32, 8, 4), 3, 3.0, 1, "k_conv_fwd<128, 32, 4, 1, 2>"),
    _r(FWD_NORM, U8, (3, 36, 36, 16, 8, 4), 8193, 3.0, 1, "k_conv_fwd<256, 32, 4, 1, 5>"),
    _r(FWD_NORM, F32F, (3, 36, 36, 16, 8, 4), 8193, 0.0, 1, "k_conv_fwd<256, 32, 4, 1, 4>"),
    _r(FWD_NORM, F32F, (3, 13, 17, 16, 4, 2), 14981, 0.0, 1, "k_conv_fwd<256, 32, 4, 1, 2>"),        # Mtot 524335
    _r(FWD_NORM, U8, (3, 36, 36, 48, 8, 4), 3, 3.0, 1, "k_conv_fwd<128, 64, 2, 2, 5>"),
    _r(FWD_NORM, F32F, (3, 36, 36, 48, 8, 4), 3, 1.5, 1, "k_conv_fwd<128, 64, 2, 2, 4>"),
    _r(FWD_NORM, F32F, (3, 13, 17, 48, 4, 2), 3, 0.0, 0, "k_conv_fwd<128, 64, 2, 2, 2>"),
    _r(FWD_NORM, U8, (4, 36, 36, 48, 8, 4), 1, 3.0, 1, "k_conv_fwd<64, 64, 2, 2, 5>"),
    _r(FWD_NORM, F32F, (4, 36, 36, 48, 8, 4), 1, 0.0, 1, "k_conv_fwd<64, 64, 2, 2, 4>"),
    _r(FWD_NORM, U8, (3, 13, 17, 48, 4, 2), 1, 3.0, 1, "k_conv_fwd<64, 64, 2, 2, 2>"),
    _r(WGRAD_NORM, U8, NATURE1, 77, 3.0, 0, "k_conv1_wgrad_img_norm<2, 4>"),
    _r(WGRAD_NORM, U8, (3, 36, 36, 16, 8, 4), 5, 3.0, 0, "k_conv_wgrad<32, 4, 1, 5>"),
    _r(WGRAD_NORM, F32F, (3, 36, 36, 16, 8, 4), 5, 1.5, 0, "k_conv_wgrad<32, 4, 1, 4>"),
    _r(WGRAD_NORM, U8, (1, 45, 53, 32, 8, 4), 3, 3.0, 0, "k_conv_wgrad<32, 4, 1, 2>"),
    _r(WGRAD_NORM, U8, (3, 36, 36, 48, 8, 4), 3, 3.0, 0, "k_conv_wgrad<64, 2, 2, 5>"),
    _r(WGRAD_NORM, F32F, (3, 36, 36, 48, 8, 4), 3, 1.5, 0, "k_conv_wgrad<64, 2, 2, 4>"),
    _r(WGRAD_NORM, F32F, (3, 13, 17, 48, 4, 2), 3, 0.0, 0, "k_conv_wgrad<64, 2, 2, 2>"),
]

# (op, name) -> why no row pins it: kernels without a small shape, and compiled instantiations the DEFAULT dispatch cannot
# reach at any shape (a switch group reaches them, and then an existing row runs them: the roster is checked per group).
_BIG = ("selected only when an operand of the launch has 2^30 elements or more (the 32-bit lane offsets of the _z form no "
        "longer fit): gigabytes of operands, no shape a quick test can run")
_INT_MEAN = ("a zero mean is an integer, so the exact-product bf16 kernel takes every launch of this one by default; "
             "SF_CONV1_BF16=0 selects it, and the Nature conv1 rows with mean 0 then run it")
EXCLUDED = {
    (FWD_T, "k_fwd_glds<128, 64, 2, 2, 2>"): _BIG,  # (swept: conv2 at n = 140000 is 1.8e9 input elements)
    (FWD_T, "k_fwd_glds<64, 64, 2, 2, 2>"): _BIG,
    (FWD_T, "k_fwd_glds<128, 128, 2, 2, 2>"): _BIG,
    (DGRAD, "k_fwd_glds<64, 64, 2, 2, 2>"): _BIG,
    (DGRAD, "k_fwd_glds<128, 128, 2, 2, 2>"): _BIG,
    (FWD, "k_conv_u8_img<2, 4, 5, 16, false>"): _INT_MEAN,
    (WGRAD, "k_conv1_wgrad_img<2, 4, false>"): _INT_MEAN,
}


def make_desc(fmt, geom, mean=0.0, act=1):
    Cin, H, W, Cout, K, S = geom
    return lib.sf_conv_desc(Cin=Cin, H=H, W=W, Cout=Cout, KH=K, KW=K, stride=S, OH=(H - K) // S + 1, OW=(W - K) // S + 1,
                            in_u8=fmt, relu=act, traj_T=0, sub_mean=mean if fmt != F32 else 0.0, inv_scale=INV[fmt])


# ------------------------------------------------------------------------------------------------ float64 references
def _conv64(x, w, b, S):
    """F.conv2d in float64; a 1x1 layer on a 1x1 image as the matrix product it is (same operation, no per-sample loop)"""
    if w.shape[2] == 1 and w.shape[3] == 1 and x.shape[2] == 1 and x.shape[3] == 1:
        y = x.flatten(1) @ w.flatten(1).t()
        return (y if b is None else y + b)[:, :, None, None]
    return F.conv2d(x, w, b, stride=S)


def _rows(t):  # [n, C, OH, OW] -> [n * OH * OW, C], the kernels' output layout
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _to_kmajor(w, frame):  # OIHW -> [K, Cout]; frames: k = (c*KH + kh)*KW + kw, NHWC: k = (kh*KW + kw)*Cin + c
    O = w.shape[0]
    return (w.reshape(O, -1).t() if frame else w.permute(2, 3, 1, 0).reshape(-1, O)).contiguous()


class Case:
    """inputs of one (format, geometry, n, mean, normalised?) built the way tests/test_gpu_nn.py builds them, and the
    float64 results every row on them needs; built once, shared by the rows, never written to"""

    def __init__(self, fmt, geom, n, mean, norm):
        Cin, H, W, Cout, K, S = geom
        g = torch.Generator().manual_seed(Cin * 131 + H * 17 + Cout * 7 + n + int(mean * 2) + (5 if norm else 0))
        self.frame, self.S, self.stride = fmt != F32, S, Cin * H * W
        if fmt == U8:
            x = torch.randint(0, 256, (n, Cin, H, W), generator=g, dtype=torch.uint8)
            self.x_dev = x.cuda()
        elif fmt == F32F:
            x = torch.rand((n, Cin, H, W), generator=g) * 3.0 - 1.0
            self.x_dev = x.cuda()
        else:
            x = torch.randn((n, Cin, H, W), generator=g)
            self.x_dev = x.permute(0, 2, 3, 1).contiguous().cuda()  # NHWC
        self.x = x.double() if fmt == F32 else (x.double() - mean) * INV[fmt]
        self.xabs = self.x.abs()  # magnitude of the terms an input element is rounded against
        self.mu = self.rstd = None
        if norm:  # tables for pixels scaled to about [0, 1] (tests/test_gpu_u8_norm.py): part of every frame clamps at +-5
            mu = torch.rand(Cin * H * W, generator=g) * 0.6 + 0.2
            rstd = 1.0 / torch.sqrt(torch.rand(Cin * H * W, generator=g) * 0.2 + 1e-3)
            self.mu, self.rstd = mu.cuda(), rstd.cuda()
            m4, r4 = mu.double().view(1, Cin, H, W), rstd.double().view(1, Cin, H, W)
            self.xabs = (self.x.abs() + m4) * r4  # (clamping does not enlarge an error)
            self.x = ((self.x - m4) * r4).clamp(-5, 5)
            assert float((self.x.abs() == 5).double().mean()) > 1e-3
        self.w = torch.randn((Cout, Cin, K, K), generator=g) / np.sqrt(Cin * K * K)
        self.b = torch.randn(Cout, generator=g) * 0.1
        self.wk = _to_kmajor(self.w, self.frame).cuda()
        self.b_dev = self.b.cuda()
        self.OH, self.OW = (H - K) // S + 1, (W - K) // S + 1
        self.dy = torch.randn((n, Cout, self.OH, self.OW), generator=g)

    @functools.cached_property
    def dy_dev(self):
        return _rows(self.dy).contiguous().cuda()

    @functools.cached_property
    def forward(self):
        """(pre-activation, sum |x| |w| + |b|) as [n * OH * OW, Cout] float64"""
        w, b = self.w.double(), self.b.double()
        return _rows(_conv64(self.x, w, b, self.S)), _rows(_conv64(self.xabs, w.abs(), b.abs(), self.S))

    @functools.cached_property
    def grads(self):
        """(dW [K, Cout] in the kernel's layout, db, dX [n, H, W, Cin], sum |dy| |w| in dX's layout) for self.dy"""
        x, w = self.x.clone().requires_grad_(True), self.w.double().requires_grad_(True)
        b = self.b.double().requires_grad_(True)
        _conv64(x, w, b, self.S).backward(self.dy.double())
        xz = torch.zeros_like(self.x).requires_grad_(True)
        _conv64(xz, self.w.double().abs(), None, self.S).backward(self.dy.double().abs())
        return (_to_kmajor(w.grad, self.frame), b.grad, x.grad.permute(0, 2, 3, 1).contiguous(),
                xz.grad.permute(0, 2, 3, 1).contiguous())


@functools.lru_cache(maxsize=2)
def _case(fmt, geom, n, mean, norm):
    return Case(fmt, geom, n, mean, norm)


# ------------------------------------------------------------------------------------------------ guard bands
BAND, PATTERN = 4096, 0x3C5AA5C3  # elements on either side of an output, and the 32-bit pattern they hold


class Guarded:
    """an output tensor as a view into a larger buffer: BAND 32-bit words of PATTERN before and after it, 7.0 inside"""

    def __init__(self, shape, nbytes=None):
        words = int(np.prod(shape)) if nbytes is None else nbytes // 4
        assert nbytes is None or nbytes % 4 == 0
        self.words = words
        self.buf = torch.empty(words + 2 * BAND, dtype=torch.int32, device="cuda")
        self.buf.fill_(PATTERN)
        inner = self.buf[BAND:BAND + words].view(torch.float32)
        inner.fill_(7.0)
        self.t = inner.view(torch.uint8) if nbytes is not None else inner.view(shape)

    def intact(self):
        return bool((self.buf[:BAND] == PATTERN).all()) and bool((self.buf[BAND + self.words:] == PATTERN).all())


def _workspace(nbytes):
    return Guarded(None, nbytes) if nbytes else None


# ------------------------------------------------------------------------------------------------ the checks
U = 2.0 ** -24


def _elementwise(got, ref, mag, L, what):
    """|got - ref| <= 2 gamma_L mag + 2u |ref|: the a-priori bound of an f32 sum of L products in ANY order (the factor 2:
    the matrix pipe's internal order is not documented); +19: 16 split-K slices, the bias add, the input scaling"""
    gam = (L + 19) * U / (1.0 - (L + 19) * U)
    bound = 2.0 * gam * mag + 2.0 * U * ref.abs() + 1e-30
    ratio = float(((got - ref).abs() / bound).max())
    assert ratio <= 1.0, f"{what}: an element is {ratio:.3g} x its a-priori bound (L = {L})"
    return ratio


def _maxnorm(got, ref, tol, what):
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    assert err <= tol * max(1.0, scale), f"{what}: max|err| {err:.3g} > {tol:g} * max(1, {scale:.3g})"
    return err / scale if scale > 0 else 0.0


def _run_forward(row, d, c):
    Cin, H, W, Cout, K, S = row.geom
    M = row.n * d.OH * d.OW

    def launch():
        out = Guarded((M, Cout))
        if row.op == FWD:
            ws = _workspace(lib.conv_fwd_workspace(row.n, d))
            lib.conv_fwd(c.x_dev, c.stride, None, 0, c.wk, c.b_dev, out.t, row.n, d, ws.t if ws else None)
        elif row.op == FWD_T:
            ws = _workspace(lib.conv_fwd_t_workspace(row.n, d))
            lib.conv_fwd_t(c.x_dev, c.stride, wt, c.b_dev, out.t, row.n, d, ws.t if ws else None)
        else:
            ws = None
            lib.conv_fwd_norm(c.x_dev, c.stride, None, 0, c.mu, c.rstd, c.wk, c.b_dev, out.t, row.n, d)
        torch.cuda.synchronize()
        assert out.intact(), "the forward wrote outside its output"
        assert ws is None or ws.intact(), "the forward wrote outside its workspace"
        return out.t

    wt = c.wk.t().contiguous() if row.op == FWD_T else None
    out = launch()
    pre, mag = c.forward
    ref = torch.relu(pre) if row.act == 1 else pre  # (ReLU does not enlarge an error)
    got = out.cpu().double()
    rel = _maxnorm(got, ref, 3e-5, "forward")
    bf16 = lib.conv_kernel_name(row.op, row.n, d).startswith("k_conv1_u8_bf16")  # three exact bf16 terms per weight
    ratio = _elementwise(got, ref, mag, (3 if bf16 else 1) * K * K * Cin, "forward")
    assert torch.equal(out, launch()), "two launches differ: the summation order is not fixed"
    return [("out", rel, ratio)]


def _run_wgrad(row, d, c):
    Cin, H, W, Cout, K, S = row.geom
    M = row.n * d.OH * d.OW
    assert M <= 202500, "no row reduces over more rows than tests/test_gpu_nn.py already holds to 2e-4"
    tol = 3e-5 if M < 65536 else 2e-4

    def launch():
        dw, db = Guarded((K * K * Cin, Cout)), Guarded((Cout,))
        ws = _workspace(lib.conv_wgrad_workspace(row.n, d))
        if row.op == WGRAD:
            lib.conv_wgrad(c.x_dev, c.stride, None, 0, c.dy_dev, dw.t, db.t, row.n, d, ws.t)
        else:
            lib.conv_wgrad_norm(c.x_dev, c.stride, None, 0, c.mu, c.rstd, c.dy_dev, dw.t, db.t, row.n, d, ws.t)
        torch.cuda.synchronize()
        assert dw.intact() and db.intact(), "the weight gradient wrote outside dw / db"
        assert ws.intact(), "the weight gradient wrote outside its workspace"
        return dw.t, db.t

    dw, db = launch()
    gw, gb, _, _ = c.grads
    res = [("dw", _maxnorm(dw.cpu().double(), gw, tol, "weight gradient"), None),
           ("db", _maxnorm(db.cpu().double(), gb, tol, "bias gradient"), None)]
    dw2, db2 = launch()
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two launches differ: the summation order is not fixed"
    return res


def _run_dgrad(row, d, c):
    Cin, H, W, Cout, K, S = row.geom
    _, _, gx, gmag = c.grads
    mask = (c.x > 0).permute(0, 2, 3, 1)
    res = []
    for act, ref, mag, what in ((c.x_dev, gx * mask, gmag * mask, "dgrad"), (None, gx, gmag, "dgrad nomask")):
        def launch():
            din = Guarded((row.n, H, W, Cin))
            lib.conv_dgrad(c.dy_dev, c.wk, act, din.t, row.n, d)
            torch.cuda.synchronize()
            assert din.intact(), "the data gradient wrote outside din"
            return din.t

        din = launch()
        got = din.cpu().double()
        rel = _maxnorm(got, ref, 3e-5, what)
        res.append((what, rel, _elementwise(got, ref, mag, K * K * Cout, what)))
        assert torch.equal(din, launch()), "two launches differ: the summation order is not fixed"
    return res


@pytest.mark.parametrize("row", LEDGER, ids=[r.id for r in LEDGER])
def test_ledger_row(row):
    d = make_desc(row.fmt, row.geom, row.mean, row.act)
    if row.op == FWD_T and not lib.conv_fwd_t_supported(row.n, d):
        assert not DEFAULT_SWITCHES, "the default dispatch must take this launch"
        pytest.skip("the switch under test sends this launch to sf_conv_fwd")
    if row.op >= FWD_NORM and not lib.conv_norm_supported(row.n, d):
        assert not DEFAULT_SWITCHES, "the default dispatch must take this launch"
        pytest.skip("the switch under test turns the normalising entry points off")
    name = lib.conv_kernel_name(row.op, row.n, d)
    if DEFAULT_SWITCHES:
        assert name == row.name
    c = _case(row.fmt, row.geom, row.n, row.mean, row.op >= FWD_NORM)
    run = _run_forward if row.op in (FWD, FWD_T, FWD_NORM) else _run_dgrad if row.op == DGRAD else _run_wgrad
    for what, rel, ratio in run(row, d, c):
        print(f"ledger {row.id} {name} {what}: max|err|/max|ref| {rel:.3g}" +
              ("" if ratio is None else f" max(err/bound) {ratio:.3g}"))


def test_ledger_table_is_well_formed():
    """every row has its own id; data gradients and sf_conv_fwd_t take activations, the normalising entry points frames"""
    assert len({r.id for r in LEDGER}) == len(LEDGER)
    assert all(r.fmt == F32 for r in LEDGER if r.op in (DGRAD, FWD_T))
    assert all(r.fmt != F32 for r in LEDGER if r.op >= FWD_NORM)


# ------------------------------------------------------------------------------------------------ the roster
FIRST_LAYERS = [  # read observation frames (u8 or f32) or, as activations, f32 NHWC
    NATURE1, (3, 72, 128, 32, 8, 4), (4, 84, 84, 16, 8, 4),                      # Nature CNN, convnet_simple, convnet_impala
    (4, 84, 84, 24, 8, 4), (4, 36, 36, 32, 8, 4), (4, 36, 36, 48, 8, 4), (3, 36, 36, 16, 8, 4), (3, 36, 36, 48, 8, 4),
    (1, 45, 53, 32, 8, 4), (3, 13, 17, 16, 4, 2), (3, 13, 17, 48, 4, 2), (3, 9, 9, 5, 3, 1), (3, 9, 9, 48, 3, 1),
    (3, 9, 9, 50, 3, 1), (4, 9, 9, 8, 3, 1), (4, 20, 20, 128, 4, 2),
]
INNER_LAYERS = [  # f32 NHWC only
    CONV2, CONV3, (3136, 1, 1, 512, 1, 1),                                        # Nature CNN
    (32, 17, 31, 64, 4, 2), (64, 7, 14, 128, 3, 2), (2304, 1, 1, 512, 1, 1),      # convnet_simple on 3x72x128
    (16, 20, 20, 32, 4, 2), (2592, 1, 1, 512, 1, 1),                              # convnet_impala
    (512, 1, 1, 2048, 1, 1), (512, 1, 1, 1536, 1, 1), (64, 1, 1, 2048, 1, 1),     # recurrent projections
    *[(512, 1, 1, a, 1, 1) for a in range(6, 21)], *[(64, 1, 1, a, 1, 1) for a in (5, 6, 8, 17, 20)],  # heads
    (16, 11, 13, 48, 3, 2), (8, 6, 6, 128, 3, 1), (16, 9, 9, 32, 3, 1), (16, 9, 9, 64, 3, 1), (16, 9, 9, 68, 4, 1),
    (40, 6, 6, 48, 3, 1), (40, 6, 6, 64, 3, 1), (40, 6, 6, 96, 3, 1), (20, 10, 14, 64, 4, 2), (20, 10, 14, 96, 4, 2),
    (32, 11, 13, 96, 3, 2), (32, 11, 13, 136, 3, 2), (32, 12, 14, 64, 3, 2), (64, 5, 5, 136, 5, 1), (33, 7, 7, 7, 3, 1),
    (16, 1, 1, 5, 1, 1), (27, 1, 1, 17, 1, 1), (27, 1, 1, 64, 1, 1), (32, 1, 1, 160, 1, 1), (40, 1, 1, 5, 1, 1),
    (48, 1, 1, 7, 1, 1), (48, 1, 1, 20, 1, 1), (64, 1, 1, 64, 1, 1), (64, 1, 1, 520, 1, 1), (64, 1, 1, 544, 1, 1),
    (96, 1, 1, 72, 1, 1), (96, 1, 1, 160, 1, 1), (136, 1, 1, 96, 1, 1), (384, 1, 1, 160, 1, 1), (512, 1, 1, 8, 1, 1),
    (1024, 1, 1, 200, 1, 1), (1056, 1, 1, 136, 1, 1), (3136, 1, 1, 7, 1, 1), (3136, 1, 1, 136, 1, 1), (3136, 1, 1, 520, 1, 1),
]
SWEEP_N = [1, 3, 5, 37, 77, 130, 257, 513, 1025, 2049, 4096, 8193, 10700, 16399, 32769, 70001, 140000]


def roster_sweep():
    """{(op, kernel name): [(fmt, geom, n, mean), ...]} over the fixed grid; host-only calls"""
    seen = {}
    launches = [(F32, g, 0.0) for g in FIRST_LAYERS + INNER_LAYERS]
    launches += [(fmt, g, mean) for fmt in (U8, F32F) for g in FIRST_LAYERS for mean in (0.0, 3.0, 1.5)]
    for fmt, geom, mean in launches:
        d = make_desc(fmt, geom, mean)
        for n in SWEEP_N:
            if n * d.OH * d.OW >= 2 ** 31:
                continue
            ops = [FWD, WGRAD]
            if fmt == F32 and (geom[3] % 4 == 0 or geom[4] == 1):  # what sf_conv_dgrad accepts
                ops.append(DGRAD)
            if lib.conv_fwd_t_supported(n, d):
                ops.append(FWD_T)
            if lib.conv_norm_supported(n, d):
                ops += [FWD_NORM, WGRAD_NORM]
            for op in ops:
                seen.setdefault((op, lib.conv_kernel_name(op, n, d)), []).append((fmt, geom, n, mean))
    return seen


def test_roster_every_selectable_kernel_has_a_row():
    """names are computed in THIS process, so the check also holds under non-default switches: a kernel a switch makes
    selectable needs a row that reaches it under that switch, or a reason"""
    lib.load()
    torch.cuda.init()  # the occupancy queries of the plans answer for the device
    pinned = {(r.op, lib.conv_kernel_name(r.op, r.n, make_desc(r.fmt, r.geom, r.mean, r.act))) for r in LEDGER
              if r.op != FWD_T or lib.conv_fwd_t_supported(r.n, make_desc(r.fmt, r.geom, r.mean, r.act))}
    seen = roster_sweep()
    assert sum(len(v) for v in seen.values()) > 3000
    missing = {k: v[0] for k, v in seen.items() if k not in pinned and k not in EXCLUDED}
    assert not missing, "selectable kernels without a ledger row (op, name) -> first launch that picks it:\n" + \
        "\n".join(f"  {k}: {v}" for k, v in sorted(missing.items()))
    if DEFAULT_SWITCHES:
        assert pinned == {(r.op, r.name) for r in LEDGER}
        assert not set(EXCLUDED) & pinned, "an excluded kernel has a row after all"


# ------------------------------------------------------------------------------------------------ the A/B switch groups
def _groups():
    from tests.test_gpu_switches import GROUPS
    return [g[0] for g in GROUPS]


@pytest.mark.parametrize("switches", _groups())
def test_ledger_and_roster_under_non_default_switches(switches):
    """every row's numerics, guard bands and reproducibility (the name asserts are suspended) and the roster, in a fresh
    process per group of A/B switches"""
    env = dict(os.environ, **dict(kv.split("=") for kv in switches.split()))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_ledger_row or test_roster", "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    tail = r.stdout[-2500:]
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, f"{switches}:\n{tail}\n{r.stderr[-500:]}"


# ------------------------------------------------------------------------------------------------ names under a switch
# Launches whose kernel a switch changes.  sf_conv_kernel_name answers from the plan the launcher runs, so the name
# follows the switch (the hand-kept query this replaced reported the default kernel in each of these cases); the expected
# names were checked against a rocprofv3 kernel trace of the rows under the switch groups (profiles/conv_plan_same_launches.log).
SWITCHED_NAMES = [
    ("SF_DGRAD_PIX=2", [(DGRAD, F32, (16, 9, 9, 32, 3, 1), 1025, 0.0, "k_dgrad_pix<128, 32, 4, 1>")]),
    ("SF_CONV1_BF16=0 SF_CONV1_IMG=0", [(FWD, U8, NATURE1, 257, 3.0, "k_conv_fwd<128, 32, 4, 1, 1>"),
                                        (WGRAD, U8, NATURE1, 257, 3.0, "k_conv_wgrad<32, 4, 1, 1>")]),
    ("SF_WGRAD_GLDS=0", [(WGRAD, F32, (96, 1, 1, 72, 1, 1), 70001, 0.0, "k_conv_wgrad<64, 2, 2, 0>")]),
]
_NAME_QUERIES = """
import json, sys
from tests.test_gpu_kernel_ledger import lib, make_desc
print(json.dumps([lib.conv_kernel_name(op, n, make_desc(fmt, tuple(geom), mean)) for op, fmt, geom, n, mean in json.loads(sys.argv[1])]))
"""


@pytest.mark.parametrize("switches,cases", SWITCHED_NAMES, ids=[s.replace(" ", ",") for s, _ in SWITCHED_NAMES])
def test_kernel_name_follows_the_switches(switches, cases):
    """name queries only, in a fresh process (the switches are read once per process)"""
    import json
    env = dict(os.environ, **dict(kv.split("=") for kv in switches.split()))
    r = subprocess.run([sys.executable, "-c", _NAME_QUERIES, json.dumps([c[:5] for c in cases])], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [c[5] for c in cases]
