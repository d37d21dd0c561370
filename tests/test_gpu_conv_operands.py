"""The conv kernels under the operands sf_conv_kernel_name cannot see.  The name query plans for query_operands() (every
pointer aligned, dense samples, no index, traj_T = 0, a large enough split-K workspace) and tests/test_gpu_kernel_ledger.py
launches exactly that.  This file runs the ledger's geometries (A) through the loaders' sample addressing and (B) through
every branch of plan_conv_fwd / plan_conv_wgrad / plan_conv_dgrad that depends on an operand, with the ledger's float64
references and bounds (no tolerance of its own), guard bands, unchanged inputs and bit reproducibility.  The kernel of a
launch here cannot be asserted (the query does not see the operands): the tables below say which kernel the plan selects, as
read from csrc/sf_nn.hip; the names the ledger pins are asserted for the dense launches this file compares with.

What the suite reached before this file (and this file does not repeat):
  * tests/test_gpu_nn.py test_conv1_reads_slab_in_place: k_conv_fwd MODE 1 at (4, 36, 36, 32, 8, 4) n = 16 / 8, index + traj_T
    and offset + traj_T against a dense copy (bytes), sample stride == sample size, no padding, forward only.
  * tests/test_gpu_nn.py test_conv1_strip_image_kernels_read_slab_in_place: the bf16 strip kernels (forward n = 300 / 264,
    weight gradient n = 300) at mean 0, index + traj_T and offset + traj_T, bytes of a dense copy, stride == sample size.
  * tests/test_gpu_nn.py test_conv1_relu_sign_bits_between_forward_and_weight_gradient: the sign-bit forms through
    index + traj_T at n = 300, compared with the plain entry points; its refusal: a launch below n = 256.
  * tests/test_gpu_nn.py test_conv1_loader_fused_normalisation_vs_float64 and tests/test_gpu_u8_norm.py
    test_conv_fwd_wgrad_norm_on_u8_frames_vs_float64: the normalising strip kernels and MODE 5 / MODE 2 on u8 frames,
    offset 2 or an index WITHOUT repeats, traj_T 5 / 8, stride == sample size, max-norm against float64.
  * tests/test_gpu_f32_frames.py test_conv_fwd_wgrad_on_f32_frames: MODE 3 / 4 / 2 on four geometries at n = 7 .. 10 in the
    modes dense / index / traj / strided (stride = sample + 4), allclose against float64.
  * tests/test_gpu_headline_sizes.py test_forward_rows_do_not_depend_on_batch_position and
    test_conv1_reads_the_last_rows_of_a_32768_env_slab: conv1's bf16 forward through an index at the headline size.
  * tests/test_gpu_fwd_two_segment.py test_refusals: sf_conv_fwd_t_os2 with a misaligned dense segment.
  * the odd-address tests (test_gpu_nn.py test_fused_input_normalisation_on_a_frame_view_at_an_odd_address,
    test_gpu_u8_norm.py test_frames_at_an_odd_address_give_the_same_heads, test_gpu_f32_frames.py
    test_normalize_input_fused_and_materialised_agree) run the MODEL, which gathers such frames into an aligned copy: no
    misaligned pointer reaches the C ABI in them, and no test passed a misaligned weight, gradient, output or table, a
    sample stride off the 4-element grid or a short split-K workspace to a conv entry point.
None of them walks the ledger's list: MODE 0 / 2 through an index, every 256-row and 64-row tile form, the f32 strip kernels
(k_conv_u8_img, k_conv1_wgrad_img), the LDS-image / LDS-DMA weight gradients and k_linear_wgrad_small with an offset or a
padded stride were unreached.

Part A.  One case per ledger row of ops FWD, WGRAD, FWD_NORM, WGRAD_NORM (+ the sign-bit forms at the Nature conv1 rows): the
row's geometry, format, mean and n on a slab [E, T + 1] (T = 3, E = ceil((n + 7) / T) + 1) whose samples are PAD = 4 elements
longer than a sample; the padding and the t == T rows hold poison (NaN; 255 for u8, whose real pixels stay below 255).  Modes:
  offset       index NULL, offset 5, traj_T = T (the run crosses trajectory boundaries)
  index        a fixed-seed permutation of the dataset rows with repeats, traj_T = T
  index_flat   the same index, traj_T = 0, on a dense array of the same padded samples
  offset_flat  index NULL, offset 5, traj_T = 0 on that array: the one mode in which plan_conv_wgrad still selects
               k_linear_wgrad_small / k_wgrad_img / k_wgrad_glds(_z), which take neither index nor offset as an argument
Where the plan selects the row's kernel whatever the addressing (every forward row; weight gradients outside the table
below) the result equals, byte for byte, the dense launch on a host-gathered aligned copy of the same samples.

    ledger kernel (dense launch)      excluded by                              the launch then runs (plan_conv_wgrad)
    k_linear_wgrad_small              o.index, or traj_T != 0 (linear_1x1)      k_conv_wgrad<32 | 64, .., MODE 0 or 2>
    k_wgrad_img<..>                   o.index, or traj_T != 0                   k_conv_wgrad<64, 2, 2, 0>
    k_wgrad_glds<..> / _z<..>         o.index, or traj_T != 0                   k_conv_wgrad<64 | 32, .., 0>
  (modes offset, index, index_flat; these are held to the float64 bound only.  offset_flat keeps the ledger kernel.)

Part B.  One operand fact broken per case at the geometry and n at which the aligned launch selects the specialised
kernel: B_CASES, with the kernel the plan falls to.  Entry points that refuse instead: test_refusals_leave_the_output_alone.
Part C.  test_every_operand_branch_has_a_case.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_kernel_ledger import (BAND, CONV2, CONV3, DEFAULT_SWITCHES, DGRAD, F32, F32F, FWD, FWD_NORM,  # noqa: E402
                                          FWD_T, INV, LEDGER, NATURE1, PATTERN, U8, WGRAD, WGRAD_NORM, Case, Guarded,
                                          _conv64, _elementwise, _maxnorm, _rows, _to_kmajor, make_desc)

T, PAD, OFFSET = 3, 4, 5
MODES = ("offset", "index", "index_flat", "offset_flat")
NAN = float("nan")
NO_INDEX_KERNELS = ("k_linear_wgrad_small", "k_wgrad_img", "k_wgrad_glds")  # the table above


def _bits(t):
    """a tensor as integers, so that NaN poison compares equal to itself"""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Carved:
    """`words` 32-bit words starting `off` words past a 16-byte boundary, NaN-filled, PATTERN on either side"""

    def __init__(self, words, off=0):
        self.words, self.lo = int(words), BAND + off
        self.buf = torch.full((self.words + 2 * BAND + off,), PATTERN, dtype=torch.int32, device="cuda")
        self.t = self.buf[self.lo:self.lo + self.words].view(torch.float32)
        self.t.fill_(NAN)
        assert self.t.data_ptr() % 16 == 4 * off

    def intact(self):
        return bool((self.buf[:self.lo] == PATTERN).all()) and bool((self.buf[self.lo + self.words:] == PATTERN).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def _off_grid(t):
    """a contiguous copy of t whose base is one ELEMENT past an aligned address (f32: 4 bytes off 16, u8: 1 byte off 4)"""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size()
    return v


# ================================================================================================ Part A: addressing
class SlabCase:
    """the inputs of one ledger row as a dataset of E * T samples: a slab [E, T + 1, size + PAD] and a dense strided array
    [E * T + 1, size + PAD], poison wherever no sample lives; float64 inputs per dataset row; built once, never written"""

    def __init__(self, fmt, geom, n, mean, norm):
        Cin, H, W, Cout, K, S = geom
        g = torch.Generator().manual_seed(Cin * 131 + H * 17 + Cout * 7 + n + int(mean * 2) + (5 if norm else 0) + 1000)
        self.n, self.E = n, -(-(n + 7) // T) + 1
        R = self.R = self.E * T
        self.frame, self.S, self.size = fmt != F32, S, Cin * H * W
        self.pitch = self.size + PAD
        if fmt == U8:
            x = torch.randint(0, 255, (R, Cin, H, W), generator=g, dtype=torch.uint8)  # (a real pixel is never 255)
            rows, poison = x.reshape(R, -1), 255
        elif fmt == F32F:
            x = torch.rand((R, Cin, H, W), generator=g) * 3.0 - 1.0
            rows, poison = x.reshape(R, -1), NAN
        else:
            x = torch.randn((R, Cin, H, W), generator=g)
            rows, poison = x.permute(0, 2, 3, 1).reshape(R, -1), NAN  # NHWC
        flat = torch.full((R + 1, self.pitch), poison, dtype=rows.dtype)
        flat[:R, :self.size] = rows
        slab = torch.full((self.E, T + 1, self.pitch), poison, dtype=rows.dtype)
        slab[:, :T, :self.size] = rows.view(self.E, T, self.size)
        self.flat_dev, self.slab_dev = flat.cuda(), slab.cuda()
        self.flat_ref, self.slab_ref = self.flat_dev.clone(), self.slab_dev.clone()
        self.x = x.double() if fmt == F32 else (x.double() - mean) * INV[fmt]
        self.xabs = self.x.abs()
        self.mu = self.rstd = None
        if norm:  # the ledger's tables: part of every frame clamps at +-5
            mu = torch.rand(self.size, generator=g) * 0.6 + 0.2
            rstd = 1.0 / torch.sqrt(torch.rand(self.size, generator=g) * 0.2 + 1e-3)
            self.mu, self.rstd = mu.cuda(), rstd.cuda()
            m4, r4 = mu.double().view(1, Cin, H, W), rstd.double().view(1, Cin, H, W)
            self.xabs = (self.x.abs() + m4) * r4
            self.x = ((self.x - m4) * r4).clamp(-5, 5)
        self.w = torch.randn((Cout, Cin, K, K), generator=g) / np.sqrt(Cin * K * K)
        self.b = torch.randn(Cout, generator=g) * 0.1
        self.wk, self.b_dev = _to_kmajor(self.w, self.frame).cuda(), self.b.cuda()
        self.OH, self.OW = (H - K) // S + 1, (W - K) // S + 1
        self.dy = torch.randn((n, Cout, self.OH, self.OW), generator=g)
        self.dy_dev = _rows(self.dy).contiguous().cuda()
        perm = torch.randperm(R, generator=g)[:n]
        if n >= 3:
            perm[n - 1] = perm[0]
        if n >= 8:
            perm[5], perm[6] = perm[2], perm[2]
        self.index = perm
        self.index_dev = perm.to(torch.int32).cuda()

    def rows(self, mode):
        return self.index if mode.startswith("index") else torch.arange(OFFSET, OFFSET + self.n)

    def operands(self, mode):
        """(source, pristine copy, index, offset, traj_T) of a launch in this mode"""
        slab = mode in ("offset", "index")
        src, ref = (self.slab_dev, self.slab_ref) if slab else (self.flat_dev, self.flat_ref)
        return src, ref, self.index_dev if mode.startswith("index") else None, 0 if mode.startswith("index") else OFFSET, \
            T if slab else 0

    def dense(self, mode):
        """the samples of the launch gathered on the host side into an aligned dense [n, size] array"""
        return self.flat_dev[self.rows(mode).cuda(), :self.size].contiguous()

    @functools.cached_property
    def forward_all(self):
        """(pre-activation, sum |x| |w| + |b|) of EVERY dataset row as [R, OH * OW, Cout] float64"""
        w, b = self.w.double(), self.b.double()
        pre, mag = _conv64(self.x, w, b, self.S), _conv64(self.xabs, w.abs(), b.abs(), self.S)
        return [t.permute(0, 2, 3, 1).reshape(self.R, -1, t.shape[1]) for t in (pre, mag)]

    def grads(self, mode, dy=None):
        """(dW [K, Cout], db) of the samples of the launch for self.dy (or dy), float64; the weights do not enter"""
        w = torch.zeros_like(self.w, dtype=torch.float64).requires_grad_(True)
        b = torch.zeros_like(self.b, dtype=torch.float64).requires_grad_(True)
        _conv64(self.x[self.rows(mode)], w, b, self.S).backward((self.dy if dy is None else dy).double())
        return _to_kmajor(w.grad, self.frame), b.grad


@functools.lru_cache(maxsize=1)
def _slab_case(fmt, geom, n, mean, norm):
    return SlabCase(fmt, geom, n, mean, norm)


def _fwd_launch(op, d, c, src, stride, index, offset, w=None, mu=None, rstd=None, out_off=0, with_mask=False, ws_bytes=None):
    """one forward launch into NaN-filled guarded buffers -> (out [M, Cout], sign-bit words | None, workspace | None)"""
    M = c.n * c.OH * c.OW
    out = Carved(M * d.Cout, out_off)
    mask, ws = (Carved(M) if with_mask else None), None
    w = c.wk if w is None else w
    if op == FWD and with_mask:
        lib.conv_fwd_relu_mask(src, stride, index, offset, w, c.b_dev, out.t.view(M, d.Cout), mask.t.view(torch.int32), c.n, d)
    elif op == FWD:
        nb = lib.conv_fwd_workspace(c.n, d) if ws_bytes is None else ws_bytes
        ws = Guarded(None, nb) if nb else None
        lib.conv_fwd(src, stride, index, offset, w, c.b_dev, out.t.view(M, d.Cout), c.n, d, ws.t if ws else None)
    else:
        lib.conv_fwd_norm(src, stride, index, offset, c.mu if mu is None else mu, c.rstd if rstd is None else rstd, w,
                          c.b_dev, out.t.view(M, d.Cout), c.n, d)
    torch.cuda.synchronize()
    assert out.intact(), "the forward wrote outside its output"
    assert mask is None or mask.intact(), "the forward wrote outside its sign-bit words"
    assert ws is None or ws.intact(), "the forward wrote outside its workspace"
    return out.t.view(M, d.Cout), None if mask is None else mask.t.view(torch.int32), ws


def _wgrad_launch(op, d, c, src, stride, index, offset, dy=None, mu=None, rstd=None, mask=None):
    """one weight-gradient launch -> (dw [K, Cout], db [Cout]), guard bands checked"""
    K = d.KH * d.KW * d.Cin
    dw, db = Carved(K * d.Cout), Carved(d.Cout)
    ws = Guarded(None, lib.conv_wgrad_workspace(c.n, d))
    dy = c.dy_dev if dy is None else dy
    if mask is not None:
        lib.conv_wgrad_relu_mask(src, stride, index, offset, dy, mask, dw.t.view(K, d.Cout), db.t, c.n, d, ws.t)
    elif op == WGRAD:
        lib.conv_wgrad(src, stride, index, offset, dy, dw.t.view(K, d.Cout), db.t, c.n, d, ws.t)
    else:
        lib.conv_wgrad_norm(src, stride, index, offset, c.mu if mu is None else mu, c.rstd if rstd is None else rstd, dy,
                            dw.t.view(K, d.Cout), db.t, c.n, d, ws.t)
    torch.cuda.synchronize()
    assert dw.intact() and db.intact(), "the weight gradient wrote outside dw / db"
    assert ws.intact(), "the weight gradient wrote outside its workspace"
    return dw.t.view(K, d.Cout), db.t


def _check_forward(out, pre, mag, row_or_L, act, what):
    ref = torch.relu(pre) if act == 1 else pre
    got = out.cpu().double()
    rel = _maxnorm(got, ref, 3e-5, what)
    return rel, _elementwise(got, ref, mag, row_or_L, what)


def _wgrad_tol(M):
    assert M <= 202500, "no row reduces over more rows than tests/test_gpu_nn.py already holds to 2e-4"
    return 3e-5 if M < 65536 else 2e-4


def _norm_skip(row, d):
    if row.op >= FWD_NORM and not lib.conv_norm_supported(row.n, d):
        assert not DEFAULT_SWITCHES, "the default dispatch must take this launch"
        pytest.skip("the switch under test turns the normalising entry points off")


A_ROWS = [r for r in LEDGER if r.op in (FWD, WGRAD, FWD_NORM, WGRAD_NORM)]
A_PARAMS = [(r, m) for r in A_ROWS for m in MODES]


@pytest.mark.parametrize("row,mode", A_PARAMS, ids=[f"{r.id}-{m}" for r, m in A_PARAMS])
def test_addressing(row, mode):
    Cin, H, W, Cout, K, S = row.geom
    d0 = make_desc(row.fmt, row.geom, row.mean, row.act)
    _norm_skip(row, d0)
    name = lib.conv_kernel_name(row.op, row.n, d0)  # the kernel of the DENSE launch
    if DEFAULT_SWITCHES:
        assert name == row.name
    c = _slab_case(row.fmt, row.geom, row.n, row.mean, row.op >= FWD_NORM)
    src, pristine, index, offset, traj = c.operands(mode)
    d = make_desc(row.fmt, row.geom, row.mean, row.act)
    d.traj_T = traj
    rows = c.rows(mode)
    if row.op in (FWD, FWD_NORM):
        out, _, _ = _fwd_launch(row.op, d, c, src, c.pitch, index, offset)
        pre, mag = (t[rows].reshape(-1, Cout) for t in c.forward_all)
        L = (3 if name.startswith("k_conv1_u8_bf16") else 1) * K * K * Cin  # three exact bf16 terms per weight
        rel, ratio = _check_forward(out, pre, mag, L, row.act, f"forward ({mode})")
        print(f"operands {row.id} {mode} {name}: max|err|/max|ref| {rel:.3g} max(err/bound) {ratio:.3g}")
        again, _, _ = _fwd_launch(row.op, d, c, src, c.pitch, index, offset)
        assert torch.equal(_bits(out), _bits(again)), "two launches differ: the summation order is not fixed"
        dense, _, _ = _fwd_launch(row.op, d0, c, c.dense(mode), c.size, None, 0)
        assert torch.equal(_bits(out), _bits(dense)), "a sample's result depends on where it was read from"
    else:
        tol = _wgrad_tol(row.n * c.OH * c.OW)
        dw, db = _wgrad_launch(row.op, d, c, src, c.pitch, index, offset)
        gw, gb = c.grads(mode)
        rw, rb = _maxnorm(dw.cpu().double(), gw, tol, f"weight gradient ({mode})"), \
            _maxnorm(db.cpu().double(), gb, tol, f"bias gradient ({mode})")
        print(f"operands {row.id} {mode} {name}: dw {rw:.3g} db {rb:.3g}")
        dw2, db2 = _wgrad_launch(row.op, d, c, src, c.pitch, index, offset)
        assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(db), _bits(db2)), "two launches differ"
        if mode == "offset_flat" or not name.startswith(NO_INDEX_KERNELS):
            dwd, dbd = _wgrad_launch(row.op, d0, c, c.dense(mode), c.size, None, 0)
            assert torch.equal(_bits(dw), _bits(dwd)) and torch.equal(_bits(db), _bits(dbd)), \
                "the result depends on where the samples were read from"
    assert torch.equal(_bits(src), _bits(pristine)), "the launch wrote into its input"


MASK_ROWS = [r for r in LEDGER if r.geom == NATURE1 and r.fmt == U8 and r.op in (FWD, WGRAD) and r.mean == float(int(r.mean))
             and (r.op == WGRAD or r.act == 1)]
MASK_PARAMS = [(r, m) for r in MASK_ROWS for m in MODES]


@pytest.mark.parametrize("row,mode", MASK_PARAMS, ids=[f"{r.id}-{m}" for r, m in MASK_PARAMS])
def test_addressing_of_the_sign_bit_forms(row, mode):
    """sf_conv_fwd_relu_mask / sf_conv_wgrad_relu_mask at the Nature conv1 rows (ReLU, the bf16 kernels): the forward's words
    are the signs of its output, the weight gradient of the UNMASKED dY under those words is the float64 gradient of dY times
    the signs; both equal the dense launch byte for byte"""
    Cin, H, W, Cout, K, S = row.geom
    d0 = make_desc(row.fmt, row.geom, row.mean, 1)
    if not lib.conv_relu_mask_supported(row.n, d0):
        assert not DEFAULT_SWITCHES, "the default dispatch records sign bits for this launch"
        pytest.skip("the switch under test turns the sign-bit kernels off")
    c = _slab_case(row.fmt, row.geom, row.n, row.mean, False)
    src, pristine, index, offset, traj = c.operands(mode)
    d = make_desc(row.fmt, row.geom, row.mean, 1)
    d.traj_T = traj
    rows = c.rows(mode)
    out, mask, _ = _fwd_launch(FWD, d, c, src, c.pitch, index, offset, with_mask=True)
    signs = ((mask.view(-1, 1) >> torch.arange(32, device="cuda", dtype=torch.int32)) & 1).bool()
    assert torch.equal(signs, out > 0), "the sign-bit words are not the signs of the output"
    dense, dmask, _ = _fwd_launch(FWD, d0, c, c.dense(mode), c.size, None, 0, with_mask=True)
    if row.op == FWD:
        pre, mag = (t[rows].reshape(-1, Cout) for t in c.forward_all)
        _check_forward(out, pre, mag, 3 * K * K * Cin, 1, f"forward ({mode})")
        again, amask, _ = _fwd_launch(FWD, d, c, src, c.pitch, index, offset, with_mask=True)
        assert torch.equal(_bits(out), _bits(again)) and torch.equal(mask, amask), "two launches differ"
        assert torch.equal(_bits(out), _bits(dense)) and torch.equal(mask, dmask), "the result depends on the addressing"
    else:
        tol = _wgrad_tol(row.n * c.OH * c.OW)
        dw, db = _wgrad_launch(WGRAD, d, c, src, c.pitch, index, offset, mask=mask)
        sg = signs.view(c.n, c.OH, c.OW, Cout).permute(0, 3, 1, 2).cpu()
        gw, gb = c.grads(mode, c.dy * sg)
        _maxnorm(dw.cpu().double(), gw, tol, f"weight gradient ({mode})")
        _maxnorm(db.cpu().double(), gb, tol, f"bias gradient ({mode})")
        dw2, db2 = _wgrad_launch(WGRAD, d, c, src, c.pitch, index, offset, mask=mask)
        assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(db), _bits(db2)), "two launches differ"
        dwd, dbd = _wgrad_launch(WGRAD, d0, c, c.dense(mode), c.size, None, 0, mask=dmask)
        assert torch.equal(_bits(dw), _bits(dwd)) and torch.equal(_bits(db), _bits(dbd)), "the result depends on the addressing"
    assert torch.equal(_bits(src), _bits(pristine)), "the launch wrote into its input"


def test_part_a_walks_the_ledger():
    """every row whose entry point takes (index, offset, traj_T, in_sample_stride) is run in every mode"""
    assert {r.id for r, _ in A_PARAMS} == {r.id for r in LEDGER if r.op not in (DGRAD, FWD_T)}
    assert all(sum(1 for r, m in A_PARAMS if r.id == row.id) == len(MODES) for row in A_ROWS)
    assert {(r.op, r.mean) for r in MASK_ROWS} == {(FWD, 3.0), (WGRAD, 3.0), (WGRAD, 0.0)}


# ================================================================================================ Part B: fallbacks
# id, the plan's predicates the case breaks, op, format, geometry, n, mean, act, the operand fact broken, the kernel the plan
# then selects (csrc/sf_nn.hip; the aligned launch runs the kernel the ledger pins for this geometry and n).
#   in      the activation base one element past its grid (f32: 4 bytes off 16; u8: 1 byte off 4)
#   stride  in_sample_stride = sample size + 1 (stride % 4 == 1), the base aligned
#   w / dout / out / mu / rstd   that operand 4 bytes off 16
#   index   a (monotone) index instead of NULL;  traj  traj_T = n + 1 (every sample stays in its place)
B = namedtuple("B", "id preds op fmt geom n mean act broken kernel")
NATURE24, SPLITK = (4, 84, 84, 24, 8, 4), (3136, 1, 1, 136, 1, 1)
B_CASES = [
    # ---- plan_conv_fwd: act_aligned / aligned(o.w) -> MODE_GENERIC; in4 gates the conv1 strip, bf16 and whole-line kernels
    B("fwd-f32-in", ("act_aligned",), FWD, F32, (16, 11, 13, 48, 3, 2), 37, 0.0, 1, "in", "k_conv_fwd<128, 64, 2, 2, 2>"),
    B("fwd-f32-stride", ("act_aligned",), FWD, F32, (4, 9, 9, 8, 3, 1), 3, 0.0, 1, "stride", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwd-f32f-in", ("act_aligned",), FWD, F32F, (3, 36, 36, 16, 8, 4), 5, 1.5, 1, "in", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwd-f32-w", ("aligned(o.w)",), FWD, F32, (16, 11, 13, 48, 3, 2), 37, 0.0, 1, "w", "k_conv_fwd<128, 64, 2, 2, 2>"),
    B("fwd-conv1-wide-in", ("act_aligned", "in4"), FWD, U8, NATURE1, 257, 3.0, 1, "in", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwd-conv1-wide-w", ("aligned(o.w)",), FWD, U8, NATURE1, 257, 0.0, 0, "w", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwd-conv1-bf16-stride", ("act_aligned", "in4"), FWD, U8, NATURE24, 257, 3.0, 1, "stride", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwd-conv1-strip-in", ("act_aligned", "in4"), FWD, U8, NATURE24, 257, 1.5, 1, "in", "k_conv_fwd<128, 32, 4, 1, 2>"),
    # aligned(o.out): the whole-line-store kernel needs it; otherwise k_conv1_u8_bf16 at Cout == 32 (the ledger: Cout == 24)
    B("fwd-conv1-out-m3", ("aligned(o.out)",), FWD, U8, NATURE1, 257, 3.0, 1, "out", "k_conv1_u8_bf16<true>"),
    B("fwd-conv1-out-m0", ("aligned(o.out)",), FWD, U8, NATURE1, 257, 0.0, 0, "out", "k_conv1_u8_bf16<false>"),
    # tabs16 gates the normalising strip kernel (and, through act_aligned, the vector loaders of MODE 4 / 5)
    B("fwdnorm-conv1-mu", ("tabs16", "act_aligned"), FWD_NORM, U8, NATURE1, 77, 3.0, 1, "mu", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwdnorm-conv1-rstd", ("tabs16", "act_aligned"), FWD_NORM, U8, NATURE1, 77, 3.0, 1, "rstd", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwdnorm-conv1-in", ("in4", "act_aligned"), FWD_NORM, U8, NATURE1, 77, 3.0, 1, "in", "k_conv_fwd<128, 32, 4, 1, 2>"),
    B("fwdnorm-f32f-mu", ("act_aligned",), FWD_NORM, F32F, (3, 36, 36, 16, 8, 4), 5, 1.5, 0, "mu", "k_conv_fwd<128, 32, 4, 1, 2>"),
    # ---- plan_conv_wgrad: act_aligned / aligned(o.dout) -> MODE_GENERIC; strip_ops gates the three conv1 strip kernels
    B("wgrad-f32-in", ("act_aligned",), WGRAD, F32, (16, 11, 13, 48, 3, 2), 37, 0.0, 0, "in", "k_conv_wgrad<64, 2, 2, 2>"),
    B("wgrad-conv1-bf16-in", ("act_aligned", "in4"), WGRAD, U8, NATURE1, 257, 3.0, 0, "in", "k_conv_wgrad<32, 4, 1, 2>"),
    B("wgrad-conv1-strip-stride", ("act_aligned", "in4"), WGRAD, U8, NATURE1, 257, 1.5, 0, "stride", "k_conv_wgrad<32, 4, 1, 2>"),
    B("wgrad-conv1-bf16-dout", ("aligned(o.dout)",), WGRAD, U8, NATURE1, 257, 0.0, 0, "dout", "k_conv_wgrad<32, 4, 1, 2>"),
    B("wgradnorm-conv1-rstd", ("tabs16", "act_aligned"), WGRAD_NORM, U8, NATURE1, 77, 3.0, 0, "rstd", "k_conv_wgrad<32, 4, 1, 2>"),
    B("wgradnorm-conv1-dout", ("aligned(o.dout)",), WGRAD_NORM, U8, NATURE1, 77, 3.0, 0, "dout", "k_conv_wgrad<32, 4, 1, 2>"),
    B("wgrad-conv2-dout", ("aligned(o.dout)",), WGRAD, F32, CONV2, 513, 0.0, 0, "dout", "k_conv_wgrad<64, 2, 2, 2>"),
    B("wgrad-conv3-dout", ("aligned(o.dout)",), WGRAD, F32, CONV3, 513, 0.0, 0, "dout", "k_conv_wgrad<64, 2, 2, 2>"),
    B("wgrad-glds-dout", ("aligned(o.dout)",), WGRAD, F32, (4, 20, 20, 128, 4, 2), 810, 0.0, 0, "dout", "k_conv_wgrad<64, 2, 2, 2>"),
    # !o.index excludes k_linear_wgrad_small, k_wgrad_img and k_wgrad_glds(_z); the last two also need traj_T == 0
    B("wgrad-conv2-index", ("o.index",), WGRAD, F32, CONV2, 513, 0.0, 0, "index", "k_conv_wgrad<64, 2, 2, 0>"),
    B("wgrad-conv3-index", ("o.index",), WGRAD, F32, CONV3, 513, 0.0, 0, "index", "k_conv_wgrad<64, 2, 2, 0>"),
    B("wgrad-small-index", ("o.index",), WGRAD, F32, (27, 1, 1, 17, 1, 1), 1001, 0.0, 0, "index", "k_conv_wgrad<32, 4, 1, 2>"),
    B("wgrad-glds_z-index", ("o.index",), WGRAD, F32, (64, 1, 1, 520, 1, 1), 16399, 0.0, 0, "index", "k_conv_wgrad<64, 2, 2, 0>"),
    B("wgrad-glds-traj", ("traj_T == 0",), WGRAD, F32, (4, 20, 20, 128, 4, 2), 810, 0.0, 0, "traj", "k_conv_wgrad<64, 2, 2, 0>"),
    B("wgrad-conv3-traj", ("traj_T == 0",), WGRAD, F32, CONV3, 513, 0.0, 0, "traj", "k_conv_wgrad<64, 2, 2, 0>"),
    B("wgrad-small-traj", ("traj_T == 0",), WGRAD, F32, (27, 1, 1, 17, 1, 1), 1001, 0.0, 0, "traj", "k_conv_wgrad<32, 4, 1, 2>"),
    # ---- plan_conv_dgrad: al16 gates both linear LDS-DMA forms and, through vec, the pixel-major and row-walking kernels
    B("dgrad-pix256-dout", ("al16",), DGRAD, F32, (16, 9, 9, 32, 3, 1), 1025, 0.0, 1, "dout", "k_conv_dgrad<128, 32, 4, 1, false>"),
    B("dgrad-pix256z-w", ("al16",), DGRAD, F32, (16, 9, 9, 64, 3, 1), 1025, 0.0, 1, "w", "k_conv_dgrad<128, 32, 4, 1, false>"),
    B("dgrad-pix128-w", ("al16",), DGRAD, F32, (40, 6, 6, 96, 3, 1), 1025, 0.0, 1, "w", "k_conv_dgrad<64, 64, 2, 2, false>"),
    B("dgrad-pix128z-dout", ("al16",), DGRAD, F32, (40, 6, 6, 64, 3, 1), 1025, 0.0, 1, "dout", "k_conv_dgrad<64, 64, 2, 2, false>"),
    B("dgrad-quadrow-dout", ("al16",), DGRAD, F32, (20, 10, 14, 96, 4, 2), 1025, 0.0, 1, "dout", "k_conv_dgrad<128, 32, 4, 1, false>"),
    B("dgrad-quadrowz-w", ("al16",), DGRAD, F32, (20, 10, 14, 64, 4, 2), 1025, 0.0, 1, "w", "k_conv_dgrad<128, 32, 4, 1, false>"),
    B("dgrad-linear128-dout", ("al16",), DGRAD, F32, (136, 1, 1, 96, 1, 1), 32700, 0.0, 1, "dout", "k_conv_dgrad<64, 64, 2, 2, false>"),
    B("dgrad-linear64-w", ("al16",), DGRAD, F32, (64, 1, 1, 544, 1, 1), 8193, 0.0, 1, "w", "k_conv_dgrad<64, 64, 2, 2, false>"),
]
# ws_floats (plan_fwd): test_split_k_workspace_threshold, on the ledger's split-K row
B_SPECIAL = {"ws_floats": "test_split_k_workspace_threshold"}


@functools.lru_cache(maxsize=1)
def _dense_case(fmt, geom, n, mean, norm):
    return Case(fmt, geom, n, mean, norm)


def _broken_operands(case, c, d):
    """the ledger case's operands with exactly one fact broken -> dict of launch arguments + [(tensor, pristine copy)]"""
    n, size = case.n, c.stride
    a = dict(src=c.x_dev.reshape(n, size), stride=size, index=None, w=c.wk, dy=c.dy_dev if case.op != FWD else None, mu=c.mu,
             rstd=c.rstd, out_off=0)
    if case.op in (FWD, FWD_NORM):
        a["dy"] = None
    kind = case.broken
    if kind == "in":
        a["src"] = _off_grid(a["src"])
    elif kind == "stride":
        pitched = torch.full((n, size + 1), 255 if case.fmt == U8 else NAN, dtype=c.x_dev.dtype, device="cuda")
        pitched[:, :size] = a["src"]
        a["src"], a["stride"] = pitched, size + 1
        assert a["stride"] % 4 == 1
    elif kind == "w":
        a["w"] = _off_grid(c.wk)
    elif kind == "dout":
        a["dy"] = _off_grid(c.dy_dev)
    elif kind in ("mu", "rstd"):
        a[kind] = _off_grid(getattr(c, kind))
    elif kind == "out":
        a["out_off"] = 1
    elif kind == "index":
        a["index"] = torch.arange(n, dtype=torch.int32, device="cuda")
    elif kind == "traj":
        d.traj_T = n + 1  # d + d / traj_T == d for every sample of the launch
    else:
        raise AssertionError(kind)
    a["kept"] = [(t, t.clone()) for t in (a["src"], a["w"], a["dy"], a["mu"], a["rstd"]) if t is not None]
    return a


class _View:
    """what the launch helpers read of a case: the ledger Case under the names of SlabCase"""

    def __init__(self, c, n):
        self.n, self.OH, self.OW, self.wk, self.b_dev, self.mu, self.rstd, self.dy_dev = n, c.OH, c.OW, c.wk, c.b_dev, c.mu, \
            c.rstd, None


@pytest.mark.parametrize("case", B_CASES, ids=[b.id for b in B_CASES])
def test_fallback(case):
    Cin, H, W, Cout, K, S = case.geom
    d = make_desc(case.fmt, case.geom, case.mean, case.act)
    if case.op >= FWD_NORM and not lib.conv_norm_supported(case.n, d):
        assert not DEFAULT_SWITCHES
        pytest.skip("the switch under test turns the normalising entry points off")
    if DEFAULT_SWITCHES:  # the aligned launch runs a ledger kernel other than the fallback
        aligned_name = lib.conv_kernel_name(case.op, case.n, d)
        assert aligned_name != case.kernel and any(r.op == case.op and r.name == aligned_name for r in LEDGER), aligned_name
    c = _dense_case(case.fmt, case.geom, case.n, case.mean, case.op >= FWD_NORM)
    a = _broken_operands(case, c, d)
    v = _View(c, case.n)
    if case.op in (FWD, FWD_NORM):
        with_mask = case.broken == "out" and bool(lib.conv_relu_mask_supported(case.n, d))
        run = lambda m: _fwd_launch(case.op, d, v, a["src"], a["stride"], a["index"], 0, w=a["w"], mu=a["mu"], rstd=a["rstd"],  # noqa: E731
                                    out_off=a["out_off"], with_mask=m)
        out, _, _ = run(False)
        pre, mag = c.forward
        bf16 = case.kernel.startswith("k_conv1_u8_bf16")
        rel, ratio = _check_forward(out, pre, mag, (3 if bf16 else 1) * K * K * Cin, case.act, "forward")
        print(f"fallback {case.id} -> {case.kernel}: max|err|/max|ref| {rel:.3g} max(err/bound) {ratio:.3g}")
        assert torch.equal(_bits(out), _bits(run(False)[0])), "two launches differ: the summation order is not fixed"
        if with_mask:  # the sign-bit form on the same kernel: same bytes, words = the signs
            mout, mask, _ = run(True)
            assert torch.equal(_bits(out), _bits(mout))
            signs = ((mask.view(-1, 1) >> torch.arange(32, device="cuda", dtype=torch.int32)) & 1).bool()
            assert torch.equal(signs, mout > 0), "the sign-bit words are not the signs of the output"
    elif case.op in (WGRAD, WGRAD_NORM):
        tol = _wgrad_tol(case.n * c.OH * c.OW)
        run = lambda: _wgrad_launch(case.op, d, v, a["src"], a["stride"], a["index"], 0, dy=a["dy"], mu=a["mu"], rstd=a["rstd"])  # noqa: E731
        dw, db = run()
        gw, gb, _, _ = c.grads
        rw, rb = _maxnorm(dw.cpu().double(), gw, tol, "weight gradient"), _maxnorm(db.cpu().double(), gb, tol, "bias gradient")
        print(f"fallback {case.id} -> {case.kernel}: dw {rw:.3g} db {rb:.3g}")
        dw2, db2 = run()
        assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(db), _bits(db2)), "two launches differ"
    else:
        _, _, gx, gmag = c.grads
        mask = (c.x > 0).permute(0, 2, 3, 1)
        for act, ref, mag, what in ((c.x_dev, gx * mask, gmag * mask, "dgrad"), (None, gx, gmag, "dgrad nomask")):
            def run():
                din = Carved(case.n * H * W * Cin)
                lib.conv_dgrad(a["dy"], a["w"], act, din.t.view(case.n, H, W, Cin), case.n, d)
                torch.cuda.synchronize()
                assert din.intact(), "the data gradient wrote outside din"
                return din.t.view(case.n, H, W, Cin)

            din = run()
            got = din.cpu().double()
            rel = _maxnorm(got, ref, 3e-5, what)
            ratio = _elementwise(got, ref, mag, K * K * Cout, what)
            print(f"fallback {case.id} -> {case.kernel} {what}: max|err|/max|ref| {rel:.3g} max(err/bound) {ratio:.3g}")
            assert torch.equal(_bits(din), _bits(run())), "two launches differ: the summation order is not fixed"
    for t, pristine in a["kept"]:
        assert torch.equal(_bits(t), _bits(pristine)), "the launch wrote into an input"


def test_split_k_workspace_threshold():
    """plan_fwd splits along K only if the workspace holds splits * Mtot * N floats: sf_conv_fwd_workspace's own answer (less
    its 256 bytes of slack) is enough, one float fewer is not, and then the same geometry runs unsplit
    (k_conv_fwd<128, 64, 2, 2, 0>, one slice, no k_splitk_finish).  A split launch leaves its partial sums in the workspace, an
    unsplit one does not touch it; both are held to the ledger's bounds."""
    row = next(r for r in LEDGER if r.op == FWD and r.geom == SPLITK)
    Cin, H, W, Cout, K, S = row.geom
    d = make_desc(row.fmt, row.geom, row.mean, row.act)
    c = _dense_case(row.fmt, row.geom, row.n, row.mean, False)
    v = _View(c, row.n)
    queried = lib.conv_fwd_workspace(row.n, d)
    assert queried > 256, "the ledger's split-K row is split"
    need = queried - 256  # bytes of the partial sums the plan asks for
    assert need % (4 * row.n * Cout) == 0 and need // (4 * row.n * Cout) > 1  # a whole number of slices
    pre, mag = c.forward
    outs = {}
    for what, nbytes, split in (("queried", queried, True), ("exact", need, True), ("one float short", need - 4, False)):
        out, _, ws = _fwd_launch(FWD, d, v, c.x_dev, c.stride, None, 0, ws_bytes=nbytes)
        rel, ratio = _check_forward(out, pre, mag, Cin, row.act, f"forward, workspace {what}")
        written = bool((ws.t.view(torch.float32)[:nbytes // 4] != 7.0).any())
        print(f"split-K workspace {what} ({nbytes} bytes): written {written} max|err|/max|ref| {rel:.3g} max(err/bound) {ratio:.3g}")
        assert written == split, f"workspace {what}: the launch {'did not split' if split else 'split'}"
        again, _, _ = _fwd_launch(FWD, d, v, c.x_dev, c.stride, None, 0, ws_bytes=nbytes)
        assert torch.equal(_bits(out), _bits(again)), "two launches differ: the summation order is not fixed"
        outs[what] = out
    assert torch.equal(_bits(outs["queried"]), _bits(outs["exact"]))


# ================================================================================================ refusals
def _refused(call, *outs):
    with pytest.raises(lib.SfHipError):
        call()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "a refused launch wrote into its output"


def test_refusals_leave_the_output_alone():
    """the entry points that refuse a misaligned operand instead of falling back: sf_conv_fwd_t (16-byte input and weights,
    stride % 4, its split-K workspace), sf_conv_fwd_t_os / _os2 (input, weights, first-segment output), the sign-bit forms
    (sf_conv_fwd_relu_mask: frames 4-byte aligned, stride % 4, weights through the plan; sf_conv_wgrad_relu_mask: words 8-byte
    aligned, dY 16-byte aligned) and the 16-byte workspaces of sf_conv_fwd / sf_conv_wgrad.  (sf_conv_fwd_t_os2's dense output
    segment: tests/test_gpu_fwd_two_segment.py test_refusals.)"""
    n = 513
    d = make_desc(F32, CONV3, 0.0, 1)
    c = _dense_case(F32, CONV3, n, 0.0, False)
    M, size, L = n * c.OH * c.OW, c.stride, c.OH * c.OW * d.Cout
    x, wt = c.x_dev.reshape(n, size), c.wk.t().contiguous()
    out = Carved(M * d.Cout)
    o2 = out.t.view(M, d.Cout)
    _refused(lambda: lib.conv_fwd_t(_off_grid(x), size, wt, c.b_dev, o2, n, d), out)
    _refused(lambda: lib.conv_fwd_t(x, size, _off_grid(wt), c.b_dev, o2, n, d), out)
    _refused(lambda: lib.conv_fwd_t(x, size + 1, wt, c.b_dev, o2, n - 1, d), out)
    strided = Carved(n * 2 * L)
    s2 = strided.t.view(n, 2, L)
    if lib.conv_fwd_os_supported("fwd_t", n, d, size, 2 * L):
        _refused(lambda: lib.conv_fwd_t_os(_off_grid(x), size, wt, c.b_dev, s2[:, 1], 2 * L, n, d), strided)
        _refused(lambda: lib.conv_fwd_t_os(x, size, _off_grid(wt), c.b_dev, s2[:, 1], 2 * L, n, d), strided)
        _refused(lambda: lib.conv_fwd_t_os(x, size, wt, c.b_dev, strided.t[1:].view(-1)[:(n - 1) * 2 * L].view(n - 1, 2, L)[:, 0],
                                           2 * L, n - 1, d), strided)
        dense2 = Carved((n - 100) * L)
        _refused(lambda: lib.conv_fwd_t_os2(s2[:100, 1], 2 * L, _off_grid(x[100:]), wt, c.b_dev, s2[:100, 1], 2 * L,
                                            dense2.t.view(n - 100, L), 100, n, d), strided, dense2)
    # sf_conv_fwd_t's split-K workspace: 16-byte aligned and large enough
    ds = make_desc(F32, SPLITK, 0.0, 1)
    ns = next(m for m in (130, 257, 513, 1025, 2049) if lib.conv_fwd_t_workspace(m, ds))
    cs = Case(F32, SPLITK, ns, 0.0, False)
    wsb, wts = lib.conv_fwd_t_workspace(ns, ds), cs.wk.t().contiguous()
    ws = torch.empty(wsb + 16, dtype=torch.uint8, device="cuda")
    outs = Carved(ns * ds.Cout)
    _refused(lambda: lib.conv_fwd_t(cs.x_dev, cs.stride, wts, cs.b_dev, outs.t.view(ns, -1), ns, ds, ws[4:4 + wsb]), outs)
    _refused(lambda: lib.conv_fwd_t(cs.x_dev, cs.stride, wts, cs.b_dev, outs.t.view(ns, -1), ns, ds, ws[:wsb - 256 - 4]), outs)
    # ... and the workspaces of sf_conv_fwd / sf_conv_wgrad
    fb = lib.conv_fwd_workspace(ns, ds)
    fws = torch.empty(max(fb, 256) + 16, dtype=torch.uint8, device="cuda")
    _refused(lambda: lib.conv_fwd(cs.x_dev, cs.stride, None, 0, cs.wk, cs.b_dev, outs.t.view(ns, -1), ns, ds, fws[4:]), outs)
    K = d.KH * d.KW * d.Cin
    dw, db = Carved(K * d.Cout), Carved(d.Cout)
    gws = torch.empty(lib.conv_wgrad_workspace(n, d) + 16, dtype=torch.uint8, device="cuda")
    _refused(lambda: lib.conv_wgrad(x, size, None, 0, c.dy_dev, dw.t.view(K, -1), db.t, n, d, gws[4:]), dw, db)
    # the sign-bit forms at the Nature conv1
    n1 = 257
    d1 = make_desc(U8, NATURE1, 3.0, 1)
    if not lib.conv_relu_mask_supported(n1, d1):
        assert not DEFAULT_SWITCHES
        return
    c1 = _dense_case(U8, NATURE1, n1, 3.0, False)
    M1, s1 = n1 * c1.OH * c1.OW, c1.stride
    x1 = c1.x_dev.reshape(n1, s1)
    out1, words = Carved(M1 * 32), Carved(M1 + 2)
    o1, wd = out1.t.view(M1, 32), words.t.view(torch.int32)
    pitched = torch.zeros((n1, s1 + 1), dtype=torch.uint8, device="cuda")
    _refused(lambda: lib.conv_fwd_relu_mask(_off_grid(x1), s1, None, 0, c1.wk, c1.b_dev, o1, wd[:M1], n1, d1), out1, words)
    _refused(lambda: lib.conv_fwd_relu_mask(pitched, s1 + 1, None, 0, c1.wk, c1.b_dev, o1, wd[:M1], n1, d1), out1, words)
    _refused(lambda: lib.conv_fwd_relu_mask(x1, s1, None, 0, _off_grid(c1.wk), c1.b_dev, o1, wd[:M1], n1, d1), out1, words)
    K1 = 256
    dw1, db1 = Carved(K1 * 32), Carved(32)
    ws1 = torch.empty(lib.conv_wgrad_workspace(n1, d1), dtype=torch.uint8, device="cuda")
    good = torch.zeros(M1 + 2, dtype=torch.int32, device="cuda")
    assert good.data_ptr() % 8 == 0
    args = lambda xin, st, dy, mk: (xin, st, None, 0, dy, mk, dw1.t.view(K1, 32), db1.t, n1, d1, ws1)  # noqa: E731
    _refused(lambda: lib.conv_wgrad_relu_mask(*args(x1, s1, c1.dy_dev, good[1:1 + M1])), dw1, db1)       # words 4 bytes off 8
    _refused(lambda: lib.conv_wgrad_relu_mask(*args(x1, s1, _off_grid(c1.dy_dev), good[:M1])), dw1, db1)  # dY 4 bytes off 16
    _refused(lambda: lib.conv_wgrad_relu_mask(*args(_off_grid(x1), s1, c1.dy_dev, good[:M1])), dw1, db1)  # frames 1 byte off
    _refused(lambda: lib.conv_wgrad_relu_mask(*args(pitched, s1 + 1, c1.dy_dev, good[:M1])), dw1, db1)    # stride % 4 == 1
    lib.conv_wgrad_relu_mask(*args(x1, s1, c1.dy_dev, good[:M1]))  # and the aligned call is taken
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw1.t).all()) and dw1.intact() and db1.intact()


# ================================================================================================ Part C: the roster
# the operand predicates of plan_conv_fwd, plan_conv_wgrad and plan_conv_dgrad (csrc/sf_nn.hip), as the plans spell them
OPERAND_PREDICATES = ["act_aligned", "aligned(o.w)", "aligned(o.dout)", "aligned(o.out)", "in4", "tabs16", "o.index",
                      "traj_T == 0", "ws_floats", "al16"]


def test_every_operand_branch_has_a_case():
    """a plain table check: every predicate has a Part B case, every case names predicates of the list, ids are unique"""
    covered = {p for b in B_CASES for p in b.preds} | set(B_SPECIAL)
    assert covered == set(OPERAND_PREDICATES), set(OPERAND_PREDICATES) ^ covered
    assert all(name in globals() for name in B_SPECIAL.values())
    assert len({b.id for b in B_CASES}) == len(B_CASES)
    assert all(b.kernel.startswith(("k_conv_fwd<", "k_conv_wgrad<", "k_conv_dgrad<", "k_conv1_u8_bf16<")) for b in B_CASES)
    # each of the three plans has its fallbacks covered, and every broken fact of the issue's list appears
    assert {b.op for b in B_CASES} == {FWD, FWD_NORM, WGRAD, WGRAD_NORM, DGRAD}
    assert {b.broken for b in B_CASES} == {"in", "stride", "w", "dout", "out", "mu", "rstd", "index", "traj"}
