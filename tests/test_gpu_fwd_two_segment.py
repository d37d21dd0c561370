"""The two-segment forwards (sf_conv_fwd_relu_mask_os2, sf_conv_fwd_t_os2): of a rollout launch of n samples
only the first keep_n belong to the learner's first minibatch.  Samples s < keep_n are written into slot SLOT of a kept
[n, T, OH*OW*Cout] buffer (and read from such a slot by the next layer), samples s >= keep_n are written densely to a second
buffer, counted from keep_n (and read densely from one), and leave no sign-bit words.

Per layer of the Nature CNN at the shapes tests/test_gpu_fwd_out_stride.py found critical (conv1 n = 258 / 259; conv2 n = 258:
20898 rows with a ragged last tile, n = 1620: 64-row tail tiles; conv3 n = 258 / 514), T = 3 slots, slot 1, every buffer and its
guard bands filled with NaN (-1 for the sign-bit words), keep_n in {0, 1, 100, n - 1, n} — at 100 the split is inside a 128-row
tile of conv2 (8100 rows) and inside a 4-row group of conv3 (4900 rows of 49-row samples):
  * kept slot of the samples below keep_n + dense rows from keep_n on == the dense entry point, byte for byte (compared, as in
    the out-stride test, with the head of the dense launch on the larger batch where the dense dispatch runs these kernels);
  * slots 0 and 2, the kept rows from keep_n on, every guard band and the sign-bit words from keep_n on still hold their fill;
  * every element that should be written is finite.
The fc layer (3136 -> 512) reads the two segments through k_fwd_glds_z_os<64, 64, 2, 2>; it is compared with the dense entry
point at the smallest n at which that runs k_fwd_glds_z<64, 64, 2, 2> unsplit (found from the library).
The fc reuse rests on the 64 x 64 and the 128 x 128 form of that kernel writing the same bytes: one launch of each, compared.
Chain: conv1 -> conv2 -> conv3 -> fc, each layer reading the two-segment output of the one before, n = 258, keep_n = 100.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_fwd_out_stride import DENSE_N, LAYERS, _batch, _dense, _desc  # noqa: E402
from tests.test_gpu_kernel_ledger import BAND, DEFAULT_SWITCHES, F32, Case, make_desc  # noqa: E402

T, SLOT = 3, 1
NAN = float("nan")
FC_GEOM = (3136, 1, 1, 512, 1, 1)
FC_DENSE, FC_TWIN = "k_fwd_glds_z<64, 64, 2, 2>", "k_fwd_glds_z_os<64, 64, 2, 2>"
CASES = [("conv1", 258), ("conv1", 259), ("conv2", 258), ("conv2", 1620), ("conv3", 258), ("conv3", 514)]


def _keeps(n):
    return [0, 1, 100, n - 1, n]


def _lens(d):
    return d.H * d.W * d.Cin, d.OH * d.OW * d.Cout, d.OH * d.OW


def _banded(rows, L, fill=NAN, dtype=torch.float32):
    """a filled buffer of `rows` rows of L elements between two guard bands -> (rows view [rows, L], flat incl. bands)"""
    flat = torch.full((rows * L + 2 * BAND,), fill, dtype=dtype, device="cuda")
    return flat[BAND:BAND + rows * L].view(rows, L), flat


def _bands_hold(flat, rows_elems, fill_is):
    return bool(fill_is(flat[:BAND]).all()) and bool(fill_is(flat[BAND + rows_elems:]).all())


class TwoSeg:
    """an activation in two segments: samples [0, kn) in slot SLOT of kept [n, T, L], samples [kn, n) in dense [n - kn, L]"""

    def __init__(self, n, kn, L, fill=NAN, dtype=torch.float32):
        self.n, self.kn, self.L = n, kn, L
        kept, self.kept_flat = _banded(n, T * L, fill, dtype)
        self.kept = kept.view(n, T, L)
        self.dense, self.dense_flat = _banded(max(n - kn, 1), L, fill, dtype)

    def fill_from(self, x):  # x: [n, L] dense
        self.kept[:self.kn, SLOT] = x[:self.kn]
        if self.kn < self.n:
            self.dense[:self.n - self.kn] = x[self.kn:self.n]

    def joined(self):
        return torch.cat([self.kept[:self.kn, SLOT], self.dense[:self.n - self.kn]], 0)

    def check_fill(self, fill_is, what):
        kn, n = self.kn, self.n
        assert bool(fill_is(self.kept[:, 0]).all()) and bool(fill_is(self.kept[:, 2]).all()), f"{what}: a neighbouring slot was written"
        assert bool(fill_is(self.kept[kn:, SLOT]).all()), f"{what}: kept rows at or beyond keep_n were written"
        assert _bands_hold(self.kept_flat, n * T * self.L, fill_is), f"{what}: a guard band of the kept buffer was written"
        assert _bands_hold(self.dense_flat, max(n - kn, 1) * self.L, fill_is), f"{what}: a guard band of the dense buffer was written"
        if kn == n:
            assert bool(fill_is(self.dense).all()), f"{what}: the dense buffer of an empty segment was written"


def _launch(layer_or_desc, c, n, kn, src, wt=None):
    """run the two-segment entry point of a layer -> (TwoSeg out, TwoSeg mask | None); src: the u8 frames (conv1) or a TwoSeg"""
    d = _desc(layer_or_desc) if isinstance(layer_or_desc, str) else layer_or_desc
    Lin, L, P = _lens(d)
    out = TwoSeg(n, kn, L)
    o1, o2 = out.kept[:kn, SLOT] if kn else None, out.dense if kn < n else None
    if d.in_u8:
        mk = TwoSeg(n, kn, P, -1, torch.int32)
        assert lib.conv_fwd_os2_supported("fwd", n, kn, d, c.stride, T * L)
        lib.conv_fwd_relu_mask_os2(src, c.stride, None, 0, c.wk, c.b_dev, o1 if kn else out.kept[:1, SLOT], T * L,
                                   mk.kept[:max(kn, 1), SLOT], T * P, o2, kn, n, d)
        torch.cuda.synchronize()
        return out, mk
    assert lib.conv_fwd_os2_supported("fwd_t", n, kn, d, T * Lin, T * L)
    i1, i2 = src.kept[:kn, SLOT] if kn else src.kept[:1, SLOT], src.dense if kn < n else None
    lib.conv_fwd_t_os2(i1, T * Lin, i2, wt if wt is not None else c.wk.t().contiguous(), c.b_dev,
                       o1 if kn else out.kept[:1, SLOT], T * L, o2, kn, n, d)
    torch.cuda.synchronize()
    return out, None


def _bytes_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(out, ref, what):
    got = out.joined()
    assert bool(torch.isfinite(got).all()), f"{what}: an element that should be written was not"
    assert _bytes_equal(got, ref), f"{what}: bytes differ from the dense entry point"
    out.check_fill(torch.isnan, what)


PARAMS = [(layer, n, kn) for layer, n in CASES for kn in _keeps(n)]


@pytest.mark.parametrize("layer,n,kn", PARAMS, ids=[f"{l}-n{n}-keep{k}" for l, n, k in PARAMS])
def test_two_segments_equal_dense(layer, n, kn):
    c, d = _batch(layer), _desc(layer)
    Lin, L, P = _lens(d)
    dense, dmask = _dense(layer, max(n, DENSE_N[layer]))
    if layer == "conv1":
        out, mk = _launch(layer, c, n, kn, c.x_dev)
        _check(out, dense[:n], f"{layer} n={n} keep_n={kn}")
        assert torch.equal(mk.kept[:kn, SLOT], dmask[:kn]), "sign-bit words of the kept samples differ"
        mk.check_fill(lambda t: t == -1, "sign-bit words")
        assert bool((mk.dense == -1).all()), "sign-bit words were stored beyond the split"
    else:
        src = TwoSeg(n, kn, Lin)
        src.fill_from(c.x_dev[:n].reshape(n, Lin))
        out, _ = _launch(layer, c, n, kn, src)
        _check(out, dense[:n], f"{layer} n={n} keep_n={kn}")


# ------------------------------------------------------------------------------------------------------------ fc
@functools.lru_cache(maxsize=1)
def _fc():
    """(desc, n_dense, case of n_dense samples, dense output): n_dense = the smallest multiple-of-64-plus-one n at which the
    dense entry point runs the rollout-size fc kernel unsplit"""
    d = make_desc(F32, FC_GEOM, 0.0, 1)
    n_dense = next(n for n in range(65, 16385, 64)
                   if lib.conv_kernel_name(3, n, d) == FC_DENSE and lib.conv_fwd_t_workspace(n, d) == 0)
    c = Case(F32, FC_GEOM, n_dense, 0.0, False)
    out = torch.full((n_dense, 512), NAN, device="cuda")
    lib.conv_fwd_t(c.x_dev, c.stride, c.wk.t().contiguous(), c.b_dev, out, n_dense, d)
    torch.cuda.synchronize()
    return d, n_dense, c, out


FC_PARAMS = [(258, k) for k in _keeps(258)] + [(300, 130)]  # (300, 130): both segments end in a ragged 64-row tile


@pytest.mark.parametrize("n,kn", FC_PARAMS, ids=[f"n{n}-keep{k}" for n, k in FC_PARAMS])
def test_fc_two_segments_equal_dense(n, kn):
    d, n_dense, c, dense = _fc()
    assert n <= n_dense
    src = TwoSeg(n, kn, 3136)
    src.fill_from(c.x_dev[:n].reshape(n, 3136))
    out, _ = _launch(d, c, n, kn, src)
    _check(out, dense[:n], f"fc n={n} keep_n={kn}")


def test_fc_tile_shapes_give_the_same_bytes():
    """the condition of the fc reuse (rollout_reuse.fc_reusable): the rollout-size fc kernel (64 x 64 tiles) and the training
    kernel (128 x 128 tiles), both unsplit, write the same bytes at K = 3136, N = 512.  One training-kernel launch at the
    smallest n at which the dense dispatch runs it unsplit (found from the library), its first rows against the rollout-size
    kernel on the same rows."""
    from sample_factory_amd.algo.learning.rollout_reuse import FC_SAME_BYTES_FORMS
    d = make_desc(F32, FC_GEOM, 0.0, 1)
    unsplit = lambda n, name: lib.conv_kernel_name(3, n, d) == name and lib.conv_fwd_t_workspace(n, d) == 0
    train = lib.conv_kernel_name(3, 32768, d)
    n_small = next(n for n in range(64, 32769, 64) if unsplit(n, FC_DENSE))
    n_big = next(n for n in range(n_small, 32769, 64) if unsplit(n, train))
    print(f"rollout-size kernel {FC_DENSE} at n = {n_small}, training kernel {train} at n = {n_big}")
    if DEFAULT_SWITCHES:
        assert (FC_DENSE, train) == FC_SAME_BYTES_FORMS
    g = torch.Generator(device="cuda").manual_seed(3136)
    x = torch.randn((n_big, 3136), device="cuda", generator=g)
    wt = torch.randn((512, 3136), device="cuda", generator=g) / 56.0
    b = torch.randn(512, device="cuda", generator=g) * 0.1
    small, big = torch.full((n_small, 512), NAN, device="cuda"), torch.full((n_big, 512), NAN, device="cuda")
    lib.conv_fwd_t(x, 3136, wt, b, small, n_small, d)
    lib.conv_fwd_t(x, 3136, wt, b, big, n_big, d)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(big).all()) and bool((small > 0).any()) and bool((small == 0).any())
    assert _bytes_equal(small, big[:n_small]), "the two tile shapes round differently: the fc output must not be reused"


def test_chain():
    """conv1 -> conv2 -> conv3 -> fc, every layer reading the two segments the one before wrote"""
    n, kn = 258, 100
    c1 = _batch("conv1")
    a, _ = _launch("conv1", c1, n, kn, c1.x_dev)
    x = _dense("conv1", max(n, DENSE_N["conv1"]))[0][:n]
    _check(a, x, "chain conv1")
    for layer in ("conv2", "conv3"):
        c, d = _batch(layer), _desc(layer)
        nd = max(n, DENSE_N[layer])
        # the dense chain: the dense entry point on the previous dense result (padded with the batch's own samples up to the
        # size at which the dense dispatch runs this kernel; a sample's result does not depend on the others)
        xin = torch.cat([x, c.x_dev[n:nd].reshape(nd - n, -1)], 0).contiguous()
        ref = torch.full((nd, _lens(d)[1]), NAN, device="cuda")
        lib.conv_fwd_t(xin, c.stride, c.wk.t().contiguous(), c.b_dev, ref, nd, d)
        a, _ = _launch(layer, c, n, kn, a)
        x = ref[:n]
        _check(a, x, f"chain {layer}")
    d, n_dense, c, _ = _fc()
    xin = torch.cat([x, c.x_dev[n:n_dense].reshape(n_dense - n, -1)], 0).contiguous()
    ref = torch.full((n_dense, 512), NAN, device="cuda")
    lib.conv_fwd_t(xin, c.stride, c.wk.t().contiguous(), c.b_dev, ref, n_dense, d)
    a, _ = _launch(d, c, n, kn, a)
    _check(a, ref[:n], "chain fc")


def test_kernel_names():
    """ops 6 and 7 name what they named before, the fc twin is named after its dense kernel, the dense names are unchanged"""
    from sample_factory_amd.algo.learning.rollout_reuse import twin_name
    d = make_desc(F32, FC_GEOM, 0.0, 1)
    assert twin_name(FC_DENSE) == FC_TWIN
    assert lib.conv_kernel_name(7, 258, d) == FC_TWIN and lib.conv_kernel_name(7, 4096, d) == FC_TWIN
    if not DEFAULT_SWITCHES:
        return
    assert lib.conv_kernel_name(3, 4096, d) == FC_DENSE and lib.conv_fwd_t_workspace(4096, d) == 0
    assert lib.conv_kernel_name(3, 32768, d) == "k_fwd_glds_z<128, 128, 2, 2>"
    for layer, (fmt, geom, dense, strided, _) in LAYERS.items():
        dl = _desc(layer)
        for n in (258, 4096):
            assert lib.conv_kernel_name(6 if layer == "conv1" else 7, n, dl) == strided
        for n in (4096, 32768):
            assert lib.conv_kernel_name(0 if layer == "conv1" else 3, n, dl) == dense


def test_refusals():
    """a split outside [0, n], a misaligned dense segment or a launch without a twin is refused, never run on another kernel"""
    d = _desc("conv2")
    Lin, L, _ = _lens(d)
    assert not lib.conv_fwd_os2_supported("fwd_t", 258, 259, d, T * Lin, T * L)
    assert not lib.conv_fwd_os2_supported("fwd_t", 258, -1, d, T * Lin, T * L)
    c = _batch("conv2")
    src, out = TwoSeg(258, 100, Lin), TwoSeg(258, 100, L)
    with pytest.raises(lib.SfHipError):
        lib.conv_fwd_t_os2(src.kept[:100, SLOT], T * Lin, src.dense, c.wk.t().contiguous(), c.b_dev, out.kept[:100, SLOT], T * L,
                           out.dense.view(-1)[1:], 100, 258, d)
