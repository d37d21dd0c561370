"""sf_frame_resize on the GPU against the NumPy model of its arithmetic (envs/frame_ops.py), BIT FOR BIT: both filters,
grey-scale on and off, channel-last and planar sources, every alignment class (dword loads / stores and their bytewise
fall-backs), strips, bands and sub-bands, the row loop, and the bytewise 64-bit path.  Every destination sits in a buffer of
canary bytes — before the first row, in the pitch padding between the rows and behind the last — that must stay untouched.
Integer arithmetic has no tolerance: every comparison is exact."""
import numpy as np
import pytest
import torch

from sample_factory_amd.envs import frame_ops

pytestmark = pytest.mark.gpu

CANARY = 0xA5
# (H, W) -> (OH, OW)
GEOMS = [((10, 7), (4, 3)),      # fractional on both axes, byte stores (OH OW = 12 but OW = 3: rows of 3 bytes)
         ((8, 12), (4, 4)),      # integer factors 2 and 3, dword stores
         ((21, 16), (8, 8)),
         ((5, 6), (5, 6)),       # identity: grey-scale / de-interleave alone
         ((97, 5), (3, 5)),      # one output row spans more source rows (33) than a band (32) holds
         ((4, 4), (9, 7)),       # nearest only: an up-scale
         ((210, 160), (84, 84))]  # the real case
CHANNELS = [(1, False), (3, False), (3, True), (4, False)]   # (C, grey)
# (dst offset into its buffer, dst pitch: None = tight | "slab", src offset, src pitch extra)
LAYOUTS = {"tight": (64, None, 0, 0), "slab": (64, "slab", 0, 16), "dst_plus_1": (65, None, 0, 0), "src_plus_1": (64, None, 1, 1)}


def _content(kind, shape, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "saturated":
        return np.full(shape, 255, np.uint8)
    # ties: image rows alternate 1, 0 (every 2-row box averages to exactly 1/2) — shape [rows, C, H, W]
    a = np.zeros(shape, np.uint8)
    a[:, :, 0::2, :] = 1
    return a


def _run(frames_chw, hwc, OH, OW, interp, gray, layout):
    """frames_chw: numpy [rows, C, H, W].  Lays the source and the destination out as `layout` says, launches, checks the
    destination rows against the model and every other byte of the destination buffer against the canary"""
    from sample_factory_amd import lib
    rows, Cn, H, W = frames_chw.shape
    dst_off, dst_pitch, src_off, src_extra = LAYOUTS[layout]
    native = np.ascontiguousarray(frames_chw.transpose(0, 2, 3, 1)) if hwc else frames_chw
    fb, cp = H * W * Cn, 1 if gray else Cn
    rb = cp * OH * OW
    dp = rb if dst_pitch is None else 3 * ((rb + 3) // 4 * 4) + 16   # a column of a slab with three more beside it
    sp = fb + src_extra
    src_flat = torch.full((src_off + rows * sp + 8,), 0x5A, dtype=torch.uint8)
    src_flat[src_off:src_off + rows * sp].view(rows, sp)[:, :fb] = torch.from_numpy(native.reshape(rows, fb))
    src_flat = src_flat.cuda()
    src = src_flat.as_strided((rows,) + native.shape[1:], (sp,) + tuple(int(s) for s in np.array(native.strides[1:])), src_off)
    dst_flat = torch.full((dst_off + rows * dp + 64,), CANARY, dtype=torch.uint8, device="cuda")
    dst = dst_flat.as_strided((rows, cp, OH, OW), (dp, OH * OW, OW, 1), dst_off)
    assert src.data_ptr() % 4 == src_off % 4 and dst.data_ptr() % 4 == dst_off % 4
    want = frame_ops.preprocess_frames(native, "hwc" if hwc else "chw", OH, OW, interp, gray)
    expect = np.full(dst_flat.numel(), CANARY, np.uint8)
    for b in range(rows):
        expect[dst_off + b * dp:dst_off + b * dp + rb] = want[b].reshape(-1)
    src_before = src_flat.clone()
    lib.frame_resize(dst, src, hwc, interp, gray)
    torch.cuda.synchronize()
    got = dst_flat.cpu().numpy()
    what = f"{(H, W)}->{(OH, OW)} C={Cn} gray={gray} hwc={hwc} {interp} {layout} rows={rows}"
    assert np.array_equal(dst.cpu().numpy(), want), "result differs from the model: " + what
    assert np.array_equal(got, expect), "bytes outside the destination rows changed: " + what
    assert torch.equal(src_flat, src_before), "the source changed: " + what


# (the area filter only shrinks: the up-scale is a nearest case)
CASES = [(g, i) for g in GEOMS for i in ("area", "nearest") if i == "nearest" or (g[1][0] <= g[0][0] and g[1][1] <= g[0][1])]


@pytest.mark.parametrize("hwc", [True, False], ids=["hwc", "chw"])
@pytest.mark.parametrize("cg", CHANNELS, ids=lambda cg: f"C{cg[0]}{'gray' if cg[1] else ''}")
@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}x{}_{}x{}_{}".format(*c[0][0], *c[0][1], c[1]))
def test_kernel_equals_the_numpy_model_bit_for_bit(case, cg, hwc):
    ((H, W), (OH, OW)), interp = case
    (Cn, gray) = cg
    rows = 3 if H == 210 else 5
    for layout in LAYOUTS:
        for kind in ("random", "zeros", "saturated", "ties"):
            if kind != "random" and layout not in ("tight", "src_plus_1"):
                continue
            _run(_content(kind, (rows, Cn, H, W), seed=H * W + Cn), hwc, OH, OW, interp, gray, layout)


@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("interp", ["area", "nearest"])
def test_row_counts_on_the_small_frame(interp, rows):
    for hwc, (Cn, gray) in ((True, (3, True)), (False, (3, False)), (True, (4, False))):
        for layout in ("tight", "slab"):
            _run(_content("random", (rows, Cn, 10, 7), seed=rows), hwc, 4, 3, interp, gray, layout)


def test_row_loop_past_the_grid():
    """65539 frames of 4 x 4 x 3 -> 2 x 2 grey: more rows than gridDim.y holds"""
    for interp in ("area", "nearest"):
        _run(_content("random", (65539, 3, 4, 4), seed=1), True, 2, 2, interp, True, "tight")


def test_tie_blocks_round_up():
    """2 x 2 boxes [1, 1, 0, 0] -> 1 and [0, 1, 0, 0] -> 0, on the device"""
    from sample_factory_amd import lib
    src = torch.tensor([[1, 1, 0, 1], [0, 0, 0, 0]], dtype=torch.uint8).view(1, 1, 2, 4).cuda()
    dst = torch.full((1, 1, 1, 2), 9, dtype=torch.uint8, device="cuda")
    lib.frame_resize(dst, src, False, "area", False)
    torch.cuda.synchronize()
    assert dst.flatten().tolist() == [1, 0]


@pytest.mark.parametrize("case", ["row_wider_than_the_band", "index_products_past_31_bits"])
def test_bytewise_wide_path(case):
    """frames the LDS kernel does not take: a source row above 32 KB, and W OW = 2^31"""
    from sample_factory_amd import lib
    rng = np.random.default_rng(5)
    if case == "row_wider_than_the_band":
        for hwc, (Cn, gray) in ((True, (3, True)), (False, (1, False))):
            _run(rng.integers(0, 256, (2, Cn, 3, 40000), dtype=np.uint8), hwc, 2, 100, "area", gray, "tight")
        return
    W, OW = 1 << 22, 512                      # an integer factor of 8192: the model is a block mean
    frame = rng.integers(0, 256, (1, 1, 1, W), dtype=np.uint8)
    src = torch.from_numpy(frame).cuda()
    dst = torch.zeros((1, 1, 1, OW), dtype=torch.uint8, device="cuda")
    lib.frame_resize(dst, src, False, "area", False)
    sums = frame.reshape(OW, W // OW).astype(np.int64).sum(1)
    assert np.array_equal(dst.cpu().numpy().reshape(-1), (2 * sums + W // OW) // (2 * (W // OW)))
    lib.frame_resize(dst, src, False, "nearest", False)
    assert np.array_equal(dst.cpu().numpy().reshape(-1), frame.reshape(-1)[::W // OW])


def test_write_into_the_last_slot_of_a_stacked_column_then_the_plain_stack():
    """what the runner does under --device_framestack=4: sf_frame_resize into the last slot of obs[:, t + 1], then
    framestack_step(frame=None) shifts the other slots over from obs[:, t] or refills them where the episode ended"""
    from sample_factory_amd import lib
    rows, k, T, (H, W), (OH, OW) = 6, 4, 2, (21, 16), (8, 8)
    rng = np.random.default_rng(11)
    slab = torch.from_numpy(rng.integers(0, 256, (rows, T + 1, k, OH, OW), dtype=np.uint8)).cuda()
    before = slab.cpu().numpy().copy()
    frames = rng.integers(0, 256, (rows, H, W, 3), dtype=np.uint8)
    term = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.bool).cuda()
    small = frame_ops.preprocess_frames(frames, "hwc", OH, OW, "area", True)          # [rows, 1, OH, OW]
    lib.frame_resize(slab[:, 2, k - 1:], torch.from_numpy(frames).cuda(), True, "area", True)
    lib.framestack_step(slab[:, 2], slab[:, 1], k, None, term, None)
    torch.cuda.synchronize()
    want = before.copy()
    for b in range(rows):
        want[b, 2] = small[b] if term[b] else np.concatenate([before[b, 1, 1:], small[b]])
    assert np.array_equal(slab.cpu().numpy(), want)


def test_binding_refuses_views_it_cannot_describe():
    from sample_factory_amd import lib
    src = torch.zeros((4, 10, 8, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((4, 1, 5, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.SfHipError, match="planes"):
        lib.frame_resize(dst, src, True, "area", False)             # 3 channels into one plane without grey
    with pytest.raises(lib.SfHipError, match="uint8"):
        lib.frame_resize(dst.float(), src.float(), True, "area", True)
    with pytest.raises(lib.SfHipError, match="interpolation"):
        lib.frame_resize(dst, src, True, "cubic", True)
    with pytest.raises(lib.SfHipError, match="contiguous blocks"):
        lib.frame_resize(dst, torch.zeros((4, 10, 8, 6), dtype=torch.uint8, device="cuda")[..., ::2], True, "area", True)
    with pytest.raises(lib.SfHipError, match="sf_frame_resize"):
        lib.frame_resize(torch.zeros((4, 1, 11, 4), dtype=torch.uint8, device="cuda"), src, True, "area", True)   # enlarges
    lib.frame_resize(dst[:0], src[:0], True, "area", True)          # no rows: nothing to do
