"""sf_hwc_to_chw against numpy.transpose and sf_framestack_step_hwc against a numpy model of FrameStack over an
auto-resetting env, on the GPU: u8 and f32, every alignment class (dwords, bytes), the channel counts with a register path
(1..4) and a generic one, the row loop past 65535, pitched slab columns, a misaligned source.  A transpose has no
tolerance: every comparison is exact.  The frame-stack result must also equal hwc_to_chw into a scratch buffer followed by
the existing framestack_step on that scratch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"u8": torch.uint8, "f32": torch.float32}
# (rows, H, W, C): odd H W = the byte path (u8); 8 x 12 = the dword path; 6 x 5 degenerate (C = 1: a row copy) and generic
# channel counts; 65539 rows = the row loop past the grid's 65535
SHAPES = [(3, 5, 7, 3), (2, 8, 12, 3), (2, 8, 12, 4), (2, 6, 5, 1), (2, 6, 5, 2), (2, 6, 5, 5), (65539, 2, 2, 3),
          (2, 4, 6, 5), (2, 4, 6, 8), (300, 84, 84, 1)]   # ... generic C on the dword path, and more than one block per row


def _frames(rows, H, W, C, dtype, seed):
    """[rows, H, W, C] with every bit pattern of the dtype in play (f32: raw bits, NaNs included: the compare is on bytes)"""
    gen = torch.Generator().manual_seed(seed)
    es = torch.empty(0, dtype=dtype).element_size()
    return torch.randint(0, 256, (rows, H, W, C * es), dtype=torch.uint8, generator=gen).view(dtype).cuda()


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hwc_to_chw_matches_numpy_transpose(shape, dt):
    from sample_factory_amd import lib
    rows, H, W, C = shape
    src = _frames(rows, H, W, C, DTYPES[dt], seed=sum(shape))
    dst = torch.zeros((rows, C, H, W), dtype=DTYPES[dt], device="cuda")
    lib.hwc_to_chw(dst, src)
    torch.cuda.synchronize()
    want = np.ascontiguousarray(_bytes(src).cpu().numpy().reshape(rows, H, W, C, -1).transpose(0, 3, 1, 2, 4))
    assert _bytes(dst).cpu().numpy().tobytes() == want.tobytes()


def test_rows_zero():
    from sample_factory_amd import lib
    lib.hwc_to_chw(torch.zeros((0, 3, 4, 4), dtype=torch.uint8, device="cuda"),
                   torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device="cuda"))
    slab = torch.zeros((0, 2, 6, 4, 4), dtype=torch.uint8, device="cuda")
    lib.framestack_step_hwc(slab[:, 1], slab[:, 0], 2, torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("geom", [(8, 12, 3), (5, 7, 3), (8, 8, 4)], ids=lambda s: "x".join(map(str, s)))
def test_destination_is_a_pitched_slab_column_and_nothing_else_is_written(geom, dt):
    from sample_factory_amd import lib
    H, W, C = geom
    rows, T, t = 5, 3, 2
    src = _frames(rows, H, W, C, DTYPES[dt], seed=5)
    slab = _frames(rows, (T + 1) * C, H, W, DTYPES[dt], seed=6).view(rows, T + 1, C, H, W).contiguous()
    want = slab.clone()
    want[:, t] = src.permute(0, 3, 1, 2)
    lib.hwc_to_chw(slab[:, t], src)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(slab), _bytes(want))
    # the last C planes of a stacked column [rows, T + 1, 2 C, H, W]
    stacked = _frames(rows, (T + 1) * 2 * C, H, W, DTYPES[dt], seed=7).view(rows, T + 1, 2 * C, H, W).contiguous()
    want = stacked.clone()
    want[:, t, C:] = src.permute(0, 3, 1, 2)
    lib.hwc_to_chw(stacked[:, t, C:], src)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(stacked), _bytes(want))


@pytest.mark.parametrize("geom", [(8, 12, 3), (8, 12, 4), (6, 6, 2)], ids=lambda s: "x".join(map(str, s)))
def test_u8_source_offset_by_one_element_takes_the_byte_path(geom):
    """the source base leaves its dword alignment (and so does the pitch of the rows behind it)"""
    from sample_factory_amd import lib
    H, W, C = geom
    rows, fb = 7, H * W * C
    flat = torch.randint(0, 256, (1 + rows * (fb + 1),), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).cuda()
    src = flat[1:].view(rows, fb + 1)[:, :fb].view(rows, H, W, C)   # base + 1, pitch fb + 1
    assert src.data_ptr() % 4 == 1 and src[0].is_contiguous()
    dst = torch.zeros((rows, C, H, W), dtype=torch.uint8, device="cuda")
    lib.hwc_to_chw(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src.permute(0, 3, 1, 2))
    dst_flat = torch.full((3 + rows * fb,), 0xA5, dtype=torch.uint8, device="cuda")   # ... and a destination off by three
    dst2 = dst_flat[3:].view(rows, C, H, W)
    lib.hwc_to_chw(dst2, src)
    torch.cuda.synchronize()
    assert torch.equal(dst2, src.permute(0, 3, 1, 2)) and bool((dst_flat[:3] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ the frame stack
T, GUARD = 3, 64   # next / prev are columns 2 / 1 of a [rows, T + 1, k C, H, W] slab whose rows are GUARD bytes apart
FLAGS = ["none_done", "all_done", "random", "only_truncated", "truncated_pointer_only", "reset"]


def framestack_model(prev: np.ndarray, frame_chw: np.ndarray, k: int, done) -> np.ndarray:
    """gym.wrappers.FrameStack over an auto-resetting env: prev [rows, k, fb] bytes, frame_chw [rows, fb] bytes, done
    [rows] bool or None (= reset) -> next [rows, k, fb]"""
    out = np.empty_like(prev)
    for b in range(prev.shape[0]):
        if done is None or done[b]:
            out[b] = frame_chw[b][None]
        else:
            out[b, :k - 1], out[b, k - 1] = prev[b, 1:], frame_chw[b]
    return out


def _flags(kind, rows, gen):
    z = torch.zeros(rows, dtype=torch.bool)
    rnd = lambda: torch.rand(rows, generator=gen) < 0.3
    term, trunc = dict(none_done=(z, z), all_done=(~z, z), random=(rnd(), rnd()), only_truncated=(z, rnd()),
                       truncated_pointer_only=(None, rnd()), reset=(None, None))[kind]
    done = None if kind == "reset" else ((term if term is not None else z) | trunc).numpy()
    dev = lambda t: None if t is None else t.cuda()
    return dev(term), dev(trunc), done


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("geom", [(8, 12, 3), (5, 7, 3), (8, 8, 4), (6, 5, 5), (4, 8, 6), (2, 6, 3), (84, 84, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_framestack_step_hwc_matches_the_model_and_the_two_launch_route(geom, k, dt):
    from sample_factory_amd import lib
    H, W, C = geom
    dtype, rows = DTYPES[dt], 37
    es = torch.empty(0, dtype=dtype).element_size()
    fb = H * W * C * es
    row_bytes = (T + 1) * k * fb
    gen = torch.Generator().manual_seed(100 * k + H)
    flat0 = torch.randint(0, 256, (rows, row_bytes + GUARD), dtype=torch.uint8, generator=gen)
    flat0[:, row_bytes:] = 0xA5   # the guard pattern between the rows
    flat0 = flat0.cuda()

    def views(flat):
        body = flat[:, :row_bytes]
        return body.view(dtype).view(rows, T + 1, k * C, H, W), body.view(rows, T + 1, k, fb)

    for kind in FLAGS:
        term, trunc, done = _flags(kind, rows, gen)
        frame = _frames(rows, H, W, C, dtype, seed=int(gen.initial_seed()) + len(kind))
        frame0 = frame.clone()
        chw = np.ascontiguousarray(_bytes(frame).cpu().numpy().reshape(rows, H, W, C, es).transpose(0, 3, 1, 2, 4)).reshape(rows, fb)
        flat = flat0.clone()
        slab, slab_b = views(flat)
        expect = flat.clone()
        views(expect)[1][:, 2] = torch.from_numpy(framestack_model(slab_b[:, 1].cpu().numpy(), chw, k, done)).cuda()
        # the route the parent's entry points offer: transpose into a scratch frame, then the plain frame stack
        two = flat.clone()
        scratch = torch.zeros((rows, C, H, W), dtype=dtype, device="cuda")
        lib.hwc_to_chw(scratch, frame)
        lib.framestack_step(views(two)[0][:, 2], views(two)[0][:, 1], k, scratch, term, trunc)
        for launch in range(2):  # a second launch must give identical bits
            lib.framestack_step_hwc(slab[:, 2], slab[:, 1], k, frame, term, trunc)
            torch.cuda.synchronize()
            what = f"{geom} {dt} k={k} flags={kind} launch={launch}"
            assert torch.equal(views(flat)[1][:, 2], views(expect)[1][:, 2]), "next differs: " + what
            # everything else — prev, columns 0 and 3, the guard bytes between the rows — is untouched
            assert torch.equal(flat, expect), "bytes outside next changed: " + what
            assert torch.equal(_bytes(frame), _bytes(frame0)), "the frame buffer changed: " + what
        assert torch.equal(two, expect), f"hwc_to_chw + framestack_step differs: {geom} {dt} k={k} flags={kind}"


def test_framestack_step_hwc_row_loop_past_the_grid():
    from sample_factory_amd import lib
    rows, H, W, C, k = 65539, 2, 2, 3, 2
    gen = torch.Generator().manual_seed(3)
    slab = torch.randint(0, 256, (rows, 2, k * C, H, W), dtype=torch.uint8, generator=gen).cuda()
    frame = _frames(rows, H, W, C, torch.uint8, seed=4)
    term = (torch.rand(rows, generator=gen) < 0.5).cuda()
    want = torch.where(term[:, None, None, None], frame.permute(0, 3, 1, 2).repeat(1, k, 1, 1),
                       torch.cat([slab[:, 0, C:], frame.permute(0, 3, 1, 2)], 1))
    lib.framestack_step_hwc(slab[:, 1], slab[:, 0], k, frame, term, None)
    torch.cuda.synchronize()
    assert torch.equal(slab[:, 1], want)


def test_binding_refuses_what_is_not_a_channel_last_frame_beside_a_slab_column():
    from sample_factory_amd import lib
    slab = torch.zeros((4, T + 1, 12, 5, 6), dtype=torch.uint8, device="cuda")
    frame = torch.zeros((4, 5, 6, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.SfHipError, match="sf_framestack_step_hwc"):
        lib.framestack_step_hwc(slab[:, 2], slab[:, 2], 4, frame)                       # next is prev
    with pytest.raises(lib.SfHipError, match=r"\[rows, H, W, C\]"):
        lib.framestack_step_hwc(slab[:, 2], slab[:, 1], 4, frame.permute(0, 3, 1, 2))   # a CHW frame
    with pytest.raises(lib.SfHipError, match=r"\[rows, H, W, C\]"):
        lib.framestack_step_hwc(slab[:, 2], slab[:, 1], 3, frame)                       # 12 channels are not 3 x 3
    with pytest.raises(lib.SfHipError, match="mandatory"):
        lib.framestack_step_hwc(slab[:, 2], slab[:, 1], 4, None)
    with pytest.raises(lib.SfHipError, match="one dtype"):
        lib.hwc_to_chw(slab[:, 2, :3], frame.float())
    with pytest.raises(lib.SfHipError, match="one dtype"):
        lib.hwc_to_chw(slab[:, 2, :3].to(torch.int32), frame.to(torch.int32))
    with pytest.raises(lib.SfHipError, match="contiguous blocks"):
        lib.hwc_to_chw(slab[:, 2, :3], torch.zeros((4, 5, 6, 6), dtype=torch.uint8, device="cuda")[..., ::2])
    with pytest.raises(lib.SfHipError, match="device views"):
        lib.hwc_to_chw(slab[:, 2, :3], frame.cpu())
