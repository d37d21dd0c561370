"""sf_augment_gather on the GPU against the NumPy model (envs/frame_ops.py: augment_frames and its draws), BIT FOR BIT: the
shapes, source alignments and addressings of tests/test_gpu_augment_shift.py, with each op alone, each pair and all three;
cutout side ranges (1, 1), (2, 5) and (H + 3, H + 9) (the whole frame), both fills; intensity amplitudes 1, 64 and 255 on
frames that hold 0, 1, 127, 128, 254 and 255; guard bands around the destination; samples that take the strip and the
LDS-free paths; the pad-only launch against sf_random_shift_gather.  No tolerance: every comparison is exact."""
import numpy as np
import pytest
import torch

from sample_factory_amd.envs import frame_ops

pytestmark = pytest.mark.gpu

E, T = 6, 4            # the slab is [E, T + 1, C, H, W]: dataset row d of traj_T = T sits at slab row d + d // T
GUARD = 0xA5
EDGE_BYTES = (0, 1, 127, 128, 254, 255)


def _frames(shape, dtype, rows, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        a = rng.integers(0, 256, (rows,) + shape, dtype=np.uint8)
        flat = a.reshape(rows, -1)
        flat[:, :len(EDGE_BYTES)] = np.array(EDGE_BYTES, np.uint8)[:flat.shape[1]]  # the values the rounding turns on
        return a
    return rng.standard_normal((rows,) + shape).astype(np.float32)  # negative values too; none is subnormal


def _device_view(frames: np.ndarray, byte_offset: int, pitch_extra: int = 0):
    """the frames on the device as a view whose first byte sits `byte_offset` bytes behind an allocation's start and whose
    samples are S + pitch_extra elements apart -> (view of sample 0 onwards, sample stride in elements)"""
    rows, es = frames.shape[0], frames.itemsize
    S = int(np.prod(frames.shape[1:]))
    assert byte_offset % es == 0
    flat = torch.full((byte_offset // es + rows * (S + pitch_extra) + 4,), 77, dtype=torch.from_numpy(frames).dtype, device="cuda")
    body = flat[byte_offset // es:byte_offset // es + rows * (S + pitch_extra)].view(rows, S + pitch_extra)
    body[:, :S].copy_(torch.from_numpy(frames.reshape(rows, S)))
    return body, S + pitch_extra


def _rows_of(kind, n, recurrence, traj_T, rng):
    """(index tensor | None, offset, dataset rows int64 [n]) — the index is whole recurrence-long chunks in shuffled order
    with one chunk repeated"""
    nd = E * T if traj_T else E * (T + 1)
    if kind == "offset":
        offset = recurrence  # a chunk boundary that is not 0
        return None, offset, np.arange(offset, offset + n, dtype=np.int64)
    starts = rng.permutation(np.arange(0, nd - recurrence + 1, recurrence))
    starts = np.concatenate([starts[:2], starts[:1], starts[2:]])  # chunk 0 of the shuffle comes twice
    d = (starts[:, None] + np.arange(recurrence)[None, :]).reshape(-1)[:n]
    assert len(d) == n
    return torch.from_numpy(d.astype(np.int32)).cuda(), 0, d.astype(np.int64)


def _configs(shape, dtype):
    """each op alone, each pair, all three; the three side ranges; both fills (u8); the three amplitudes"""
    H = shape[1]
    fill = "random" if dtype == np.uint8 else "zero"
    return [dict(pad=4),
            dict(cutout=(2, 5)),
            dict(intensity=64),
            dict(pad=4, cutout=(1, 1), cutout_fill=fill),
            dict(pad=1, intensity=255),
            dict(cutout=(H + 3, H + 9), intensity=1),
            dict(pad=4, cutout=(2, 5), cutout_fill=fill, intensity=64),
            dict(cutout=(2, 5), cutout_fill=fill)]


def _expect(frames, d, traj_T, recurrence, seed, draw_id, ops):
    rows = d + d // traj_T if traj_T else d
    return frame_ops.augment_frames(frames[rows], seed, draw_id, d // recurrence, **ops)


def _launch_and_check(lib, frames, src, stride, shape, n, index, offset, d, traj_T, recurrence, seed, draw_id, ops, what):
    S = int(np.prod(shape))
    full = torch.full((n + 2, S + 5), GUARD, dtype=src.dtype, device="cuda")  # a guard row in front and behind, 5 elements
    dst = full[1:n + 1, :S]                                                    # behind every sample
    lib.augment_gather(dst, src, n, shape, sample_stride=stride, index=index, offset=offset, traj_T=traj_T,
                       recurrence=recurrence, seed=seed, draw_id=draw_id, **ops)
    got = full.cpu().numpy()
    want = _expect(frames, d, traj_T, recurrence, seed, draw_id, ops).reshape(n, S)
    assert np.array_equal(np.ascontiguousarray(got[1:n + 1, :S]).view(np.uint8), want.view(np.uint8)), what
    guard = np.full(1, GUARD, np.uint8).astype(got.dtype)[0]
    assert (got[0] == guard).all() and (got[n + 1] == guard).all() and (got[:, S:] == guard).all(), what
    return dst


def _sweep(shape, dtype, n, byte_offset=0, pitch_extra=0):
    from sample_factory_amd import lib
    frames = _frames(shape, dtype, E * (T + 1), sum(shape) + byte_offset)
    src, stride = _device_view(frames, byte_offset, pitch_extra)
    S = int(np.prod(shape))
    rng = np.random.default_rng(5)
    launches = 0
    for kind in ("index", "offset"):
        for traj_T in (T, 0):
            for recurrence in (1, 4):
                index, offset, d = _rows_of(kind, n, recurrence, traj_T, rng)
                for ops in _configs(shape, dtype):
                    for draw_id, seed in ((0, 12345), (7, 99)):
                        what = (shape, kind, traj_T, recurrence, ops, draw_id, seed, byte_offset)
                        dst = _launch_and_check(lib, frames, src, stride, shape, n, index, offset, d, traj_T, recurrence, seed,
                                                draw_id, ops, what)
                        launches += 1
                        if set(ops) == {"pad"}:  # the shift alone: the bytes of sf_random_shift_gather
                            old = torch.full((n, S), GUARD, dtype=src.dtype, device="cuda")
                            lib.random_shift_gather(old, src, n, shape, sample_stride=stride, index=index, offset=offset,
                                                    traj_T=traj_T, recurrence=recurrence, seed=seed, draw_id=draw_id, **ops)
                            assert torch.equal(dst.contiguous().view(torch.uint8), old.view(torch.uint8)), what
    return launches


def test_u8_3x5x7_nothing_aligned():
    assert _sweep((3, 5, 7), np.uint8, 8) == 128          # samples of 105 bytes


def test_u8_4x84x84():
    assert _sweep((4, 84, 84), np.uint8, 6) == 128


def test_u8_1x9x130_row_wider_than_a_wave_of_dwords():
    assert _sweep((1, 9, 130), np.uint8, 8) == 128


def test_u8_1x3x3_rows_narrower_than_a_dword():
    assert _sweep((1, 3, 3), np.uint8, 8) == 128


@pytest.mark.parametrize("byte_offset", [1, 2, 3])
def test_u8_2x6x16_from_a_source_off_the_dword_grid(byte_offset):
    assert _sweep((2, 6, 16), np.uint8, 8, byte_offset=byte_offset) == 128


def test_u8_3x5x7_with_a_source_pitch_that_is_no_multiple_of_four():
    assert _sweep((3, 5, 7), np.uint8, 8, byte_offset=2, pitch_extra=6) == 128   # samples 111 bytes apart


def test_f32_3x5x7():
    assert _sweep((3, 5, 7), np.float32, 8) == 128


def test_f32_1x1x10_vector_key():
    assert _sweep((1, 1, 10), np.float32, 8, byte_offset=4) == 128


def test_the_sweeps_rectangles_cut_dwords_and_touch_row_ends():
    """what the (2, 5) sweeps above rely on, read off the model's draws: at 2 x 6 x 16 some rectangles begin and some end off
    the 4-pixel grid, some reach the last column (the dword that holds a row end) and some the first"""
    y0, x0, ch, cw = frame_ops.cutout_draws(12345, 0, np.arange(E * (T + 1)), 6, 16, 2, 5)
    assert (x0 % 4 != 0).any() and ((x0 + cw) % 4 != 0).any()
    assert (x0 + cw == 16).any() and (x0 == 0).any() and (y0 + ch == 6).any() and (y0 == 0).any()
    whole = frame_ops.cutout_draws(12345, 0, np.arange(8), 6, 16, 9, 15)
    assert (whole[2] == 6).all() and (whole[0] == 0).all()            # (H + 3, H + 9): every row


@pytest.mark.parametrize("shape,dtype", [((3, 300, 100), np.uint8),    # 90000 bytes: strips of the sample through the LDS
                                         ((2, 40, 300), np.float32),   # 96000 bytes, f32
                                         ((1, 2, 40000), np.uint8)],   # a row does not fit the LDS: the dword-wise path
                         ids=["u8_strips", "f32_strips", "u8_wide_rows"])
def test_samples_larger_than_the_lds(shape, dtype):
    from sample_factory_amd import lib
    frames = _frames(shape, dtype, E * (T + 1), 3)
    src, stride = _device_view(frames, 0 if dtype == np.float32 else 3, 0 if dtype == np.float32 else 1)
    n = 4
    index, offset, d = _rows_of("index", n, 1, T, np.random.default_rng(1))
    fill = "random" if dtype == np.uint8 else "zero"
    for ops in (dict(pad=4, cutout=(20, 150), cutout_fill=fill, intensity=64), dict(cutout=(1, 60000), intensity=255)):
        _launch_and_check(lib, frames, src, stride, shape, n, index, offset, d, T, 1, 4, 9, ops, (shape, ops))


def test_n_zero_is_a_no_op_and_typed_refusals():
    from sample_factory_amd import lib
    src = torch.zeros((8, 3, 5, 7), dtype=torch.uint8, device="cuda")
    dst = torch.full((4, 105), GUARD, dtype=torch.uint8, device="cuda")
    on = dict(pad=4, cutout=(2, 5), cutout_fill="random", intensity=64, seed=1, draw_id=1)
    lib.augment_gather(dst, src, 0, (3, 5, 7), **on)
    assert (dst == GUARD).all()
    with pytest.raises(lib.SfHipError, match="dtype"):
        lib.augment_gather(dst.float(), src, 4, (3, 5, 7), **on)
    with pytest.raises(lib.SfHipError, match="dtype"):
        lib.augment_gather(dst.cpu(), src, 4, (3, 5, 7), **on)
    with pytest.raises(lib.SfHipError, match="at least n"):
        lib.augment_gather(dst, src, 5, (3, 5, 7), **on)                  # dst holds 4 rows
    with pytest.raises(lib.SfHipError, match="contiguous rows"):
        lib.augment_gather(dst[:, :104], src, 4, (3, 5, 7), **on)
    with pytest.raises(lib.SfHipError, match="index"):
        lib.augment_gather(dst, src, 4, (3, 5, 7), index=torch.zeros(4, dtype=torch.int64, device="cuda"), **on)
    with pytest.raises(lib.SfHipError, match="cutout must be"):
        lib.augment_gather(dst, src, 4, (3, 5, 7), cutout=(2,))
    with pytest.raises(lib.SfHipError, match="cutout_fill"):
        lib.augment_gather(dst, src, 4, (3, 5, 7), cutout=(2, 5), cutout_fill="mean")
    for bad in (dict(pad=256), dict(cutout=(0, 5)), dict(cutout=(6, 5)), dict(cutout=(1, 65536)), dict(intensity=256),
                dict(intensity=-1)):
        with pytest.raises(lib.SfHipError, match="sf_augment_gather"):
            lib.augment_gather(dst, src, 4, (3, 5, 7), **bad)
    with pytest.raises(lib.SfHipError, match="sf_augment_gather"):       # a random byte is no f32 value
        lib.augment_gather(dst.float(), src.float(), 4, (3, 5, 7), cutout=(2, 5), cutout_fill="random")
    assert (dst == GUARD).all()
