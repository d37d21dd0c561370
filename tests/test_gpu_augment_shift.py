"""sf_random_shift_gather on the GPU against the NumPy model (envs/frame_ops.py: random_shift_draws, random_shift_frames),
BIT FOR BIT: u8 and f32 frames, sizes at which nothing is aligned, a row wider than one wave of dwords, source views off the
dword grid, both row addressings (index with repeated chunks / offset, slab rows with traj_T / dense rows), chunk-wise draws,
pad 0 (= index_select), 1 and 4, two draw ids and two seeds; guard bands around the destination; samples that take the strip
and the LDS-free paths.  No tolerance: every comparison is exact."""
import numpy as np
import pytest
import torch

from sample_factory_amd.envs import frame_ops

pytestmark = pytest.mark.gpu

E, T = 6, 4            # the slab is [E, T + 1, C, H, W]: dataset row d of traj_T = T sits at slab row d + d // T
GUARD = 0xA5


def _frames(shape, dtype, rows, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (rows,) + shape, dtype=np.uint8)
    return rng.standard_normal((rows,) + shape).astype(np.float32)


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
    with one chunk repeated, as the learner's shuffled minibatches are (plus the repeat)"""
    nd = E * T if traj_T else E * (T + 1)
    if kind == "offset":
        offset = recurrence  # a chunk boundary that is not 0
        return None, offset, np.arange(offset, offset + n, dtype=np.int64)
    starts = rng.permutation(np.arange(0, nd - recurrence + 1, recurrence))
    starts = np.concatenate([starts[:2], starts[:1], starts[2:]])  # chunk 0 of the shuffle comes twice
    d = (starts[:, None] + np.arange(recurrence)[None, :]).reshape(-1)[:n]
    assert len(d) == n
    return torch.from_numpy(d.astype(np.int32)).cuda(), 0, d.astype(np.int64)


def _expect(frames, d, traj_T, recurrence, pad, seed, draw_id):
    rows = d + d // traj_T if traj_T else d
    dy, dx = frame_ops.random_shift_draws(seed, draw_id, d // recurrence, pad)
    return frame_ops.random_shift_frames(frames[rows], dy, dx, pad)


def _sweep(shape, dtype, n, byte_offset=0, pitch_extra=0):
    from sample_factory_amd import lib
    frames = _frames(shape, dtype, E * (T + 1), sum(shape) + byte_offset)
    src, stride = _device_view(frames, byte_offset, pitch_extra)
    S = int(np.prod(shape))
    tdt = src.dtype
    rng = np.random.default_rng(5)
    launches = 0
    for kind in ("index", "offset"):
        for traj_T in (T, 0):
            for recurrence in (1, 4):
                index, offset, d = _rows_of(kind, n, recurrence, traj_T, rng)
                for pad in (0, 1, 4):
                    for draw_id, seed in ((0, 12345), (7, 12345), (0, 99), (7, 99)):
                        # a guard row in front and behind, 5 guard elements behind every sample
                        full = torch.full((n + 2, S + 5), GUARD, dtype=tdt, device="cuda")
                        dst = full[1:n + 1, :S]
                        lib.random_shift_gather(dst, src, n, shape, sample_stride=stride, index=index, offset=offset,
                                                traj_T=traj_T, pad=pad, recurrence=recurrence, seed=seed, draw_id=draw_id)
                        launches += 1
                        got = full.cpu().numpy()
                        want = _expect(frames, d, traj_T, recurrence, pad, seed, draw_id).reshape(n, S)
                        what = (shape, kind, traj_T, recurrence, pad, draw_id, seed, byte_offset)
                        assert np.array_equal(np.ascontiguousarray(got[1:n + 1, :S]).view(np.uint8), want.view(np.uint8)), what
                        assert (got[0] == GUARD).all() and (got[n + 1] == GUARD).all() and (got[:, S:] == GUARD).all(), what
                        if pad == 0:  # the plain gather: torch's index_select of the slab rows
                            rows = torch.from_numpy(d + d // traj_T if traj_T else d).cuda()
                            sel = src[:, :S].index_select(0, rows)
                            assert torch.equal(dst.contiguous().view(torch.uint8), sel.contiguous().view(torch.uint8)), what
                        if recurrence == 4 and pad == 4 and kind == "index":  # every row of a chunk got ONE shift
                            dy, dx = frame_ops.random_shift_draws(seed, draw_id, d // recurrence, pad)
                            full_chunks = (n // 4) * 4
                            assert (dy[:full_chunks].reshape(-1, 4) == dy[:full_chunks:4, None]).all()
                            assert (dx[:full_chunks].reshape(-1, 4) == dx[:full_chunks:4, None]).all()
    return launches


def test_u8_3x5x7_nothing_aligned_most_columns_clamp():
    assert _sweep((3, 5, 7), np.uint8, 8) == 96          # samples of 105 bytes


def test_u8_4x84x84():
    assert _sweep((4, 84, 84), np.uint8, 6) == 96


def test_u8_1x9x130_row_wider_than_a_wave_of_dwords():
    assert _sweep((1, 9, 130), np.uint8, 8) == 96


@pytest.mark.parametrize("byte_offset", [1, 2, 3])
def test_u8_2x6x16_from_a_source_off_the_dword_grid(byte_offset):
    assert _sweep((2, 6, 16), np.uint8, 8, byte_offset=byte_offset) == 96


def test_u8_3x5x7_with_a_source_pitch_that_is_no_multiple_of_four():
    assert _sweep((3, 5, 7), np.uint8, 8, byte_offset=2, pitch_extra=6) == 96   # samples 111 bytes apart


def test_f32_3x5x7():
    assert _sweep((3, 5, 7), np.float32, 8) == 96


def test_f32_1x1x10_vector_key():
    assert _sweep((1, 1, 10), np.float32, 8, byte_offset=4) == 96


@pytest.mark.parametrize("shape,dtype", [((3, 300, 100), np.uint8),    # 90000 bytes: strips of the sample through the LDS
                                         ((2, 40, 300), np.float32),   # 96000 bytes, f32
                                         ((1, 2, 40000), np.uint8)],   # a row does not fit the LDS: the dword-wise path
                         ids=["u8_strips", "f32_strips", "u8_wide_rows"])
def test_samples_larger_than_the_lds(shape, dtype):
    from sample_factory_amd import lib
    frames = _frames(shape, dtype, E * (T + 1), 3)
    src, stride = _device_view(frames, 0 if dtype == np.float32 else 3, 0 if dtype == np.float32 else 1)
    S, n = int(np.prod(shape)), 4
    index, offset, d = _rows_of("index", n, 1, T, np.random.default_rng(1))
    for pad in (0, 4):
        full = torch.full((n + 2, S + 3), GUARD, dtype=src.dtype, device="cuda")
        lib.random_shift_gather(full[1:n + 1, :S], src, n, shape, sample_stride=stride, index=index, offset=offset, traj_T=T,
                                pad=pad, recurrence=1, seed=4, draw_id=9)
        got = full.cpu().numpy()
        want = _expect(frames, d, T, 1, pad, 4, 9).reshape(n, S)
        assert np.array_equal(np.ascontiguousarray(got[1:n + 1, :S]).view(np.uint8), want.view(np.uint8)), (shape, pad)
        assert (got[0] == GUARD).all() and (got[n + 1] == GUARD).all() and (got[:, S:] == GUARD).all(), (shape, pad)


def test_n_zero_is_a_no_op_and_typed_refusals():
    from sample_factory_amd import lib
    src = torch.zeros((8, 3, 5, 7), dtype=torch.uint8, device="cuda")
    dst = torch.full((4, 105), GUARD, dtype=torch.uint8, device="cuda")
    lib.random_shift_gather(dst, src, 0, (3, 5, 7), pad=4, seed=1, draw_id=1)
    assert (dst == GUARD).all()
    with pytest.raises(lib.SfHipError, match="dtype"):
        lib.random_shift_gather(dst.float(), src, 4, (3, 5, 7))
    with pytest.raises(lib.SfHipError, match="dtype"):
        lib.random_shift_gather(dst.cpu(), src, 4, (3, 5, 7))
    with pytest.raises(lib.SfHipError, match="at least n"):
        lib.random_shift_gather(dst, src, 5, (3, 5, 7))                  # dst holds 4 rows
    with pytest.raises(lib.SfHipError, match="contiguous rows"):
        lib.random_shift_gather(dst[:, :104], src, 4, (3, 5, 7))
    with pytest.raises(lib.SfHipError, match="index"):
        lib.random_shift_gather(dst, src, 4, (3, 5, 7), index=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(lib.SfHipError, match="sf_random_shift_gather"):
        lib.random_shift_gather(dst, src, 4, (3, 5, 7), pad=256)
    assert (dst == GUARD).all()
