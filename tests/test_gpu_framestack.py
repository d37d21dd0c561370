"""sf_framestack_step against a numpy deque on the GPU: every access width (16 / 4 / 1 bytes), in-place and separate new
frames, every flag pattern, slab columns with guard bands around the slab.  A copy: every comparison is exact."""
from collections import deque

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 3          # next / prev are columns 2 / 1 of a [rows, T + 1, k C, H, W] slab
GUARD = 256    # sentinel bytes in front of and behind the slab
FRAMES = {     # name -> (shape, dtype); the comment: the access unit an aligned slab gets
    "u8_1x7x9_63B": ((1, 7, 9), torch.uint8),        # bytes
    "u8_1x8x8_64B": ((1, 8, 8), torch.uint8),        # 16-byte units
    "u8_3x6x6_108B": ((3, 6, 6), torch.uint8),       # 4-byte units
    "f32_3x5x4_240B": ((3, 5, 4), torch.float32),    # 16-byte units
    "u8_1x84x84": ((1, 84, 84), torch.uint8),        # the Atari frame, 16-byte units
}
FLAGS = ["none_done", "all_done", "random", "only_truncated", "truncated_pointer_only", "reset"]


def deque_reference(prev: np.ndarray, frame: np.ndarray, k: int, done) -> np.ndarray:
    """prev [rows, k, fb] bytes, frame [rows, fb] bytes, done [rows] bool or None (= reset) -> next [rows, k, fb]"""
    out = np.empty_like(prev)
    for b in range(prev.shape[0]):
        d = deque((prev[b, j] for j in range(k)), maxlen=k)
        for _ in range(k if (done is None or done[b]) else 1):
            d.append(frame[b])
        out[b] = np.stack(list(d))
    return out


def _flags(kind, rows, gen):
    z = torch.zeros(rows, dtype=torch.bool)
    rnd = lambda: torch.rand(rows, generator=gen) < 0.3
    term, trunc = dict(none_done=(z, z), all_done=(~z, z), random=(rnd(), rnd()), only_truncated=(z, rnd()),
                       truncated_pointer_only=(None, rnd()), reset=(None, None))[kind]
    done = None if kind == "reset" else ((term if term is not None else z) | trunc).numpy()
    dev = lambda t: None if t is None else t.cuda()
    return dev(term), dev(trunc), done


def _run_case(shape, dtype, k, rows, offset_elems, seed):
    from sample_factory_amd import lib
    es = torch.empty(0, dtype=dtype).element_size()
    c, h, w = shape
    fb = c * h * w * es
    off = offset_elems * es
    slab_bytes = rows * (T + 1) * k * fb
    gen = torch.Generator().manual_seed(seed)
    flat0 = torch.randint(0, 256, (GUARD + off + slab_bytes + GUARD,), dtype=torch.uint8, generator=gen)
    flat0[:GUARD + off] = 0xA5
    flat0[GUARD + off + slab_bytes:] = 0x5A
    flat0 = flat0.cuda()

    def views(flat):
        body = flat[GUARD + off: GUARD + off + slab_bytes]
        return body.view(dtype).view(rows, T + 1, k * c, h, w), body.view(rows, T + 1, k, fb)

    for in_place in (True, False):
        for kind in FLAGS:
            term, trunc, done = _flags(kind, rows, gen)
            new = torch.randint(0, 256, (rows, fb), dtype=torch.uint8, generator=gen)
            flat = flat0.clone()
            slab, slab_b = views(flat)
            wide = None
            if in_place:   # the DMA's job: the new frame already sits in the last slot of column t + 1
                slab_b[:, 2, k - 1] = new.cuda()
                frame = None
            else:          # a separate buffer with its own, larger pitch
                wide = torch.full((rows, fb + 48), 0x3C, dtype=torch.uint8).cuda()
                wide[:, :fb] = new.cuda()
                frame = wide[:, :fb].view(dtype)
            wide0 = None if wide is None else wide.clone()
            expect = flat.clone()
            ref = deque_reference(slab_b[:, 1].cpu().numpy(), new.numpy(), k, done)
            views(expect)[1][:, 2] = torch.from_numpy(ref).cuda()
            for launch in range(2):  # a second launch must give identical bits
                lib.framestack_step(slab[:, 2], slab[:, 1], k, frame, term, trunc)
                torch.cuda.synchronize()
                what = f"{shape} {dtype} k={k} rows={rows} off={offset_elems} in_place={in_place} flags={kind} launch={launch}"
                assert torch.equal(views(flat)[1][:, 2], views(expect)[1][:, 2]), "next differs: " + what
                # everything else — prev, columns 0 and 3, both guard bands — is untouched
                assert torch.equal(flat, expect), "bytes outside next changed: " + what
                if wide is not None:
                    assert torch.equal(wide, wide0), "the frame buffer changed: " + what


@pytest.mark.parametrize("rows", [1, 37, 300])
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("name", list(FRAMES))
def test_framestack_step_matches_a_deque(name, k, rows):
    shape, dtype = FRAMES[name]
    _run_case(shape, dtype, k, rows, offset_elems=0, seed=1000 * k + rows)


@pytest.mark.parametrize("name", ["u8_1x8x8_64B", "f32_3x5x4_240B", "u8_1x84x84"])
def test_framestack_step_on_a_base_offset_by_one_element(name):
    """every address moves off its 16-byte (u8: also its 4-byte) alignment: the narrower path must be taken"""
    shape, dtype = FRAMES[name]
    _run_case(shape, dtype, 4, 37, offset_elems=1, seed=7)


def test_binding_refuses_what_is_not_a_pair_of_slab_columns():
    from sample_factory_amd import lib
    slab = torch.zeros((4, T + 1, 8, 5, 5), dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.SfHipError, match="sf_framestack_step"):
        lib.framestack_step(slab[:, 2], slab[:, 2], 4)                       # next is prev
    with pytest.raises(lib.SfHipError, match="not k = 3 frames"):
        lib.framestack_step(slab[:, 2], slab[:, 1], 3)
    with pytest.raises(lib.SfHipError, match="equal shape"):
        lib.framestack_step(slab[:, 2], slab[:, 1, :4], 4)
    with pytest.raises(lib.SfHipError, match="frame must be"):
        lib.framestack_step(slab[:, 2], slab[:, 1], 4, frame=torch.zeros((4, 3, 5, 5), dtype=torch.uint8, device="cuda"))
    with pytest.raises(lib.SfHipError, match="k=17"):
        lib.framestack_step(torch.zeros((2, 2, 34), dtype=torch.uint8, device="cuda")[:, 0],
                            torch.zeros((2, 2, 34), dtype=torch.uint8, device="cuda")[:, 1], 17)
