"""sf_pixcatch_reset_levels / sf_pixcatch_step_levels against the NumPy model (sample_factory_amd/envs/pixel_catch.py), bit for
bit: every plane, reward, flag and state word at every one of 300 steps of random actions, values outside 0 .. 2 among them.

Shapes: 20 x 20, 36 x 36 and 84 x 84 planes are multiples of 16 bytes in a field at least 16 wide (16-byte units of at most
two rows, the decoys one aligned 16-byte read of the plane kept in LDS); 12 x 12 takes the generic 16-byte units, 10 x 10 x 4
generic 16-byte units that straddle a plane end (100 % 16), 10 x 10 x 1 and 9 x 9 x 4 the 4-byte units (the latter across
plane ends): their decoy bytes are aligned dwords shifted by bytes, past the plane's end the next plane's first bytes.
balls = 1: an episode, and with it the level, turns over every D / vy steps.  Every shape meets every pair of nd in {1, 3, 8}
and (L, S) in {(1, 0), (4, 17), (0, 4294967290)}; the small fields spread N = 1, 5, 257 over the pairs, the two large ones run
N = 5.  obs_out is a column of a pitched slab with guard bytes behind every row, which must come back untouched."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd import lib  # noqa: E402
from sample_factory_amd.envs import pixel_catch as pc  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, BALLS, GUARD, FILL = 300, 1, 16, 0xA5
SMALL = [(12, 12, 1), (12, 12, 4), (10, 10, 1), (10, 10, 4), (9, 9, 4), (20, 20, 4)]
LARGE = [(36, 36, 4), (84, 84, 4)]
DECOYS, SETS, NS = (1, 3, 8), ((1, 0), (4, 17), (0, 4294967290)), (1, 5, 257)
CASES = [(H, W, k, NS[(i + j) % 3], DECOYS[i], *SETS[j]) for H, W, k in SMALL for i in range(3) for j in range(3)] + \
        [(H, W, k, 5, DECOYS[i], *SETS[j]) for H, W, k in LARGE for i in range(3) for j in range(3)]


class Slab:
    """[N, 2 columns] of k H W frame bytes + GUARD guard bytes each, filled with FILL; column(t) is the view the runner
    hands over as obs[:, t].  `shift`: bytes the slab's base is moved off its 16-byte alignment."""

    def __init__(self, N, H, W, k, shift=0, guard=GUARD):
        self.N, self.shape, self.fb, self.cell, self.shift = N, (k, H, W), k * H * W, k * H * W + guard, shift
        self.raw = torch.full((N * 2 * self.cell + 16,), FILL, dtype=torch.uint8, device="cuda")
        self.buf = self.raw[shift:shift + N * 2 * self.cell].view(N, 2, self.cell)

    def column(self, t):
        return self.buf[:, t, :self.fb].unflatten(1, self.shape)

    def guards_intact(self):
        end = self.shift + self.buf.numel()
        return bool((self.buf[:, :, self.fb:] == FILL).all()) and bool((self.raw[:self.shift] == FILL).all()) and \
            bool((self.raw[end:] == FILL).all())


def actions_for(rng, N):
    a = rng.integers(0, 3, N).astype(np.int32)
    odd = rng.random(N) < 0.1
    return np.where(odd, rng.choice(np.array([3, -1, 7, 2 ** 31 - 1, -2 ** 31], np.int64), N), a).astype(np.int32)


def run_against_model(N, H, W, k, nd, L, S, seed=9, env0=3, steps=STEPS, shift=0, guard=GUARD):
    slab = Slab(N, H, W, k, shift, guard)
    state = torch.zeros((N, lib.pixcatch_state_words(k)), dtype=torch.int32, device="cuda")
    rew = torch.full((N,), 7.0, dtype=torch.float32, device="cuda")
    term = torch.ones(N, dtype=torch.bool, device="cuda")
    frame = lambda st: pc.render(st, H, W, k, env0, seed, BALLS, nd, L, S)  # noqa: E731
    lib.pixcatch_reset_levels(state, slab.column(0), env0, seed, BALLS, nd, L, S)
    model = pc.model_reset(N, env0, seed, H, W, k, BALLS, nd, L, S)
    assert np.array_equal(state.cpu().numpy(), model) and np.array_equal(slab.column(0).cpu().numpy(), frame(model))
    rng, episodes, levels = np.random.default_rng(seed), 0, set()
    for s in range(steps):
        a = actions_for(rng, N)
        col = slab.column((s + 1) % 2)
        lib.pixcatch_step_levels(state, torch.from_numpy(a).cuda(), col, rew, term, env0, seed, BALLS, nd, L, S)
        model, mrew, mterm = pc.model_step(model, a, env0, seed, H, W, k, BALLS, nd, L, S)
        assert np.array_equal(state.cpu().numpy(), model), f"state words differ at step {s}"
        assert rew.cpu().numpy().tobytes() == mrew.tobytes() and np.array_equal(term.cpu().numpy(), mterm), f"step {s}"
        assert np.array_equal(col.cpu().numpy(), frame(model)), f"planes differ at step {s}"
        episodes += int(mterm.sum())
        if mterm.any():
            levels |= set(pc.episode_level(model, env0 + np.arange(N), seed, BALLS, L, S).tolist())
    assert slab.guards_intact()
    return episodes, levels


@pytest.mark.parametrize("H,W,k,N,nd,L,S", CASES)
def test_kernel_equals_the_model_bit_for_bit(H, W, k, N, nd, L, S):
    episodes, levels = run_against_model(N, H, W, k, nd, L, S)
    assert episodes >= 3 * N  # (the slowest episode is one ball of D = 78 steps at 84 x 84)
    assert len(levels) >= (1 if L == 1 else 2)
    assert all((lv - S) % 2 ** 32 < L for lv in levels) or L == 0


@pytest.mark.parametrize("shift,guard", [(4, 16), (0, 4)])
def test_misaligned_slabs_take_the_four_byte_stores(shift, guard):
    """16-byte-sized frames in a slab whose base or pitch is a multiple of 4 only: 4-byte units inside a plane"""
    run_against_model(5, 20, 20, 4, 8, 4, 17, shift=shift, guard=guard, steps=60)
    run_against_model(3, 36, 36, 4, 3, 0, 4294967290, shift=shift, guard=guard, steps=60)


def test_a_field_at_the_limit_of_the_decoy_plane():
    """255 x 255 is the largest square whose plane of decoys fits 64 KB of LDS (12 x 12 decoys, 4-byte units); 240 x 240
    takes the 16-byte units of a wide field"""
    run_against_model(2, 255, 255, 4, 8, 4, 17, steps=40)
    run_against_model(2, 240, 240, 2, 8, 0, 4294967290, steps=40)


def _free_run(N, H, W, k, actions, levels_api, seed=4, env0=100, L=4, S=17):
    slab = Slab(N, H, W, k)
    state = torch.zeros((N, lib.pixcatch_state_words(k)), dtype=torch.int32, device="cuda")
    rew = torch.zeros(N, dtype=torch.float32, device="cuda")
    term = torch.zeros(N, dtype=torch.bool, device="cuda")
    if levels_api:
        lib.pixcatch_reset_levels(state, slab.column(0), env0, seed, BALLS, 0, L, S)
    else:
        lib.pixcatch_reset(state, slab.column(0), env0, seed, BALLS)
    out = [slab.column(0).cpu().numpy().tobytes(), state.cpu().numpy().tobytes()]
    for s, a in enumerate(actions):
        col, act = slab.column((s + 1) % 2), torch.from_numpy(a).cuda()
        if levels_api:
            lib.pixcatch_step_levels(state, act, col, rew, term, env0, seed, BALLS, 0, L, S)
        else:
            lib.pixcatch_step(state, act, col, rew, term, env0, seed, BALLS)
        out += [col.cpu().numpy().tobytes(), state.cpu().numpy().tobytes(), rew.cpu().numpy().tobytes(),
                term.cpu().numpy().tobytes()]
    assert slab.guards_intact()
    return out


@pytest.mark.parametrize("H,W,k", [(12, 12, 4), (9, 9, 4), (36, 36, 4)])
def test_without_decoys_the_new_entry_points_equal_the_old_ones_byte_for_byte(H, W, k):
    rng = np.random.default_rng(2)
    acts = [actions_for(rng, 7) for _ in range(80)]
    assert _free_run(7, H, W, k, acts, True) == _free_run(7, H, W, k, acts, False)


def test_refusals_name_the_entry_point_and_launch_nothing():
    N, H, W, k = 4, 12, 12, 2
    slab = Slab(N, H, W, k)
    state = torch.full((N, lib.pixcatch_state_words(k)), -7, dtype=torch.int32, device="cuda")
    rew = torch.full((N,), 7.0, dtype=torch.float32, device="cuda")
    term = torch.ones(N, dtype=torch.bool, device="cuda")
    act = torch.zeros(N, dtype=torch.int32, device="cuda")
    col, L, st = slab.column(0), lib.load(), lib.stream()
    p = lambda t: lib.C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731

    def raw_step(state_=state, k_=k, nd=3, levels=4):
        return L.sf_pixcatch_step_levels(p(state_), p(act), p(col), lib.i64(col.stride(0)), p(rew), p(term), N, 0, lib.u32(1),
                                         H, W, k_, 2, nd, levels, lib.u32(0), st)

    def raw_reset(state_=state, k_=k, nd=3, levels=4):
        return L.sf_pixcatch_reset_levels(p(state_), p(col), lib.i64(col.stride(0)), N, 0, lib.u32(1), H, W, k_, 2, nd, levels,
                                          lib.u32(0), st)

    for kw in (dict(nd=-1), dict(nd=9), dict(levels=-1), dict(state_=None), dict(k_=9)):
        assert raw_reset(**kw) == -1 and b"sf_pixcatch_reset_levels" in L.sf_last_error(), kw
        assert raw_step(**kw) == -1 and b"sf_pixcatch_step_levels" in L.sf_last_error(), kw
    for nd, levels in ((-1, 4), (9, 4), (3, -1)):
        with pytest.raises(lib.SfHipError, match="sf_pixcatch_step_levels"):
            lib.pixcatch_step_levels(state, act, col, rew, term, 0, 1, 2, nd, levels, 0)
        with pytest.raises(lib.SfHipError, match="sf_pixcatch_reset_levels"):
            lib.pixcatch_reset_levels(state, col, 0, 1, 2, nd, levels, 0)
    # the decoys of a level are kept as one plane of bytes in LDS: a 256 x 256 field runs without decoys only
    big = torch.full((N, 256 * 256), FILL, dtype=torch.uint8, device="cuda")
    assert L.sf_pixcatch_reset_levels(p(state), p(big), lib.i64(256 * 256), N, 0, lib.u32(1), 256, 256, 1, 2, 1, 4, lib.u32(0),
                                      st) == -1 and b"LDS" in L.sf_last_error()
    with pytest.raises(ValueError, match="LDS"):
        pc.PixelCatchVecEnv(2, (256, 256), 1, decoys=1)
    torch.cuda.synchronize()
    assert bool((state == -7).all()) and bool((rew == 7.0).all()) and bool(term.all()) and bool((slab.raw == FILL).all())
    assert bool((big == FILL).all())


def test_current_levels_equal_the_model_on_the_copied_back_state():
    N, size, k, seed, env0, nd, L, S = 9, (36, 36), 4, 3, 11, 3, 4, 1000000
    env = pc.PixelCatchVecEnv(N, size, k, BALLS, seed, env0, decoys=nd, levels=L, start_level=S)
    host = pc.PixelCatchHostEnv(N, size, k, BALLS, seed, env0, decoys=nd, levels=L, start_level=S)
    o, _ = env.reset()
    ho, _ = host.reset()
    assert np.array_equal(o["obs"].cpu().numpy(), ho["obs"])
    rng, seen = np.random.default_rng(0), set()
    for _ in range(60):
        a = rng.integers(0, 3, N)
        o, rew, term, _, _ = env.step(a)
        ho, hrew, hterm, _, _ = host.step(a)
        assert np.array_equal(o["obs"].cpu().numpy(), ho["obs"]) and np.array_equal(term.cpu().numpy(), hterm)
        lv = env.current_levels()
        assert lv.dtype == np.uint32 and np.array_equal(lv, host.current_levels())
        assert np.array_equal(lv, pc.episode_level(env.state.cpu().numpy(), env0 + np.arange(N), seed, BALLS, L, S))
        seen |= set(lv.tolist())
    assert seen == set(range(S, S + L))
