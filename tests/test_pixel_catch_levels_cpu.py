"""PixelCatch levels on the CPU (the NumPy model, the contract of sf_pixcatch_reset_levels / sf_pixcatch_step_levels): decoys
change the rendered frame only, a level is drawn per episode from the set [S, S + L), and a level's decoys depend on nothing
but the level id and the field."""
import os
import re

import numpy as np
import pytest

from sample_factory_amd import lib
from sample_factory_amd.envs import pixel_catch as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [(12, 12, 2, 2), (36, 36, 4, 4), (10, 10, 1, 1), (9, 9, 4, 3)]  # H, W, k, balls


def _actions(rng, N):
    a = rng.integers(0, 3, N).astype(np.int64)
    return np.where(rng.random(N) < 0.1, rng.choice(np.array([3, -1, 7, 2 ** 31 - 1, -2 ** 31], np.int64), N), a)


def _decoy_mask(state, env0, seed, H, W, balls, nd, L, S):
    """bool [N, H, W]: the pixels of the decoys of every env's current level"""
    g = pc.geometry(H, W)
    level = pc.episode_level(state, env0 + np.arange(state.shape[0]), seed, balls, L, S)
    dx, dy = pc.level_decoys(level, nd, H, W)
    m = np.zeros((state.shape[0], H, W), bool)
    for e in range(state.shape[0]):
        for d in range(nd):
            m[e, dy[e, d]:dy[e, d] + g.bs, dx[e, d]:dx[e, d] + g.bs] = True
    return m


def test_entry_points_are_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sf_hip.h")).read(), flags=re.S)
    L = lib.load()
    for name in ("sf_pixcatch_reset_levels", "sf_pixcatch_step_levels"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/sf_hip.h"
        assert name in lib.SYMBOLS and hasattr(L, name)
    assert L.sf_abi_version() == 19


def test_philox_lanes_six_and_seven_belong_to_the_levels_and_are_documented():
    """lane 2 of the counter: 0 .. 5 are taken (tests/test_augment_shift_cpu.py counts the literal ones); the levels take 6
    and 7 as named constants of sf_pixcatch.hip, no other source names them, and the header says so"""
    csrc = os.path.join(ROOT, "sample_factory_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    own = src["sf_pixcatch.hip"]
    assert re.search(r"constexpr uint32_t PC_LANE_LEVEL = 6u;", own) and re.search(r"constexpr uint32_t PC_LANE_DECOY = 7u;", own)
    for lane, const in ((6, "PC_LANE_LEVEL"), (7, "PC_LANE_DECOY")):
        assert len(re.findall(r"sf_philox4x32_10\([^;]*?,\s*%s\s*," % const, own)) == 1
        for name, text in src.items():
            for m in re.finditer(r"sf_philox4x32_10\(([^;]*?)\);", text, re.S):
                args = [a.strip() for a in m.group(1).split(",")]
                assert not (len(args) >= 7 and args[2].rstrip("u") == str(lane)), f"{name} draws from lane {lane}"
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert "counter (ep, 0, 6, 0)" in text and "counter (d, 0, 7, 0)" in text and "0x4C564C53" in text
    assert pc.LEVEL_KEY == 0x4C564C53


@pytest.mark.parametrize("H,W,k,balls", FIELDS)
def test_without_decoys_levels_have_no_effect(H, W, k, balls):
    rng = np.random.default_rng(H + k)
    N, env0, seed = 6, 3, 9
    a0 = pc.model_reset(N, env0, seed, H, W, k, balls)
    for _ in range(4):
        L, S = int(rng.integers(0, 1000)), int(rng.integers(0, 2 ** 32))
        b0 = pc.model_reset(N, env0, seed, H, W, k, balls, 0, L, S)
        assert np.array_equal(a0, b0)
        a, b = a0, b0
        for _ in range(60):
            act = _actions(rng, N)
            a, ra, ta = pc.model_step(a, act, env0, seed, H, W, k, balls)
            b, rb, tb = pc.model_step(b, act, env0, seed, H, W, k, balls, 0, L, S)
            assert np.array_equal(a, b) and ra.tobytes() == rb.tobytes() and np.array_equal(ta, tb)
            assert np.array_equal(pc.render(a, H, W, k), pc.render(b, H, W, k, env0, seed, balls, 0, L, S))


@pytest.mark.parametrize("nd", [1, 3, 8])
@pytest.mark.parametrize("H,W,k,balls", FIELDS)
def test_decoys_change_the_frame_only_and_stay_off_the_paddle_rows(H, W, k, balls, nd):
    rng = np.random.default_rng(100 * nd + H)
    N, env0, seed, L, S = 8, 5, 4, 4, 17
    g = pc.geometry(H, W)
    a = pc.model_reset(N, env0, seed, H, W, k, balls)
    b = pc.model_reset(N, env0, seed, H, W, k, balls, nd, L, S)
    assert np.array_equal(a, b)
    changed = 0
    for _ in range(120):
        act = _actions(rng, N)
        a, ra, ta = pc.model_step(a, act, env0, seed, H, W, k, balls)
        b, rb, tb = pc.model_step(b, act, env0, seed, H, W, k, balls, nd, L, S)
        assert np.array_equal(a, b) and ra.tobytes() == rb.tobytes() and np.array_equal(ta, tb)
        plain, frame = pc.render(a, H, W, k), pc.render(b, H, W, k, env0, seed, balls, nd, L, S)
        mask = _decoy_mask(b, env0, seed, H, W, balls, nd, L, S)
        assert not mask[:, H - g.ph:].any() and mask.any((1, 2)).all()
        m = np.broadcast_to(mask[:, None], frame.shape)
        assert np.array_equal(frame[~m], plain[~m]) and (frame[m] == pc.BALL).all()
        changed += int((frame != plain).sum())
    assert changed > 0


def test_levels_lie_in_the_set_and_change_only_at_terminations():
    N, H, W, k, balls, seed, env0, L, S = 16, 12, 12, 2, 1, 3, 7, 4, 17
    env = pc.PixelCatchHostEnv(N, (H, W), k, balls, seed, env0, decoys=3, levels=L, start_level=S)
    env.reset()
    level = env.current_levels()
    assert level.dtype == np.uint32 and ((level >= S) & (level < S + L)).all()
    ep = (env.state[:, 0] - 1) // balls
    assert (ep == 0).all()
    rng, redrawn, moved = np.random.default_rng(0), 0, 0
    for _ in range(200):
        _, _, term, _, _ = env.step(rng.integers(0, 3, N))
        new, new_ep = env.current_levels(), (env.state[:, 0] - 1) // balls
        assert ((new >= S) & (new < S + L)).all()
        assert np.array_equal(new_ep, ep + term)               # the episode index increments exactly at terminated
        assert np.array_equal(new[~term], level[~term])        # constant inside an episode
        want = pc.philox(new_ep.astype(np.uint32), 0, 6, 0, seed, (env0 + np.arange(N)).astype(np.uint32))[0]
        assert np.array_equal(new, (S + ((want.astype(np.uint64) * np.uint64(L)) >> np.uint64(32))).astype(np.uint32))
        redrawn, moved = redrawn + int(term.sum()), moved + int((new[term] != level[term]).sum())
        level, ep = new, new_ep
    assert redrawn >= 10 * N and moved > redrawn // 2  # (a redraw keeps the level one time in four)


def test_every_level_of_a_small_set_occurs():
    """L = 4 over 64 envs x 50 episodes: the draw gives each level 776 .. 831 of the 3200 episodes"""
    balls, seed = 1, 1
    state = np.zeros((64, pc.state_words(1)), np.int32)
    counts = np.zeros(4, np.int64)
    for ep in range(50):
        state[:, 0] = ep * balls + 1
        counts += np.bincount(pc.episode_level(state, np.arange(64), seed, balls, 4, 0), minlength=4)
    print(f"episodes per level: {counts.tolist()}")
    assert counts.sum() == 3200 and (counts > 0).all(), counts


def test_a_level_looks_the_same_in_every_run():
    H, W, k, nd = 12, 12, 2, 3
    dx, dy = pc.level_decoys(np.uint32(7), nd, H, W)
    dx2, dy2 = pc.level_decoys(np.array([7, 7, 8], np.uint32), nd, H, W)
    assert dx.shape == (nd,) and np.array_equal(dx2[0], dx) and np.array_equal(dx2[1], dx) and np.array_equal(dy2[0], dy)
    assert not (np.array_equal(dx2[2], dx) and np.array_equal(dy2[2], dy))
    g = pc.geometry(H, W)
    assert (dx >= 0).all() and (dx <= W - g.bs).all() and (dy >= 0).all() and (dy + g.bs <= H - g.ph).all()
    # decoy d of a level does not depend on how many decoys the level has
    assert np.array_equal(pc.level_decoys(np.uint32(7), 8, H, W)[0][:nd], dx)
    # L = 1: every episode of every env, whatever the seed, plays level S; once ball and paddle agree the frames agree
    a = pc.model_reset(1, 0, 11, H, W, k, 2)
    b = pc.model_reset(1, 40, 12, H, W, k, 2)
    b[:, pc.HDR:] = a[:, pc.HDR:]
    b[:, 0] = 5                      # another episode as well
    fa = pc.render(a, H, W, k, 0, 11, 2, nd, 1, 7)
    fb = pc.render(b, H, W, k, 40, 12, 2, nd, 1, 7)
    assert np.array_equal(fa, fb) and not np.array_equal(fa, pc.render(a, H, W, k))
    assert (pc.episode_level(b, [40], 12, 2, 1, 7) == 7).all()
    # and a level of a larger set shows the same decoys as the same id in a set of one
    c = pc.render(a, H, W, k, 0, 11, 2, nd, 5, 3)
    lv = int(pc.episode_level(a, [0], 11, 2, 5, 3)[0])
    assert np.array_equal(c, pc.render(a, H, W, k, 0, 11, 2, nd, 1, lv))


def test_unlimited_levels_and_a_start_near_the_top_wrap():
    H, W, k, balls, seed, S = 12, 12, 2, 1, 2, 4294967290
    env = pc.PixelCatchHostEnv(32, (H, W), k, balls, seed, 0, decoys=8, levels=0, start_level=S)
    o, _ = env.reset()
    w = pc.philox(np.zeros(32, np.uint32), 0, 6, 0, seed, np.arange(32, dtype=np.uint32))[0]
    assert np.array_equal(env.current_levels(), ((w.astype(np.uint64) + np.uint64(S)) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert len(set(env.current_levels().tolist())) == 32 and (env.current_levels() < S).any()
    rng = np.random.default_rng(3)
    for _ in range(40):
        o, *_ = env.step(rng.integers(0, 3, 32))
    assert o["obs"].shape == (32, k, H, W) and set(np.unique(o["obs"])) <= {0, 128, 255}
    # a finite set that straddles 2^32
    lv = pc.episode_level(env.state, np.arange(32), seed, balls, 16, S)
    assert set(lv.tolist()) <= {(S + i) % 2 ** 32 for i in range(16)} and (lv < 16).any() and (lv >= S).any()


def test_refusals_and_flags():
    import argparse
    from types import SimpleNamespace
    for kw in (dict(decoys=-1), dict(decoys=9), dict(levels=-1), dict(start_level=-1), dict(start_level=2 ** 32)):
        with pytest.raises(ValueError):
            pc.PixelCatchHostEnv(2, (12, 12), 2, 2, **kw)
    with pytest.raises(ValueError):
        pc.render(pc.model_reset(1, 0, 0, 12, 12, 1, 1), 12, 12, 1, decoys=9)
    p = argparse.ArgumentParser()
    pc.add_pixel_catch_args(p)
    d = p.parse_args([])
    assert (d.pixel_catch_decoys, d.pixel_catch_levels, d.pixel_catch_start_level) == (0, 0, 0)
    a = p.parse_args(["--pixel_catch_decoys=6", "--pixel_catch_levels=8", "--pixel_catch_start_level=1000000"])
    cfg = SimpleNamespace(pixel_catch_agents=3, pixel_catch_size=12, pixel_catch_frames=2, pixel_catch_balls=2, seed=5,
                          pixel_catch_decoys=a.pixel_catch_decoys, pixel_catch_levels=a.pixel_catch_levels,
                          pixel_catch_start_level=a.pixel_catch_start_level)
    env = pc.make_pixel_catch_host_env("x", cfg, SimpleNamespace(env_id=1))
    assert (env.decoys, env.levels, env.start_level, env.env0) == (6, 8, 1000000, 3)
    plain = pc.make_pixel_catch_host_env("x", SimpleNamespace(pixel_catch_agents=3, pixel_catch_size=12, seed=5), None)
    assert (plain.decoys, plain.levels, plain.start_level) == (0, 0, 0)
