"""Random-shift augmentation (--augment_random_shift, sf_random_shift_gather) as far as it can be checked
without a GPU: the entry point's place in the C ABI, its argument refusals (all of them come before any launch), the engine
flag, and the NumPy model (envs/frame_ops.py): the distribution of the draws, what they depend on, and the shifted frames
against a literal pad-then-crop."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from sample_factory_amd.envs import frame_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sf_random_shift_gather"


def test_entry_point_is_declared_listed_and_exported_and_the_abi_version_stays():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert ENTRY in lib.SYMBOLS and re.search(r"\bint\s+" + ENTRY + r"\s*\(", text) and hasattr(L, ENTRY)
    assert callable(lib.random_shift_gather)
    assert len(lib.SYMBOLS) == len(set(lib.SYMBOLS))
    assert L.sf_abi_version() == 19
    from sample_factory_amd import build
    assert any(src == "sf_augment.hip" for src, _ in build.SOURCES)
    assert os.path.exists(os.path.join(build.CSRC, "sf_augment.hip"))


def _p(a):
    return None if a is None else C.c_void_p(a)


def _gather(L, dst=4096, dst_pitch=1 << 12, src=1 << 20, src_pitch=1 << 12, index=None, offset=0, n=8, traj_T=4, Cn=3, H=8, W=8,
            eb=1, pad=4, rec=1, seed=1, draw=0):
    return getattr(L, ENTRY)(_p(dst), C.c_int64(dst_pitch), _p(src), C.c_int64(src_pitch), _p(index), C.c_int64(offset),
                             C.c_int64(n), traj_T, Cn, H, W, eb, pad, rec, C.c_uint32(seed), C.c_uint32(draw), None)


def test_refusals_come_before_any_launch_and_name_the_entry_point():
    """made-up non-null addresses: each call must return -1 on a machine with no GPU"""
    from sample_factory_amd import lib
    L = lib.load()
    for kw in [dict(dst=None), dict(src=None), dict(n=-1), dict(pad=-1), dict(pad=256), dict(eb=0), dict(eb=2), dict(eb=8),
               dict(rec=0), dict(rec=-3), dict(H=0), dict(W=0), dict(Cn=0), dict(H=-2), dict(W=-1), dict(Cn=-1),
               dict(dst_pitch=191), dict(src_pitch=191),                      # C H W = 192
               dict(eb=4, dst_pitch=767), dict(eb=4, src_pitch=767),          # C H W elem_bytes = 768
               dict(traj_T=-1), dict(offset=-1)]:
        assert _gather(L, **kw) == -1, kw
        assert ENTRY in L.sf_last_error().decode(), (kw, L.sf_last_error().decode())


def test_n_zero_is_ok_and_launches_nothing():
    from sample_factory_amd import lib
    L = lib.load()
    assert _gather(L, n=0) == 0 and _gather(L, n=0, pad=0, eb=4, index=1 << 16) == 0
    assert _gather(L, n=0, pad=255, dst_pitch=192, src_pitch=192) == 0       # the bounds themselves are served


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_defaults_to_off_parses_and_is_bounded():
    from sample_factory_amd.cfg.arguments import ENGINE_FLAGS, FLAGS, default_cfg, parse_full_cfg, parse_sf_args, verify_cfg
    specs = {f[0]: f for f in ENGINE_FLAGS}
    assert specs["augment_random_shift"][1:] == (int, 0)
    assert "augment_random_shift" not in {f[0] for f in FLAGS}    # it shadows no reference flag
    assert default_cfg(env="x").augment_random_shift == 0
    argv = ["--env=x", "--augment_random_shift=4"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    assert cfg.augment_random_shift == 4 and cfg.cli_args["augment_random_shift"] == 4
    off = parse_full_cfg(parser, ["--env=x"])
    assert off.augment_random_shift == 0 and "augment_random_shift" not in off.cli_args
    info = type("I", (), dict(num_agents=1))()
    ok = dict(env="x", num_workers=1, num_envs_per_worker=2, rollout=4, batch_size=8, num_batches_per_epoch=1, use_rnn=False,
              recurrence=1)
    assert verify_cfg(default_cfg(**ok), info) and verify_cfg(default_cfg(augment_random_shift=255, **ok), info)
    assert not verify_cfg(default_cfg(augment_random_shift=-1, **ok), info)
    assert not verify_cfg(default_cfg(augment_random_shift=256, **ok), info)


def test_learner_refuses_the_bounds_and_a_model_it_cannot_augment():
    from sample_factory_amd.algo.learning.learner import Learner
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    img = spaces.Dict({"obs": spaces.Box(0, 255, (4, 36, 36), np.uint8)})
    vec = spaces.Dict({"obs": spaces.Box(-1.0, 1.0, (7,), np.float32)})
    model = type("M", (), dict(obs_keys=["obs"]))()
    assert Learner._augment_pad(default_cfg(env="x"), model, img) == 0
    assert Learner._augment_pad(default_cfg(env="x", augment_random_shift=4), model, img) == 4
    assert Learner._augment_pad(default_cfg(env="x", augment_random_shift=255), model, img) == 255
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="augment_random_shift"):
            Learner._augment_pad(default_cfg(env="x", augment_random_shift=bad), model, img)
    with pytest.raises(ValueError, match="no image key"):
        Learner._augment_pad(default_cfg(env="x", augment_random_shift=4), model, vec)
    from sample_factory_amd.model.torch_policy import TorchPolicyAdapter
    torch_model = TorchPolicyAdapter.__new__(TorchPolicyAdapter)
    with pytest.raises(NotImplementedError, match="torch"):
        Learner._augment_pad(default_cfg(env="x", augment_random_shift=4), torch_model, img)
    assert Learner._augment_pad(default_cfg(env="x"), torch_model, img) == 0   # flag off: nothing changes for it


def test_flag_survives_load_from_checkpoint(tmp_path):
    from sample_factory_amd.cfg.arguments import cfg_dict, load_from_checkpoint, parse_full_cfg, parse_sf_args
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=aug", "--augment_random_shift=4"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    os.makedirs(tmp_path / "aug")
    with open(tmp_path / "aug" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    assert json.load(open(tmp_path / "aug" / "config.json"))["augment_random_shift"] == 4
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=aug"]  # enjoy: the flag is not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).augment_random_shift == 4
    argv += ["--augment_random_shift=2"]  # ... and the command line still overrides the file
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).augment_random_shift == 2


def test_rollout_reuse_resolves_to_off_under_the_flag():
    """configure_keep returns before it touches the device: no kept buffers exist with the flag on"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.model.actor_critic import ActorCritic
    ac = ActorCritic.__new__(ActorCritic)
    ac.cfg = default_cfg(env="x", augment_random_shift=4, batch_size=64, num_batches_per_epoch=2, rollout=8)
    assert ac.configure_keep(16, 8, 16, 4 * 36 * 36 * 9) == 0 and ac._keep is None


# ------------------------------------------------------------------------------------------------ the draws
def test_philox_lane_five_is_free_and_documented():
    """lane 2 of the counter: sf_rl.hip uses 0 .. 3, sf_pixcatch.hip 4; the shift takes 5 and says so in the header"""
    lanes = {}
    csrc = os.path.join(ROOT, "sample_factory_amd", "csrc")
    for name in sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))):
        for m in re.finditer(r"sf_philox4x32_10\(([^;]*?)\);", open(os.path.join(csrc, name)).read(), re.S):
            args = [a.strip() for a in m.group(1).split(",")]
            if len(args) >= 7 and re.fullmatch(r"\d+u?", args[2]):
                lanes.setdefault(int(args[2].rstrip("u")), set()).add(name)
    assert lanes[5] == {"sf_augment.hip"} and lanes[4] == {"sf_pixcatch.hip"}
    assert all(lanes[k] == {"sf_rl.hip"} for k in (0, 1, 2, 3)) and set(lanes) == {0, 1, 2, 3, 4, 5}
    assert frame_ops.RANDOM_SHIFT_LANE == 5
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert "counter (draw_id, 0, 5, 0)" in text and "Counter lane 2" in text


def test_draws_cover_every_offset_evenly():
    """pad = 4, seed = 12345, draw_id 0..8, groups 0..4095: every (dy, dx) pair occurs, every marginal value's count lies
    within 10 % of 4096"""
    pad, groups = 4, np.arange(4096)
    count = np.zeros((2 * pad + 1, 2 * pad + 1), np.int64)
    for draw_id in range(9):
        dy, dx = frame_ops.random_shift_draws(12345, draw_id, groups, pad)
        assert dy.dtype == np.int32 and dx.shape == groups.shape
        assert dy.min() >= 0 and dy.max() <= 2 * pad and dx.min() >= 0 and dx.max() <= 2 * pad
        np.add.at(count, (dy, dx), 1)
    assert count.sum() == 36864 and (count > 0).all()
    for marginal in (count.sum(0), count.sum(1)):
        assert (np.abs(marginal - 4096) <= 0.10 * 4096).all(), marginal


def test_draws_depend_on_draw_id_group_and_seed_and_on_nothing_else():
    g = np.arange(512)
    base = frame_ops.random_shift_draws(7, 3, g, 4)
    again = frame_ops.random_shift_draws(7, 3, g.copy(), 4)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    for other in (frame_ops.random_shift_draws(8, 3, g, 4), frame_ops.random_shift_draws(7, 4, g, 4),
                  frame_ops.random_shift_draws(7, 3, g + 512, 4)):
        assert not np.array_equal(base[0], other[0]) and not np.array_equal(base[1], other[1])
    # a group's draw does not depend on its neighbours, the order or the shape of the query
    perm = np.random.default_rng(0).permutation(512)
    shuffled = frame_ops.random_shift_draws(7, 3, g[perm], 4)
    assert np.array_equal(shuffled[0], base[0][perm]) and np.array_equal(shuffled[1], base[1][perm])
    one = frame_ops.random_shift_draws(7, 3, np.array([137]), 4)
    assert one[0][0] == base[0][137] and one[1][0] == base[1][137]
    # draw_id and seed are read as 32-bit words; the literal formula on one block
    wrapped = frame_ops.random_shift_draws(7 + (1 << 32), 3 + (1 << 32), g, 4)
    assert np.array_equal(wrapped[0], base[0]) and np.array_equal(wrapped[1], base[1])
    from sample_factory_amd.envs.pixel_catch import philox
    w = philox(3, 0, 5, 0, 7, 137)
    assert base[1][137] == (int(w[0]) * 9) >> 32 and base[0][137] == (int(w[1]) * 9) >> 32
    # pad = 0 never moves anything; the bounds are checked
    zero = frame_ops.random_shift_draws(7, 3, g, 0)
    assert not zero[0].any() and not zero[1].any()
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="pad"):
            frame_ops.random_shift_draws(7, 3, g, bad)


def test_seed_separates_runs_policies_and_replicas():
    seeds = {frame_ops.random_shift_seed(s, p, r) for s in (None, 0, 1, 2) for p in (0, 1) for r in (0, 1, 2)}
    assert len(seeds) == 3 * 2 * 3                        # None and 0 are the same run seed
    assert all(0 <= s < 1 << 32 for s in seeds)
    assert frame_ops.random_shift_seed(5, 1) == frame_ops.random_shift_seed(5, 1, 0)


# ------------------------------------------------------------------------------------------------ the frames
@pytest.mark.parametrize("shape,dtype,pad", [((5, 3, 5, 7), np.uint8, 4), ((4, 1, 9, 13), np.uint8, 1), ((3, 2, 6, 16), np.uint8, 7),
                                             ((5, 3, 5, 7), np.float32, 4), ((2, 1, 1, 10), np.float32, 0), ((3, 2, 1, 1), np.uint8, 3)])
def test_shifted_frames_equal_pad_then_crop(shape, dtype, pad):
    rng = np.random.default_rng(sum(shape) + pad)
    frames = rng.integers(0, 256, shape).astype(dtype)
    N, _, H, W = shape
    dy, dx = rng.integers(0, 2 * pad + 1, N), rng.integers(0, 2 * pad + 1, N)
    dy[0], dx[0] = 0, 2 * pad                             # the corners of the range are there
    dy[-1], dx[-1] = 2 * pad, 0
    out = frame_ops.random_shift_frames(frames, dy, dx, pad)
    assert out.shape == frames.shape and out.dtype == frames.dtype and out.flags.c_contiguous
    for i in range(N):
        padded = np.pad(frames[i], ((0, 0), (pad, pad), (pad, pad)), mode="edge")
        assert np.array_equal(out[i], padded[:, dy[i]:dy[i] + H, dx[i]:dx[i] + W]), i
    centre = frame_ops.random_shift_frames(frames, np.full(N, pad), np.full(N, pad), pad)
    assert np.array_equal(centre, frames)                 # the draw (pad, pad) is the identity
    with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
        frame_ops.random_shift_frames(frames[0], dy[:1], dx[:1], pad)
