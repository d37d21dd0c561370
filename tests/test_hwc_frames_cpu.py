"""Channel-last image observations (--hwc_observations, sf_hwc_to_chw, sf_framestack_step_hwc) as far as
they can be checked without a GPU: the two entry points' place in the C ABI, their argument refusals (all of them come
before any launch), the CHW view of an HWC observation space, the engine flag and the channel-last test env."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

from sample_factory_amd.envs import spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSPOSE, STACK = "sf_hwc_to_chw", "sf_framestack_step_hwc"


def test_entry_points_are_declared_listed_and_exported_and_the_abi_version_stays():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    for entry in (TRANSPOSE, STACK):
        assert entry in lib.SYMBOLS and re.search(r"\bint\s+" + entry + r"\s*\(", text) and hasattr(L, entry)
    assert callable(lib.hwc_to_chw) and callable(lib.framestack_step_hwc)
    assert len(lib.SYMBOLS) == len(set(lib.SYMBOLS))
    assert L.sf_abi_version() == 19


def _p(a):
    return None if a is None else C.c_void_p(a)


def _transpose(L, dst=4096, dst_pitch=1 << 16, src=1 << 20, src_pitch=1 << 12, H=8, W=8, Cn=3, eb=1, rows=8):
    return getattr(L, TRANSPOSE)(_p(dst), C.c_int64(dst_pitch), _p(src), C.c_int64(src_pitch), H, W, Cn, eb, rows, None)


def _stack(L, next_=4096, next_pitch=1 << 16, prev=8192, prev_pitch=1 << 16, frame=1 << 20, frame_pitch=1 << 12, H=8, W=8,
           Cn=1, eb=1, k=4, term=None, trunc=None, rows=8):
    return getattr(L, STACK)(_p(next_), C.c_int64(next_pitch), _p(prev), C.c_int64(prev_pitch), _p(frame),
                             C.c_int64(frame_pitch), H, W, Cn, eb, k, _p(term), _p(trunc), rows, None)


def test_refusals_come_before_any_launch_and_name_the_entry_point():
    """made-up non-null addresses: each call must return -1 on a machine with no GPU"""
    from sample_factory_amd import lib
    L = lib.load()
    err = lambda: L.sf_last_error().decode()
    for kw in [dict(dst=None), dict(src=None), dict(eb=0), dict(eb=2), dict(eb=8), dict(Cn=0), dict(Cn=-3), dict(H=0),
               dict(W=-1), dict(dst_pitch=191), dict(src_pitch=191),     # a row is 8 * 8 * 3 = 192 bytes
               dict(eb=4, src_pitch=767), dict(rows=-1)]:
        assert _transpose(L, **kw) == -1, kw
        assert TRANSPOSE in err() and STACK not in err(), (kw, err())
    for kw in [dict(next_=None), dict(prev=None), dict(frame=None), dict(eb=0), dict(eb=2), dict(Cn=0), dict(H=0),
               dict(k=0), dict(k=-1), dict(k=17),
               dict(next_pitch=255), dict(prev_pitch=255),               # k * frame_bytes = 256
               dict(frame_pitch=63), dict(eb=4, frame_pitch=255), dict(rows=-1),
               dict(prev=4096),                                          # the same rows
               dict(prev=4096 + 255), dict(prev=4096 - 255),             # one byte shared inside a row
               dict(prev=4096 + (1 << 16) + 100),                        # interleaved columns of one slab that touch
               dict(prev=4096 - 300, prev_pitch=(1 << 16) + 16)]:        # different pitches inside one range
        assert _stack(L, **kw) == -1, kw
        assert STACK in err(), (kw, err())


def test_rows_zero_is_ok_and_launches_nothing():
    from sample_factory_amd import lib
    L = lib.load()
    assert _transpose(L, rows=0) == 0 and _transpose(L, rows=0, eb=4, dst_pitch=768, src_pitch=768) == 0
    assert _stack(L, rows=0) == 0 and _stack(L, rows=0, term=64, trunc=128) == 0


def _hwc_space():
    low = np.zeros((5, 4, 2), np.float32)
    low[..., 1] = -1.0
    high = np.arange(40, dtype=np.float32).reshape(5, 4, 2)
    vec, mask = spaces.Box(-1.0, 1.0, (7,), np.float32), spaces.Box(0, 1, (6,), np.uint8)
    return spaces.Dict({"obs": spaces.Box(0, 255, (84, 72, 3), np.uint8), "depth": spaces.Box(low, high, (5, 4, 2), np.float32),
                        "measurements": vec, "action_mask": mask}), low, high, vec, mask


def test_chw_obs_space_transposes_the_image_keys_only():
    space, low, high, vec, mask = _hwc_space()
    chw = spaces.chw_obs_space(space)
    assert sorted(chw.keys()) == sorted(space.keys())
    assert chw["obs"].shape == (3, 84, 72) and chw["obs"].dtype == np.uint8 and chw["obs"].low == 0 and chw["obs"].high == 255
    assert np.ndim(chw["obs"].low) == 0 and np.ndim(chw["obs"].high) == 0   # scalar bounds stay scalar
    assert chw["depth"].shape == (2, 5, 4) and chw["depth"].dtype == np.float32
    assert np.array_equal(chw["depth"].low, low.transpose(2, 0, 1)) and chw["depth"].low.dtype == np.float32
    assert np.array_equal(chw["depth"].high, high.transpose(2, 0, 1)) and chw["depth"].high[1, 2, 3] == high[2, 3, 1]
    assert chw["measurements"] is vec and chw["action_mask"] is mask
    assert space["obs"].shape == (84, 72, 3) and space["depth"].shape == (5, 4, 2)  # the env's own space is untouched
    # the key rule is framestack_keys': a 3-D action mask is not an image; a bare Box is treated as Dict(obs=...)
    assert sorted(spaces.framestack_keys(space)) == ["depth", "obs"]
    assert spaces.chw_obs_space(spaces.Box(0, 255, (6, 7, 3), np.uint8))["obs"].shape == (3, 6, 7)
    with pytest.raises(ValueError, match="three dimensions"):
        spaces.chw_obs_space(spaces.Dict({"obs": vec, "action_mask": spaces.Box(0, 1, (1, 2, 3), np.uint8)}))
    with pytest.raises(ValueError, match="hwc_observations"):
        spaces.chw_obs_space(vec)


def test_the_frame_stack_composes_along_the_channels_of_the_chw_space():
    space, low, high, _, _ = _hwc_space()
    st = spaces.stacked_obs_space(spaces.chw_obs_space(space), 4)
    assert st["obs"].shape == (12, 84, 72) and st["obs"].dtype == np.uint8
    assert st["depth"].shape == (8, 5, 4) and np.array_equal(st["depth"].high, np.concatenate([high.transpose(2, 0, 1)] * 4))
    assert st["measurements"] is space["measurements"] and st["action_mask"] is space["action_mask"]


def test_env_info_for_the_engine_is_a_chw_copy_and_refusals_are_typed():
    from sample_factory_amd.algo.sampling.obs_ingest import ObsIngestPlan
    from sample_factory_amd.algo.utils.env_info import EnvInfo, with_device_ingest
    from sample_factory_amd.cfg.arguments import default_cfg
    info = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (20, 24, 3), np.uint8)}), spaces.Discrete(3), 8)
    env = types.SimpleNamespace()
    assert with_device_ingest(info, env, default_cfg(env="x")) is info
    alone = with_device_ingest(info, env, default_cfg(env="x", hwc_observations=True))
    assert alone.obs_space["obs"].shape == (3, 20, 24) and info.obs_space["obs"].shape == (20, 24, 3)
    on = default_cfg(env="x", hwc_observations=True, device_framestack=4)
    out = with_device_ingest(info, env, on)
    key = ObsIngestPlan.from_cfg(info.obs_space, on, False).keys["obs"]
    assert key.hwc and key.native_shape == (20, 24, 3) and key.frame_shape == (3, 20, 24)   # one frame, transposed
    assert (out.action_space, out.num_agents, out.frameskip) == (info.action_space, 8, info.frameskip)
    assert out.obs_space["obs"].shape == (12, 20, 24) and key.slab_shape == (12, 20, 24)  # transposed before the stack
    vec_info = EnvInfo(spaces.Dict({"obs": spaces.Box(-1, 1, (5,), np.float32)}), spaces.Discrete(3), 8)
    with pytest.raises(ValueError, match="three dimensions"):
        with_device_ingest(vec_info, env, on)
    zero_copy = types.SimpleNamespace(step_into=lambda *a: None)
    with pytest.raises(NotImplementedError, match="step_into"):
        with_device_ingest(info, zero_copy, on)
    assert with_device_ingest(info, zero_copy, default_cfg(env="x")) is info


def test_flag_defaults_to_off_and_parses():
    from sample_factory_amd.cfg.arguments import ENGINE_FLAGS, FLAGS, default_cfg, parse_full_cfg, parse_sf_args
    assert ("hwc_observations", False) in [(f[0], f[2]) for f in ENGINE_FLAGS]
    assert "hwc_observations" not in [f[0] for f in FLAGS]
    assert default_cfg(env="x").hwc_observations is False
    parser, _ = parse_sf_args(["--env=x", "--hwc_observations=True"])
    cfg = parse_full_cfg(parser, ["--env=x", "--hwc_observations=True"])
    assert cfg.hwc_observations is True and cfg.pixel_format == "CHW"   # the reference's env-factory flag is not touched
    assert parse_full_cfg(parser, ["--env=x"]).hwc_observations is False


def test_flag_survives_load_from_checkpoint(tmp_path):
    from sample_factory_amd.cfg.arguments import cfg_dict, load_from_checkpoint, parse_full_cfg, parse_sf_args
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=hwc", "--hwc_observations=True"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    os.makedirs(tmp_path / "hwc")
    with open(tmp_path / "hwc" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=hwc"]  # enjoy: the flag is not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).hwc_observations is True
    argv.append("--hwc_observations=False")  # ... and the command line still overrides the file
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).hwc_observations is False


def test_host_frame_env_serves_the_same_ring_channel_last():
    from sample_factory_amd.envs.synthetic import HostFrameVecEnv, make_host_frame_env
    kw = dict(num_agents=5, obs_shape=(3, 6, 8), seed=3)
    chw, hwc, again = HostFrameVecEnv(**kw), HostFrameVecEnv(hwc=True, **kw), HostFrameVecEnv(hwc=False, **kw)
    assert chw.observation_space["obs"].shape == (3, 6, 8) and hwc.observation_space["obs"].shape == (6, 8, 3)
    assert hwc.ring.shape == (4, 5, 6, 8, 3) and hwc.ring.flags.c_contiguous and hwc.ring.dtype == np.uint8
    a, b, c = chw.reset()[0]["obs"], hwc.reset()[0]["obs"], again.reset()[0]["obs"]
    for step in range(6):  # once round the ring and on
        assert b.shape == (5, 6, 8, 3) and b.flags.c_contiguous
        assert np.array_equal(b, a.transpose(0, 2, 3, 1)) and np.array_equal(a, c), step
        acts = np.full(5, step % 6)
        (oa, ra, ta, ua, _), (ob, rb, tb, ub, _), (oc, rc, tc, uc, _) = chw.step(acts), hwc.step(acts), again.step(acts)
        assert np.array_equal(ra, rb) and np.array_equal(ta, tb) and np.array_equal(ua, ub)
        assert np.array_equal(ra, rc) and np.array_equal(ta, tc)
        a, b, c = oa["obs"], ob["obs"], oc["obs"]
    # the factory: cfg.host_env_hwc, off unless asked for
    cfg = types.SimpleNamespace(synthetic_num_agents=5, seed=3, host_env_obs_shape=(3, 6, 8))
    assert np.array_equal(make_host_frame_env("e", cfg).ring, chw.ring)
    cfg.host_env_hwc = True
    assert np.array_equal(make_host_frame_env("e", cfg).ring, hwc.ring)
