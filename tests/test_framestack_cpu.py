"""The device frame stack (--device_framestack, sf_framestack_step) as far as it can be checked without a GPU: the entry
point's place in the C ABI, its argument refusals (all of them come before any launch), the stacked observation space and
the engine flag."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from sample_factory_amd.envs import spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sf_framestack_step"


def test_entry_point_is_declared_listed_and_exported_and_the_abi_version_stays():
    from sample_factory_amd import build, lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert ENTRY in lib.SYMBOLS and re.search(r"\bint\s+" + ENTRY + r"\s*\(", text) and hasattr(L, ENTRY)
    assert callable(lib.framestack_step)
    assert "sf_ingest.hip" in [s for s, _ in build.SOURCES]
    assert L.sf_abi_version() == 19


def _call(L, next_=4096, next_pitch=1 << 16, prev=8192, prev_pitch=1 << 16, frame=None, frame_pitch=0, frame_bytes=64, k=4,
          term=None, trunc=None, rows=8):
    p = lambda a: None if a is None else C.c_void_p(a)
    return getattr(L, ENTRY)(p(next_), C.c_int64(next_pitch), p(prev), C.c_int64(prev_pitch), p(frame),
                             C.c_int64(frame_pitch), C.c_int64(frame_bytes), k, p(term), p(trunc), rows, None)


def test_refusals_come_before_any_launch_and_name_the_entry_point():
    """made-up non-null addresses: each call must return -1 on a machine with no GPU"""
    from sample_factory_amd import lib
    L = lib.load()
    err = lambda: L.sf_last_error().decode()
    bad = [
        dict(next_=None), dict(prev=None),
        dict(k=0), dict(k=-1), dict(k=17),
        dict(frame_bytes=0), dict(frame_bytes=-16),
        dict(next_pitch=255), dict(prev_pitch=255),          # k * frame_bytes = 256
        dict(frame=1 << 20, frame_pitch=63),
        dict(rows=-1),
        dict(prev=4096),                                     # the same rows
        dict(prev=4096 + 255),                               # one byte shared inside a row
        dict(prev=4096 - 255),
        dict(prev=4096 + (1 << 16) + 100),                   # interleaved columns of one slab that touch
        dict(prev=4096 + 3 * (1 << 16) - 10),
        dict(prev=4096 - 300, prev_pitch=(1 << 16) + 16),    # different pitches inside one range: rows 3.. meet
    ]
    for kw in bad:
        assert _call(L, **kw) == -1, kw
        assert ENTRY in err(), (kw, err())


def test_rows_zero_is_ok_and_launches_nothing():
    from sample_factory_amd import lib
    L = lib.load()
    assert _call(L, rows=0) == 0
    assert _call(L, rows=0, frame=1 << 20, frame_pitch=64, term=64, trunc=128) == 0


def test_stacked_obs_space_stacks_the_image_keys_only():
    low = np.zeros((2, 5, 4), np.float32)
    low[1] = -1.0
    high = np.full((2, 5, 4), 3.0, np.float32)
    vec, mask = spaces.Box(-1.0, 1.0, (7,), np.float32), spaces.Box(0, 1, (6,), np.uint8)
    space = spaces.Dict({"obs": spaces.Box(0, 255, (1, 84, 84), np.uint8), "depth": spaces.Box(low, high, (2, 5, 4), np.float32),
                         "measurements": vec, "action_mask": mask})
    st = spaces.stacked_obs_space(space, 4)
    assert sorted(st.keys()) == sorted(space.keys())
    assert st["obs"].shape == (4, 84, 84) and st["obs"].dtype == np.uint8 and st["obs"].low == 0 and st["obs"].high == 255
    assert st["depth"].shape == (8, 5, 4) and st["depth"].dtype == np.float32
    assert np.array_equal(st["depth"].low, np.concatenate([low] * 4)) and st["depth"].low.dtype == np.float32
    assert np.array_equal(st["depth"].high, np.concatenate([high] * 4))
    assert st["measurements"] is vec and st["action_mask"] is mask
    assert space["obs"].shape == (1, 84, 84) and space["depth"].shape == (2, 5, 4)  # the env's own space is untouched
    assert spaces.stacked_obs_space(space, 1) is space
    assert spaces.stacked_obs_space(space, 2)["obs"].shape == (2, 84, 84)
    # a 3-D action mask would still not be stacked; a bare Box is treated as Dict(obs=...)
    assert spaces.stacked_obs_space(spaces.Box(0, 255, (3, 6, 6), np.uint8), 2)["obs"].shape == (6, 6, 6)
    with pytest.raises(ValueError, match="device_framestack=0"):
        spaces.stacked_obs_space(space, 0)
    with pytest.raises(ValueError, match="three dimensions"):
        spaces.stacked_obs_space(spaces.Dict({"obs": vec, "action_mask": spaces.Box(0, 1, (1, 2, 3), np.uint8)}), 4)


def test_env_info_for_the_engine_is_a_stacked_copy_and_refusals_are_typed():
    import types

    from sample_factory_amd.algo.utils.env_info import EnvInfo, with_device_ingest
    from sample_factory_amd.cfg.arguments import default_cfg
    info = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (1, 12, 12), np.uint8)}), spaces.Discrete(3), 8)
    env = types.SimpleNamespace()
    assert with_device_ingest(info, env, default_cfg(env="x")) is info
    out = with_device_ingest(info, env, default_cfg(env="x", device_framestack=4))
    assert out.obs_space["obs"].shape == (4, 12, 12) and info.obs_space["obs"].shape == (1, 12, 12)
    assert (out.action_space, out.num_agents, out.frameskip) == (info.action_space, 8, info.frameskip)
    with pytest.raises(ValueError):
        with_device_ingest(info, env, default_cfg(env="x", device_framestack=0))
    vec_info = EnvInfo(spaces.Dict({"obs": spaces.Box(-1, 1, (5,), np.float32)}), spaces.Discrete(3), 8)
    with pytest.raises(ValueError):
        with_device_ingest(vec_info, env, default_cfg(env="x", device_framestack=2))
    zero_copy = types.SimpleNamespace(step_into=lambda *a: None)
    with pytest.raises(NotImplementedError, match="step_into"):
        with_device_ingest(info, zero_copy, default_cfg(env="x", device_framestack=2))
    assert with_device_ingest(info, zero_copy, default_cfg(env="x")) is info


def test_flag_defaults_to_one_and_parses():
    from sample_factory_amd.cfg.arguments import ENGINE_FLAGS, FLAGS, default_cfg, parse_full_cfg, parse_sf_args
    assert ("device_framestack", 1) in [(f[0], f[2]) for f in ENGINE_FLAGS]
    assert "device_framestack" not in [f[0] for f in FLAGS]
    assert default_cfg(env="x").device_framestack == 1
    parser, _ = parse_sf_args(["--env=x", "--device_framestack=4"])
    cfg = parse_full_cfg(parser, ["--env=x", "--device_framestack=4"])
    assert cfg.device_framestack == 4 and cfg.env_framestack == 1
    assert parse_full_cfg(parser, ["--env=x"]).device_framestack == 1


def test_flag_survives_load_from_checkpoint(tmp_path):
    from sample_factory_amd.cfg.arguments import cfg_dict, load_from_checkpoint, parse_full_cfg, parse_sf_args
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=fs", "--device_framestack=4"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    os.makedirs(tmp_path / "fs")
    with open(tmp_path / "fs" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=fs"]  # enjoy: the flag is not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    loaded = load_from_checkpoint(parse_full_cfg(parser, argv))
    assert loaded.device_framestack == 4
    argv.append("--device_framestack=2")  # ... and the command line still overrides the file
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).device_framestack == 2
