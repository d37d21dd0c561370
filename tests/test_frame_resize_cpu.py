"""Resize and grey-scale on the device (--device_resize / --device_grayscale, sf_frame_resize) as far as it
can be checked without a GPU: the entry point's place in the C ABI, its argument refusals (all of them come before any
launch), the three engine flags, the preprocessed observation space and EnvInfo, and the NumPy model of the arithmetic
(envs/frame_ops.py) against float64, against Pillow's integer box reduction and on hand-made cases."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

from sample_factory_amd.envs import frame_ops, spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sf_frame_resize"


def test_entry_point_is_declared_listed_and_exported_and_the_abi_version_stays():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert ENTRY in lib.SYMBOLS and re.search(r"\bint\s+" + ENTRY + r"\s*\(", text) and hasattr(L, ENTRY)
    assert callable(lib.frame_resize)
    assert len(lib.SYMBOLS) == len(set(lib.SYMBOLS))
    assert L.sf_abi_version() == 19
    assert L.sf_selftest_host() == 0   # includes the exactness of the kernel's rounding division for frame areas up to 2^23


def _p(a):
    return None if a is None else C.c_void_p(a)


def _resize(L, dst=4096, dst_pitch=1 << 16, src=1 << 20, src_pitch=1 << 12, H=8, W=8, Cn=3, hwc=1, OH=4, OW=4, interp=1, gray=0,
            rows=8):
    return getattr(L, ENTRY)(_p(dst), C.c_int64(dst_pitch), _p(src), C.c_int64(src_pitch), H, W, Cn, hwc, OH, OW, interp, gray,
                             rows, None)


def test_refusals_come_before_any_launch_and_name_the_entry_point():
    """made-up non-null addresses: each call must return -1 on a machine with no GPU"""
    from sample_factory_amd import lib
    L = lib.load()
    for kw in [dict(dst=None), dict(src=None), dict(H=0), dict(W=-1), dict(Cn=0), dict(OH=0), dict(OW=-2),
               dict(interp=2), dict(interp=-1),
               dict(OH=9), dict(OW=9), dict(OH=9, OW=9),                      # area only shrinks
               dict(gray=1, Cn=1), dict(gray=1, Cn=4), dict(gray=1, Cn=2, interp=0),
               dict(src_pitch=191),                                           # H W C = 192
               dict(dst_pitch=47), dict(gray=1, dst_pitch=15),                # C' OH OW = 48 / 16
               dict(interp=0, OH=16, OW=16, dst_pitch=767),                   # an up-scale's row is 768 bytes
               dict(rows=-1),
               dict(H=4096, W=2049, Cn=1, OH=4, OW=4, src_pitch=1 << 24)]:    # area sums are 32-bit: H W <= 2^23
        assert _resize(L, **kw) == -1, kw
        assert ENTRY in L.sf_last_error().decode(), (kw, L.sf_last_error().decode())


def test_rows_zero_is_ok_and_launches_nothing():
    from sample_factory_amd import lib
    L = lib.load()
    assert _resize(L, rows=0) == 0 and _resize(L, rows=0, gray=1, hwc=0) == 0
    assert _resize(L, rows=0, interp=0, OH=16, OW=3) == 0
    assert _resize(L, rows=0, H=4096, W=2048, Cn=1, src_pitch=1 << 23) == 0   # exactly 2^23 pixels is still served


# ------------------------------------------------------------------------------------------------ flags
def test_flags_default_to_off_and_parse():
    from sample_factory_amd.cfg.arguments import ENGINE_FLAGS, FLAGS, default_cfg, parse_full_cfg, parse_sf_args
    names = ("device_resize", "device_resize_interpolation", "device_grayscale")
    specs = {f[0]: f for f in ENGINE_FLAGS}
    assert specs["device_resize"][1:] == (int, [], "*") and specs["device_resize_interpolation"][1:] == (str, "area")
    assert specs["device_grayscale"][2] is False
    assert not set(names) & {f[0] for f in FLAGS}    # none shadows a reference flag
    cfg = default_cfg(env="x")
    assert cfg.device_resize == [] and cfg.device_resize_interpolation == "area" and cfg.device_grayscale is False
    argv = ["--env=x", "--device_resize", "84", "96", "--device_grayscale=True", "--device_resize_interpolation=nearest"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    assert cfg.device_resize == [84, 96] and cfg.device_grayscale is True and cfg.device_resize_interpolation == "nearest"
    assert cfg.cli_args["device_resize"] == [84, 96]
    off = parse_full_cfg(parser, ["--env=x"])
    assert off.device_resize == [] and "device_resize" not in off.cli_args


def test_wrong_number_of_sizes_and_unknown_filter_are_refused_at_set_up():
    from sample_factory_amd.algo.utils.env_info import EnvInfo, device_resize_of, with_device_ingest
    from sample_factory_amd.cfg.arguments import default_cfg
    info = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (3, 20, 24), np.uint8)}), spaces.Discrete(3), 8)
    env = types.SimpleNamespace()
    for bad in ([84], [84, 84, 3], [1, 2, 3, 4]):
        with pytest.raises(ValueError, match="device_resize"):
            with_device_ingest(info, env, default_cfg(env="x", device_resize=bad))
    with pytest.raises(ValueError, match="at least 1"):
        with_device_ingest(info, env, default_cfg(env="x", device_resize=[0, 8]))
    with pytest.raises(ValueError, match="device_resize_interpolation"):
        with_device_ingest(info, env, default_cfg(env="x", device_resize=[8, 8], device_resize_interpolation="cubic"))
    assert device_resize_of(default_cfg(env="x")) == (None, "area", False)
    assert device_resize_of(default_cfg(env="x", device_resize=[8, 9], device_grayscale=True)) == ((8, 9), "area", True)


def test_flags_survive_load_from_checkpoint(tmp_path):
    from sample_factory_amd.cfg.arguments import cfg_dict, load_from_checkpoint, parse_full_cfg, parse_sf_args
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=rs", "--device_resize", "84", "84", "--device_grayscale=True",
            "--device_resize_interpolation=nearest"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    os.makedirs(tmp_path / "rs")
    with open(tmp_path / "rs" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=rs"]  # enjoy: the flags are not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    loaded = load_from_checkpoint(parse_full_cfg(parser, argv))
    assert loaded.device_resize == [84, 84] and loaded.device_grayscale is True
    assert loaded.device_resize_interpolation == "nearest"
    argv += ["--device_resize", "42", "40"]  # ... and the command line still overrides the file
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).device_resize == [42, 40]


# ------------------------------------------------------------------------------------------------ spaces and EnvInfo
def test_resized_obs_space_changes_the_image_keys_only():
    low = np.full((3, 10, 12), 5, np.uint8)
    low[1] = 2
    high = np.full((3, 10, 12), 200, np.uint8)
    high[2, 4, 4] = 250
    vec, mask = spaces.Box(-1.0, 1.0, (7,), np.float32), spaces.Box(0, 1, (6,), np.uint8)
    space = spaces.Dict({"obs": spaces.Box(0, 255, (3, 210, 160), np.uint8), "aux": spaces.Box(low, high, (3, 10, 12), np.uint8),
                         "measurements": vec, "action_mask": mask})
    out = spaces.resized_obs_space(space, 8, 6, grayscale=False)
    assert out["obs"].shape == (3, 8, 6) and out["obs"].dtype == np.uint8 and out["obs"].low == 0 and out["obs"].high == 255
    assert np.ndim(out["obs"].low) == 0 and np.ndim(out["obs"].high) == 0          # scalar bounds are kept
    assert out["aux"].shape == (3, 8, 6) and out["aux"].low == 2 and out["aux"].high == 250   # array bounds: min and max
    assert out["measurements"] is vec and out["action_mask"] is mask
    assert space["obs"].shape == (3, 210, 160)                                      # the env's own space is untouched
    gray = spaces.resized_obs_space(space, 8, 6, grayscale=True)
    assert gray["obs"].shape == (1, 8, 6) and gray["aux"].shape == (1, 8, 6)
    assert spaces.resized_obs_space(spaces.Box(0, 255, (4, 9, 9), np.uint8), 3, 3, False)["obs"].shape == (4, 3, 3)
    f32 = spaces.Dict({"obs": spaces.Box(0, 255, (3, 20, 20), np.uint8), "depth": spaces.Box(0.0, 1.0, (1, 20, 20), np.float32)})
    with pytest.raises(ValueError, match="'depth'"):
        spaces.resized_obs_space(f32, 8, 8, False)
    with pytest.raises(ValueError, match="3 \\(R, G, B\\)"):
        spaces.resized_obs_space(spaces.Box(0, 255, (4, 9, 9), np.uint8), 3, 3, True)
    with pytest.raises(ValueError, match="three"):
        spaces.resized_obs_space(spaces.Dict({"obs": vec}), 3, 3, False)


def test_env_info_order_with_hwc_and_framestack_and_typed_refusals():
    from sample_factory_amd.algo.sampling.obs_ingest import ObsIngestPlan
    from sample_factory_amd.algo.utils.env_info import EnvInfo, with_device_ingest
    from sample_factory_amd.cfg.arguments import default_cfg
    info = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (90, 64, 3), np.uint8)}), spaces.Discrete(3), 8)
    chw = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (3, 90, 64), np.uint8)}), spaces.Discrete(3), 8)  # a CHW env
    env = types.SimpleNamespace()
    off = default_cfg(env="x")
    assert with_device_ingest(info, env, off) is info                               # flags off: the same object
    on = default_cfg(env="x", hwc_observations=True, device_resize=[36, 32], device_grayscale=True, device_framestack=4)
    key = ObsIngestPlan.from_cfg(info.obs_space, on, False).keys["obs"]
    out = with_device_ingest(info, env, on)
    assert key.hwc and key.native_shape[2:] + key.native_shape[:2] == (3, 90, 64)   # the resize: after hwc ...
    assert key.frame_shape == (1, 36, 32)
    assert info.obs_space["obs"].shape == (90, 64, 3)                               # the env's own EnvInfo keeps describing it
    assert (out.action_space, out.num_agents, out.frameskip) == (info.action_space, 8, info.frameskip)
    assert out.obs_space["obs"].shape == (4, 36, 32) and key.slab_shape == (4, 36, 32)   # ... and before the stack
    assert (key.hwc, key.resize, key.interp, key.gray, key.k) == (True, (36, 32), "area", True, 4)
    colour = default_cfg(env="x", hwc_observations=True, device_resize=[36, 32], device_resize_interpolation="nearest")
    assert with_device_ingest(info, env, colour).obs_space["obs"].shape == (3, 36, 32)
    alone = default_cfg(env="x", hwc_observations=True, device_grayscale=True)      # grey-scale alone keeps the size
    assert with_device_ingest(info, env, alone).obs_space["obs"].shape == (1, 90, 64)
    up = default_cfg(env="x", device_resize=[100, 64])
    with pytest.raises(ValueError, match="only shrinks"):
        with_device_ingest(chw, env, up)
    up.device_resize_interpolation = "nearest"
    assert with_device_ingest(chw, env, up).obs_space["obs"].shape == (3, 100, 64)
    f32 = EnvInfo(spaces.Dict({"obs": spaces.Box(0.0, 1.0, (3, 20, 24), np.float32)}), spaces.Discrete(3), 8)
    with pytest.raises(ValueError, match="'obs'"):
        with_device_ingest(f32, env, default_cfg(env="x", device_resize=[8, 8]))
    zero_copy = types.SimpleNamespace(step_into=lambda *a: None)
    with pytest.raises(NotImplementedError, match="step_into"):
        with_device_ingest(info, zero_copy, on)
    assert with_device_ingest(chw, zero_copy, off) is chw


# ------------------------------------------------------------------------------------------------ the NumPy model
def _float_box_average(frames, OH, OW):
    """floor(float64 box average + 0.5).  The overlap lengths are small integers, so the float64 weighted sum is exact; the
    one rounding is the division by D = H W, which returns an exact tie (v + 1/2) exactly and cannot carry any other sum
    across one: the nearest non-tie is 1 / (2 D) away"""
    H, W = frames.shape[-2:]
    wy, wx = frame_ops.area_weights(H, OH).astype(np.float64), frame_ops.area_weights(W, OW).astype(np.float64)
    mean = (wy @ frames.astype(np.float64) @ wx.T) / float(H * W)
    return np.floor(mean + 0.5).astype(np.uint8)


@pytest.mark.parametrize("geom", [((210, 160), (84, 84)), ((10, 7), (4, 3))], ids=["210x160_84x84", "10x7_4x3"])
def test_area_equals_the_float64_box_average_rounded_half_up(geom):
    (H, W), (OH, OW) = geom
    frames = np.random.default_rng(H).integers(0, 256, (6, H, W), dtype=np.uint8)
    got = frame_ops.resize_area_u8(frames, OH, OW)
    want = _float_box_average(frames, OH, OW)
    assert got.shape == (6, OH, OW) and got.dtype == np.uint8
    assert np.array_equal(got, want)


def test_area_ties_round_up_and_saturated_frames_stay_saturated():
    block = lambda *v: np.array(v, np.uint8).reshape(1, 2, 2)
    assert frame_ops.resize_area_u8(block(1, 1, 0, 0), 1, 1).item() == 1      # mean 1/2: a tie, up
    assert frame_ops.resize_area_u8(block(0, 1, 0, 0), 1, 1).item() == 0      # mean 1/4
    assert frame_ops.resize_area_u8(block(255, 254, 254, 255), 1, 1).item() == 255
    for shape, out in (((210, 160), (84, 84)), ((10, 7), (4, 3)), ((97, 5), (3, 5))):
        assert (frame_ops.resize_area_u8(np.full((2,) + shape, 255, np.uint8), *out) == 255).all()
        assert (frame_ops.resize_area_u8(np.zeros((2,) + shape, np.uint8), *out) == 0).all()
    with pytest.raises(ValueError, match="only shrinks"):
        frame_ops.resize_area_u8(np.zeros((4, 4), np.uint8), 5, 4)
    with pytest.raises(ValueError, match="u8"):
        frame_ops.resize_area_u8(np.zeros((4, 4), np.float32), 2, 2)


def test_area_weights_are_the_overlaps():
    w = frame_ops.area_weights(10, 4)   # destination pixel = 10 units, source pixel = 4 units
    assert w.shape == (4, 10) and (w.sum(1) == 10).all() and (w.sum(0) == 4).all()
    assert w[0].tolist() == [4, 4, 2, 0, 0, 0, 0, 0, 0, 0] and w[1].tolist() == [0, 0, 2, 4, 4, 0, 0, 0, 0, 0]
    assert np.array_equal(frame_ops.area_weights(6, 6), 6 * np.eye(6, dtype=np.int64))


def test_area_equals_pillow_reduce():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for (H, W), f, tol in (((210, 160), 2, 0), ((120, 160), 4, 0), ((210, 159), 3, 1)):
        frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
        want = np.asarray(Image.fromarray(frame, "L").reduce(f))
        got = frame_ops.resize_area_u8(frame, H // f, W // f)
        assert got.shape == want.shape
        assert np.abs(got.astype(int) - want.astype(int)).max() <= tol, (H, W, f)


def test_nearest_indices():
    frame = np.arange(4 * 4, dtype=np.uint8).reshape(4, 4)
    up = frame_ops.resize_nearest_u8(frame, 9, 7)
    assert up.shape == (9, 7)
    for y in range(9):
        for x in range(7):
            assert up[y, x] == frame[(y * 4) // 9, (x * 4) // 7]
    down = frame_ops.resize_nearest_u8(np.arange(10 * 7, dtype=np.uint8).reshape(1, 10, 7), 4, 3)
    assert down[0].tolist() == [[0, 2, 4], [14, 16, 18], [35, 37, 39], [49, 51, 53]]   # rows 0, 2, 5, 7; columns 0, 2, 4


def test_gray_values():
    px = lambda r, g, b: frame_ops.rgb_to_gray_u8(np.array([r, g, b], np.uint8).reshape(3, 1, 1)).item()
    assert px(255, 255, 255) == 255 and px(255, 0, 0) == 76 and px(0, 0, 0) == 0
    assert px(0, 255, 0) == 150 and px(0, 0, 255) == 29
    assert frame_ops.GRAY_R + frame_ops.GRAY_G + frame_ops.GRAY_B == 1 << frame_ops.GRAY_SHIFT
    assert frame_ops.rgb_to_gray_u8(np.zeros((5, 3, 4, 6), np.uint8)).shape == (5, 1, 4, 6)
    assert frame_ops.rgb_to_gray_u8(np.zeros((5, 4, 6, 3), np.uint8), -1).shape == (5, 4, 6, 1)
    with pytest.raises(ValueError, match="3 channels"):
        frame_ops.rgb_to_gray_u8(np.zeros((4, 4, 6), np.uint8))


def test_preprocess_frames_layouts_order_and_identity():
    rng = np.random.default_rng(3)
    hwc = rng.integers(0, 256, (5, 10, 7, 3), dtype=np.uint8)
    chw = np.ascontiguousarray(hwc.transpose(0, 3, 1, 2))
    for interp in frame_ops.INTERPOLATIONS:
        # identity geometry returns the input, CHW; both layouts agree
        assert np.array_equal(frame_ops.preprocess_frames(hwc, "hwc", 10, 7, interp), chw)
        assert np.array_equal(frame_ops.preprocess_frames(chw, "chw", 10, 7, interp), chw)
        a = frame_ops.preprocess_frames(hwc, "hwc", 4, 3, interp, grayscale=True)
        b = frame_ops.preprocess_frames(chw, "chw", 4, 3, interp, grayscale=True)
        assert a.shape == (5, 1, 4, 3) and a.flags.c_contiguous and np.array_equal(a, b)
        # resize first, then grey, on the rounded channels
        resize = frame_ops.resize_area_u8 if interp == "area" else frame_ops.resize_nearest_u8
        assert np.array_equal(a, frame_ops.rgb_to_gray_u8(resize(chw, 4, 3), 1))
    assert np.array_equal(frame_ops.preprocess_frames(hwc, "hwc", 10, 7, "area", True), frame_ops.rgb_to_gray_u8(chw, 1))
    with pytest.raises(ValueError, match="interpolation"):
        frame_ops.preprocess_frames(hwc, "hwc", 4, 3, "cubic")
    with pytest.raises(ValueError, match="3 channels"):
        frame_ops.preprocess_frames(hwc[..., :2], "hwc", 4, 3, "area", True)
    with pytest.raises(ValueError, match="layout"):
        frame_ops.preprocess_frames(hwc, "nhwc", 4, 3)
