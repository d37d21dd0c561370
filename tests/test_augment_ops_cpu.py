"""Cutout and intensity augmentation (--augment_cutout, --augment_intensity, --augment_mix, sf_augment_gather; DESIGN.md
3.20) as far as it can be checked without a GPU: the entry point's place in the C ABI, its argument refusals (all of them come
before any launch), the engine flags, and the NumPy model (envs/frame_ops.py): the distribution of the draws, what they
depend on, the arithmetic against literal formulas, and the one fixed order of the stages."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from sample_factory_amd.envs import frame_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sf_augment_gather"


def test_entry_point_is_declared_listed_and_exported_and_the_abi_version_stays():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert ENTRY in lib.SYMBOLS and re.search(r"\bint\s+" + ENTRY + r"\s*\(", text) and hasattr(L, ENTRY)
    assert "sf_random_shift_gather" in lib.SYMBOLS and hasattr(L, "sf_random_shift_gather")   # the old entry stays
    assert callable(lib.augment_gather) and callable(lib.random_shift_gather)
    assert len(lib.SYMBOLS) == len(set(lib.SYMBOLS))
    assert L.sf_abi_version() == 19


def _p(a):
    return None if a is None else C.c_void_p(a)


def _gather(L, dst=4096, dst_pitch=1 << 12, src=1 << 20, src_pitch=1 << 12, index=None, offset=0, n=8, traj_T=4, Cn=3, H=8, W=8,
            eb=1, pad=4, cut_min=2, cut_max=5, fill=0, amp=64, rec=1, seed=1, draw=0):
    return getattr(L, ENTRY)(_p(dst), C.c_int64(dst_pitch), _p(src), C.c_int64(src_pitch), _p(index), C.c_int64(offset),
                             C.c_int64(n), traj_T, Cn, H, W, eb, pad, cut_min, cut_max, fill, amp, rec, C.c_uint32(seed),
                             C.c_uint32(draw), None)


def test_refusals_come_before_any_launch_and_name_the_entry_point():
    """made-up non-null addresses: each call must return -1 on a machine with no GPU"""
    from sample_factory_amd import lib
    L = lib.load()
    for kw in [dict(dst=None), dict(src=None), dict(n=-1), dict(pad=-1), dict(pad=256), dict(eb=0), dict(eb=2), dict(eb=8),
               dict(rec=0), dict(rec=-3), dict(H=0), dict(W=0), dict(Cn=0), dict(H=-2), dict(W=-1), dict(Cn=-1),
               dict(dst_pitch=191), dict(src_pitch=191),                      # C H W = 192
               dict(eb=4, dst_pitch=767), dict(eb=4, src_pitch=767),          # C H W elem_bytes = 768
               dict(traj_T=-1), dict(offset=-1),                              # ... the old entry's refusals, and the new ones:
               dict(cut_min=0), dict(cut_min=-1), dict(cut_min=6), dict(cut_min=1, cut_max=65536), dict(cut_max=-1),
               dict(amp=-1), dict(amp=256), dict(fill=1, eb=4), dict(fill=2), dict(fill=-1),
               dict(fill=1, eb=4, cut_max=0, cut_min=0)]:                     # a random byte is no f32 value, cutout on or off
        assert _gather(L, **kw) == -1, kw
        assert ENTRY in L.sf_last_error().decode(), (kw, L.sf_last_error().decode())


def test_n_zero_is_ok_and_launches_nothing():
    from sample_factory_amd import lib
    L = lib.load()
    assert _gather(L, n=0) == 0 and _gather(L, n=0, pad=0, eb=4, index=1 << 16) == 0
    assert _gather(L, n=0, pad=255, cut_min=65535, cut_max=65535, fill=1, amp=255, dst_pitch=192, src_pitch=192) == 0
    assert _gather(L, n=0, cut_min=0, cut_max=0, amp=0) == 0   # cut_max = 0 is "off": cut_min is not looked at
    assert _gather(L, n=0, cut_min=-7, cut_max=0) == 0
    assert _gather(L, n=-1, cut_max=0) == -1                   # ... and n is still checked first


# ------------------------------------------------------------------------------------------------ the flags
def _argv_cfg(argv):
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    parser, _ = parse_sf_args(argv)
    return parse_full_cfg(parser, argv)


OK = dict(env="x", num_workers=1, num_envs_per_worker=2, rollout=4, batch_size=8, num_batches_per_epoch=1, use_rnn=False,
          recurrence=1)


def test_flags_default_to_off_and_parse():
    from sample_factory_amd.cfg.arguments import ENGINE_FLAGS, FLAGS, augment_ops, default_cfg
    specs = {f[0]: f for f in ENGINE_FLAGS}
    assert specs["augment_cutout"][1:] == (int, [], "*") and specs["augment_cutout_fill"][1:] == (str, "zero")
    assert specs["augment_intensity"][1:] == (int, 0) and specs["augment_mix"][1:] == (str, "all")
    assert not {"augment_cutout", "augment_cutout_fill", "augment_intensity", "augment_mix"} & {f[0] for f in FLAGS}
    d = default_cfg(env="x")
    assert (d.augment_cutout, d.augment_cutout_fill, d.augment_intensity, d.augment_mix) == ([], "zero", 0, "all")
    off = augment_ops(d)
    assert (off.pad, off.cutout, off.cutout_fill, off.intensity, off.mix, off.enabled) == (0, (), "zero", 0, "all", [])
    cfg = _argv_cfg(["--env=x", "--augment_cutout", "4", "12", "--augment_cutout_fill=random", "--augment_intensity=64",
                     "--augment_mix=one", "--augment_random_shift=4"])
    assert cfg.augment_cutout == [4, 12] and cfg.cli_args["augment_cutout"] == [4, 12]
    on = augment_ops(cfg)
    assert (on.pad, on.cutout, on.cutout_fill, on.intensity, on.mix) == (4, (4, 12), "random", 64, "one")
    assert on.enabled == ["shift", "cutout", "intensity"]
    assert augment_ops(default_cfg(env="x", augment_intensity=1)).enabled == ["intensity"]
    assert "augment_cutout" not in _argv_cfg(["--env=x"]).cli_args


def test_verify_cfg_and_the_helper_refuse_bad_values():
    from sample_factory_amd.cfg.arguments import augment_ops, default_cfg, verify_cfg
    info = type("I", (), dict(num_agents=1))()
    for good in (dict(), dict(augment_cutout=[1, 1]), dict(augment_cutout=[4, 65535], augment_cutout_fill="random"),
                 dict(augment_intensity=255), dict(augment_mix="one"), dict(augment_cutout=[2, 5], augment_intensity=3, augment_mix="one"),
                 dict(augment_cutout=[2, 5], augment_consistency_coeff=0.1),           # DrAC no longer needs the shift
                 dict(augment_intensity=8, augment_consistency_coeff=0.1)):
        assert verify_cfg(default_cfg(**good, **OK), info), good
    for bad, word in ((dict(augment_cutout=[4]), "augment_cutout"), (dict(augment_cutout=[1, 2, 3]), "augment_cutout"),
                      (dict(augment_cutout=[0, 4]), "augment_cutout"), (dict(augment_cutout=[5, 4]), "augment_cutout"),
                      (dict(augment_cutout=[1, 65536]), "augment_cutout"), (dict(augment_cutout_fill="mean"), "augment_cutout_fill"),
                      (dict(augment_intensity=-1), "augment_intensity"), (dict(augment_intensity=256), "augment_intensity"),
                      (dict(augment_mix="some"), "augment_mix"), (dict(augment_random_shift=256), "augment_random_shift")):
        assert not verify_cfg(default_cfg(**bad, **OK), info), bad
        with pytest.raises(ValueError, match=word):
            augment_ops(default_cfg(**bad, **OK))
    assert not verify_cfg(default_cfg(augment_consistency_coeff=0.1, **OK), info)      # nothing to be consistent with
    with pytest.raises(NotImplementedError, match="mask_actions_in_loss"):
        verify_cfg(default_cfg(augment_cutout=[2, 5], augment_consistency_coeff=0.1, mask_actions_in_loss=True, **OK), info)


def test_flags_survive_load_from_checkpoint(tmp_path):
    from sample_factory_amd.cfg.arguments import cfg_dict, load_from_checkpoint, parse_full_cfg, parse_sf_args
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=aug", "--augment_cutout", "4", "12", "--augment_cutout_fill=random",
            "--augment_intensity=64", "--augment_mix=one"]
    cfg = _argv_cfg(argv)
    os.makedirs(tmp_path / "aug")
    with open(tmp_path / "aug" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    saved = json.load(open(tmp_path / "aug" / "config.json"))
    assert (saved["augment_cutout"], saved["augment_cutout_fill"], saved["augment_intensity"], saved["augment_mix"]) == \
        ([4, 12], "random", 64, "one")
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=aug"]  # enjoy: the flags are not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    loaded = load_from_checkpoint(parse_full_cfg(parser, argv))
    assert (loaded.augment_cutout, loaded.augment_cutout_fill, loaded.augment_intensity, loaded.augment_mix) == \
        ([4, 12], "random", 64, "one")
    argv += ["--augment_intensity=2", "--augment_cutout", "1", "3"]  # ... and the command line still overrides the file
    over = load_from_checkpoint(parse_full_cfg(parser, argv))
    assert over.augment_intensity == 2 and over.augment_cutout == [1, 3]


def test_learner_refuses_a_model_it_cannot_augment_and_a_random_fill_on_f32():
    from sample_factory_amd.algo.learning.learner import Learner
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    img = spaces.Dict({"obs": spaces.Box(0, 255, (4, 36, 36), np.uint8)})
    imgf = spaces.Dict({"obs": spaces.Box(0.0, 1.0, (4, 36, 36), np.float32)})
    vec = spaces.Dict({"obs": spaces.Box(-1.0, 1.0, (7,), np.float32)})
    model = type("M", (), dict(obs_keys=["obs"]))()
    assert Learner._augment_plan(default_cfg(env="x"), model, img) is None
    assert Learner._augment_plan(default_cfg(env="x", augment_random_shift=4), model, img) is None   # the shift keeps its launch
    plan = Learner._augment_plan(default_cfg(env="x", augment_random_shift=4, augment_cutout=[4, 12]), model, img)
    assert (plan.pad, plan.cutout, plan.intensity, plan.enabled) == (4, (4, 12), 0, ["shift", "cutout"])
    assert Learner._augment_plan(default_cfg(env="x", augment_intensity=9), model, imgf).intensity == 9
    assert Learner._augment_plan(default_cfg(env="x", augment_cutout=[4, 12]), model, imgf).cutout == (4, 12)  # zero fill on f32
    with pytest.raises(ValueError, match="augment_cutout_fill=random"):
        Learner._augment_plan(default_cfg(env="x", augment_cutout=[4, 12], augment_cutout_fill="random"), model, imgf)
    assert Learner._augment_plan(default_cfg(env="x", augment_cutout=[4, 12], augment_cutout_fill="random"), model, img)
    for on in (dict(augment_cutout=[4, 12]), dict(augment_intensity=4)):
        with pytest.raises(ValueError, match="no image key"):
            Learner._augment_plan(default_cfg(env="x", **on), model, vec)
        from sample_factory_amd.model.torch_policy import TorchPolicyAdapter
        torch_model = TorchPolicyAdapter.__new__(TorchPolicyAdapter)
        with pytest.raises(NotImplementedError, match="torch"):
            Learner._augment_plan(default_cfg(env="x", **on), torch_model, img)
    assert Learner._augment_plan(default_cfg(env="x"), torch_model, img) is None   # flags off: nothing changes for it
    learner = Learner.__new__(Learner)                                             # bad values: before the device is touched
    learner.cfg = default_cfg(augment_cutout=[5, 4], **OK)
    learner.env_info = type("I", (), dict(obs_space=None))()
    with pytest.raises(ValueError, match="augment_cutout"):
        learner.init()


def test_mix_one_zeroes_the_ops_that_were_not_drawn():
    from sample_factory_amd.algo.learning.learner import Learner
    from sample_factory_amd.cfg.arguments import augment_ops, default_cfg
    learner = Learner.__new__(Learner)
    learner._shift_seed, learner._shift_pad = 77, 4
    learner._aug_ops = None
    learner.train_step = 0
    assert learner._step_augmentation() is None and learner._augments()           # the shift alone: its own launch
    learner._aug_ops = augment_ops(default_cfg(env="x", augment_random_shift=4, augment_cutout=[4, 12], augment_intensity=64))
    assert learner._step_augmentation() == dict(pad=4, cutout=(4, 12), cutout_fill="zero", intensity=64)
    learner._aug_ops = augment_ops(default_cfg(env="x", augment_random_shift=4, augment_cutout=[4, 12], augment_intensity=64,
                                               augment_mix="one"))
    seen = set()
    for step in range(24):
        learner.train_step = step
        p = learner._step_augmentation()
        op = frame_ops.augment_op_of_step(77, step, ["shift", "cutout", "intensity"])
        assert p == dict(pad=4 if op == "shift" else 0, cutout=(4, 12) if op == "cutout" else (), cutout_fill="zero",
                         intensity=64 if op == "intensity" else 0), (step, op, p)
        seen.add(op)
    assert seen == {"shift", "cutout", "intensity"}
    learner._shift_pad, learner._aug_ops = 0, None
    assert not learner._augments()


def test_rollout_reuse_resolves_to_off_under_the_flags():
    """configure_keep returns before it touches the device: no kept buffers exist with an augmentation on"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.model.actor_critic import ActorCritic
    for on in (dict(augment_cutout=[4, 12]), dict(augment_intensity=64)):
        ac = ActorCritic.__new__(ActorCritic)
        ac.cfg = default_cfg(env="x", batch_size=64, num_batches_per_epoch=2, rollout=8, **on)
        assert ac.configure_keep(16, 8, 16, 4 * 36 * 36 * 9) == 0 and ac._keep is None


# ------------------------------------------------------------------------------------------------ the lanes
def test_new_philox_lanes_are_named_constants_and_documented():
    """lane 2 of the counter: 0 .. 7 are taken; the cutout takes 8 and the intensity 9 as named constants of sf_augment.hip,
    10 is drawn on the host only; no other source names 8, 9 or 10, and the header says so"""
    csrc = os.path.join(ROOT, "sample_factory_amd", "csrc")
    own = open(os.path.join(csrc, "sf_augment.hip")).read()
    assert re.search(r"constexpr uint32_t AUG_LANE_CUTOUT = 8u;", own) and re.search(r"constexpr uint32_t AUG_LANE_INTENSITY = 9u;", own)
    used = set()
    for name in sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))):
        for m in re.finditer(r"sf_philox4x32_10\(([^;]*?)\);", open(os.path.join(csrc, name)).read(), re.S):
            args = [a.strip() for a in m.group(1).split(",")]
            if len(args) >= 7:
                assert args[2].rstrip("u") not in ("8", "9", "10"), f"{name} draws from lane {args[2]} as a literal"
                if args[2] in ("AUG_LANE_CUTOUT", "AUG_LANE_INTENSITY"):
                    assert name == "sf_augment.hip"
                    used.add(args[2])
    assert used == {"AUG_LANE_CUTOUT", "AUG_LANE_INTENSITY"}
    assert (frame_ops.AUGMENT_LANE_CUTOUT, frame_ops.AUGMENT_LANE_INTENSITY, frame_ops.AUGMENT_LANE_SELECT) == (8, 9, 10)
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert "8 .. 10 the cutout, the intensity and the op draw" in text
    assert "LANE = 8 (AUG_LANE_CUTOUT)" in text and "LANE = 9 (AUG_LANE_INTENSITY)" in text and "LANE = 10" in text


# ------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("H,W,lo,hi", [(6, 7, 2, 5), (5, 9, 1, 1), (4, 6, 3, 9)])
def test_cutout_rectangles_lie_inside_the_frame_and_cover_every_side_and_origin(H, W, lo, hi):
    """draw_id 0 .. 8 x 4096 groups: every side length in [MIN, MAX] (clipped to the frame) and, for every side length, every
    legal origin occurs; no rectangle leaves the frame"""
    groups = np.arange(4096)
    seen_h, seen_w = set(), set()
    for draw_id in range(9):
        y0, x0, ch, cw = frame_ops.cutout_draws(12345, draw_id, groups, H, W, lo, hi)
        assert y0.dtype == np.int32 and cw.shape == groups.shape
        assert (ch >= min(lo, H)).all() and (ch <= min(hi, H)).all() and (cw >= min(lo, W)).all() and (cw <= min(hi, W)).all()
        assert (y0 >= 0).all() and (y0 + ch <= H).all() and (x0 >= 0).all() and (x0 + cw <= W).all()
        seen_h |= set(zip(ch.tolist(), y0.tolist()))
        seen_w |= set(zip(cw.tolist(), x0.tolist()))
    assert seen_h == {(c, y) for c in range(min(lo, H), min(hi, H) + 1) for y in range(H - c + 1)}
    assert seen_w == {(c, x) for c in range(min(lo, W), min(hi, W) + 1) for x in range(W - c + 1)}


def test_cut_min_of_at_least_the_frame_gives_the_whole_frame():
    y0, x0, ch, cw = frame_ops.cutout_draws(3, 1, np.arange(256), 5, 7, 7, 30)
    assert (y0 == 0).all() and (x0 == 0).all() and (ch == 5).all() and (cw == 7).all()
    y0, x0, ch, cw = frame_ops.cutout_draws(3, 1, np.arange(256), 5, 7, 5, 6)      # whole rows, columns 5 .. 6 wide
    assert (ch == 5).all() and (y0 == 0).all() and set(cw.tolist()) == {5, 6} and (x0 + cw <= 7).all()
    for bad in ((0, 4), (5, 4), (1, 65536)):
        with pytest.raises(ValueError, match="cutout"):
            frame_ops.cutout_draws(3, 1, np.arange(4), 5, 7, *bad)


def test_intensity_draws_cover_the_range():
    for amp in (1, 64, 255):
        s = np.concatenate([frame_ops.intensity_draws(12345, k, np.arange(4096), amp)[0] for k in range(9)])
        assert set(s.tolist()) == set(range(256 - amp, 256 + amp + 1))
    s, fill = frame_ops.intensity_draws(12345, 0, np.arange(4096), 0)
    assert (s == 256).all() and set(fill.tolist()) == set(range(256))               # amp = 0: no scale, the fill is still drawn
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="intensity"):
            frame_ops.intensity_draws(1, 1, np.arange(4), bad)


def test_draws_depend_on_seed_draw_id_and_group_only_and_are_the_literal_formulas():
    from sample_factory_amd.envs.pixel_catch import philox
    g = np.arange(512)
    cut = lambda seed, draw, groups: frame_ops.cutout_draws(seed, draw, groups, 36, 40, 4, 12)      # noqa: E731
    inten = lambda seed, draw, groups: frame_ops.intensity_draws(seed, draw, groups, 64)            # noqa: E731
    for fn in (cut, inten):
        base = fn(7, 3, g)
        assert all(np.array_equal(a, b) for a, b in zip(base, fn(7, 3, g.copy())))
        for other in (fn(8, 3, g), fn(7, 4, g), fn(7, 3, g + 512)):
            assert all(not np.array_equal(a, b) for a, b in zip(base, other))
        perm = np.random.default_rng(0).permutation(512)
        assert all(np.array_equal(a, b[perm]) for a, b in zip(fn(7, 3, g[perm]), base))
        assert all(a[0] == b[137] for a, b in zip(fn(7, 3, np.array([137])), base))
        assert all(np.array_equal(a, b) for a, b in zip(fn(7 + (1 << 32), 3 + (1 << 32), g), base))   # 32-bit words
    w = [int(v) for v in philox(3, 0, 8, 0, 7, 137)]
    ch, cw = 4 + ((w[0] * 9) >> 32), 4 + ((w[1] * 9) >> 32)
    assert tuple(int(v[137]) for v in cut(7, 3, g)) == ((w[2] * (36 - ch + 1)) >> 32, (w[3] * (40 - cw + 1)) >> 32, ch, cw)
    w = [int(v) for v in philox(3, 0, 9, 0, 7, 137)]
    assert tuple(int(v[137]) for v in inten(7, 3, g)) == (256 - 64 + ((w[0] * 129) >> 32), w[1] >> 24)
    # the three ops draw from different lanes: the shift's words are not the cutout's
    assert not np.array_equal(frame_ops.random_shift_draws(7, 3, g, 4)[1], (cut(7, 3, g)[3] - 4))


def test_op_of_step_hits_every_enabled_op_and_a_single_one_always():
    from sample_factory_amd.envs.pixel_catch import philox
    ops = ["shift", "cutout", "intensity"]
    drawn = [frame_ops.augment_op_of_step(5, k, ops) for k in range(300)]
    assert set(drawn) == set(ops) and all(60 <= drawn.count(o) <= 140 for o in ops)
    assert {frame_ops.augment_op_of_step(5, k, ["cutout", "intensity"]) for k in range(64)} == {"cutout", "intensity"}
    for one in ops:
        assert all(frame_ops.augment_op_of_step(5, k, [one]) == one for k in range(64))
    w = int(philox(11, 0, 10, 0, 5, 0)[0])
    assert frame_ops.augment_op_of_step(5, 11, ops) == ops[(w * 3) >> 32]
    assert frame_ops.augment_op_of_step(5 + (1 << 32), 11 + (1 << 32), ops) == frame_ops.augment_op_of_step(5, 11, ops)
    with pytest.raises(ValueError, match="no op"):
        frame_ops.augment_op_of_step(5, 0, [])


# ------------------------------------------------------------------------------------------------ the frames
def test_intensity_on_u8_is_the_literal_formula_with_ties_and_saturation():
    x = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    for s in (1, 2, 128, 192, 255, 256, 257, 320, 511):
        got = frame_ops.intensity_frames(x, [s]).reshape(-1)
        want = np.minimum(255.0, np.floor(np.arange(256, dtype=np.float64) * s / 256.0 + 0.5))    # ties round half up
        assert got.dtype == np.uint8 and np.array_equal(got.astype(np.float64), want), s
    assert frame_ops.intensity_frames(x, [256]).tobytes() == x.tobytes()                            # s = 256 is the identity
    assert frame_ops.intensity_frames(x, [128]).reshape(-1)[[0, 1, 2, 3, 255]].tolist() == [0, 1, 1, 2, 128]   # 0.5 -> 1, 1.5 -> 2
    hi = frame_ops.intensity_frames(x, [511]).reshape(-1)                                            # A = 255: up to 511 / 256
    assert hi[0] == 0 and hi[127] == 254 and (hi[128:] == 255).all()
    lo = frame_ops.intensity_frames(x, [1]).reshape(-1)                                              # ... and down to 1 / 256
    assert (lo[:128] == 0).all() and (lo[128:] == 1).all()
    two = frame_ops.intensity_frames(np.concatenate([x, x]), [256, 511])                            # one scale per sample
    assert two[0].tobytes() == x.tobytes() and np.array_equal(two[1].reshape(-1), hi)


def test_intensity_on_f32_is_one_float32_multiply():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 2, 5, 7)).astype(np.float32)
    s = np.array([1, 300, 511])
    got = frame_ops.intensity_frames(x, s)
    assert got.dtype == np.float32
    for i in range(3):
        exact = x[i].astype(np.float64) * (s[i] / 256.0)          # s / 256 is exact: the product rounds once
        assert np.array_equal(got[i], exact.astype(np.float32)), i
    with pytest.raises(ValueError, match="dtype"):
        frame_ops.intensity_frames(x.astype(np.float64), s)


def test_cutout_frames_fill_the_rectangle_of_every_plane_and_nothing_else():
    rng = np.random.default_rng(4)
    for dtype in (np.uint8, np.float32):
        x = rng.integers(1, 256, (3, 2, 5, 7)).astype(dtype)
        y0, x0, ch, cw = np.array([0, 1, 4]), np.array([0, 3, 6]), np.array([5, 2, 1]), np.array([7, 3, 1])
        got = frame_ops.cutout_frames(x, y0, x0, ch, cw)
        assert got.dtype == dtype and not got[0].any()
        inside = np.zeros(x.shape, bool)
        for i in range(3):
            inside[i, :, y0[i]:y0[i] + ch[i], x0[i]:x0[i] + cw[i]] = True
        assert (got[inside] == 0).all() and np.array_equal(got[~inside], x[~inside])
    fill = np.array([9, 200, 255])
    got = frame_ops.cutout_frames(x.astype(np.uint8), y0, x0, ch, cw, fill)
    assert all((got[i][inside[i]] == fill[i]).all() for i in range(3))
    with pytest.raises(ValueError, match="u8"):
        frame_ops.cutout_frames(x.astype(np.float32), y0, x0, ch, cw, fill)


def test_augment_frames_with_the_shift_alone_is_random_shift_frames():
    rng = np.random.default_rng(6)
    for dtype in (np.uint8, np.float32):
        x = rng.integers(0, 256, (16, 3, 5, 7)).astype(dtype)
        groups = np.arange(16) // 4
        dy, dx = frame_ops.random_shift_draws(9, 2, groups, 4)
        got = frame_ops.augment_frames(x, 9, 2, groups, pad=4)
        assert got.tobytes() == frame_ops.random_shift_frames(x, dy, dx, 4).tobytes()
        assert frame_ops.augment_frames(x, 9, 2, groups).tobytes() == x.tobytes()   # everything off: the frames
    with pytest.raises(ValueError, match="random"):
        frame_ops.augment_frames(x, 9, 2, groups, cutout=(2, 5), cutout_fill="random")   # (x is f32 here)


def test_the_order_is_shift_then_intensity_then_cutout():
    """a random fill under intensity tells the orders apart: the fill byte is NOT scaled (cutout last), and the rectangle is
    in output coordinates (the shift does not move it)"""
    x = np.full((64, 2, 9, 11), 200, np.uint8)
    x[:, :, 4, 5] = 10                                               # one pixel the shift moves
    groups = np.arange(64)
    kw = dict(pad=2, cutout=(3, 4), cutout_fill="random", intensity=128)
    got = frame_ops.augment_frames(x, 21, 5, groups, **kw)
    dy, dx = frame_ops.random_shift_draws(21, 5, groups, 2)
    s, fill = frame_ops.intensity_draws(21, 5, groups, 128)
    y0, x0, ch, cw = frame_ops.cutout_draws(21, 5, groups, 9, 11, 3, 4)
    want = frame_ops.cutout_frames(frame_ops.intensity_frames(frame_ops.random_shift_frames(x, dy, dx, 2), s), y0, x0, ch, cw, fill)
    assert np.array_equal(got, want)
    other = frame_ops.intensity_frames(frame_ops.cutout_frames(frame_ops.random_shift_frames(x, dy, dx, 2), y0, x0, ch, cw, fill), s)
    assert not np.array_equal(got, other)                            # intensity after the cutout would scale the fill
    moved = frame_ops.random_shift_frames(frame_ops.cutout_frames(x, y0, x0, ch, cw, fill), dy, dx, 2)
    assert not np.array_equal(got, frame_ops.intensity_frames(moved, s))   # the cutout before the shift would move with it
    for i in range(64):
        assert (got[i, :, y0[i]:y0[i] + ch[i], x0[i]:x0[i] + cw[i]] == fill[i]).all(), i
    # each stage is skipped when its parameter is off
    assert np.array_equal(frame_ops.augment_frames(x, 21, 5, groups, intensity=128), frame_ops.intensity_frames(x, s))
    assert np.array_equal(frame_ops.augment_frames(x, 21, 5, groups, cutout=(3, 4)), frame_ops.cutout_frames(x, y0, x0, ch, cw))
