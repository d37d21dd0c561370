"""--augment_cutout / --augment_intensity / --augment_mix through the learner and the runner, after the
pattern of tests/test_gpu_augment_shift_e2e.py (whose helpers, nets and slabs are used).

Learner twin: a flag-on learner trains once on a batch while every gather launch is recorded.  Each recorded output must
equal the NumPy model (frame_ops.augment_frames) of the slab rows it names under the parameters the step must have had —
all enabled ops under augment_mix=all, the one op frame_ops.augment_op_of_step draws under augment_mix=one — bit for bit;
forward and backward must have been handed the same dense buffers.  Then a flag-OFF learner trains from the same weights on
the slab pre-augmented by the model: parameters and Adam moments bit-equal for the feed-forward conv model, within TIGHT of
tests/test_gpu_nn.py for the GRU with recurrence 4; a twin augmented with draw_id + 1 must FAIL the comparison.

Dispatch: the shift alone still goes through lib.random_shift_gather (its timing keys, no augment_gather key); flags off
gather nothing.  DrAC with the cutout alone is accepted; on all-zero frames a zero-filled cutout is the identity, the
consistency sums are exactly 0 and the step is the flag-off learner's.  Runner: PixelCatch, sync and async, and enjoy."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd.envs import frame_ops  # noqa: E402
from sample_factory_amd.envs import pixel_catch as pc  # noqa: E402
from tests.parity_util import compare_post_train  # noqa: E402
from tests.test_gpu_augment_shift_e2e import (E, IMG, PAD, T, _batch, _clone, _golden_of, _learner, _runner_cfg, _spaces,  # noqa: E402
                                               _spy_model)

pytestmark = pytest.mark.gpu

CUT, AMP, ALPHA = (4, 12), 64, 0.1
FLAGS = {"all": dict(augment_cutout=list(CUT), augment_intensity=AMP),
         "one": dict(augment_random_shift=PAD, augment_cutout=list(CUT), augment_intensity=AMP, augment_mix="one")}
GRU = dict(use_rnn=True, rnn_type="gru", rnn_size=32, recurrence=4, shuffle_minibatches=True)


def _spy_gathers(monkeypatch, log):
    """both gather wrappers: what every launch was asked for, and a copy of what it wrote"""
    from sample_factory_amd import lib
    for fn in ("random_shift_gather", "augment_gather"):
        def spy(dst, src, n, shape, _real=getattr(lib, fn), _fn=fn, **kw):
            _real(dst, src, n, shape, **kw)
            idx, off = kw.get("index"), int(kw.get("offset", 0))
            rows = idx[:n].cpu().numpy().astype(np.int64) if idx is not None else np.arange(off, off + n, dtype=np.int64)
            ops = dict(pad=int(kw.get("pad", 0)), cutout=tuple(kw.get("cutout", ()) or ()), cutout_fill=kw.get("cutout_fill", "zero"),
                       intensity=int(kw.get("intensity", 0)))
            log.append(dict(fn=_fn, ops=ops, draw_id=int(kw["draw_id"]), rows=rows, out=dst[:n].clone(), shape=tuple(shape),
                            seed=int(kw["seed"]), recurrence=int(kw["recurrence"]), traj_T=int(kw["traj_T"]),
                            src_ptr=src.data_ptr(), dst_ptr=dst.data_ptr(), n=int(n)))
        monkeypatch.setattr(lib, fn, spy)


def _ops_of_step(flags, seed, draw_id):
    """what the learner must hand lib.augment_gather at this draw id"""
    pad, cut, amp = int(flags.get("augment_random_shift", 0)), tuple(flags.get("augment_cutout", ())), int(flags.get("augment_intensity", 0))
    on = [name for name, v in (("shift", pad), ("cutout", cut), ("intensity", amp)) if v]
    if flags.get("augment_mix", "all") == "one":
        on = [frame_ops.augment_op_of_step(seed, draw_id, on)]
    return dict(pad=pad if "shift" in on else 0, cutout=cut if "cutout" in on else (),
                cutout_fill=flags.get("augment_cutout_fill", "zero"), intensity=amp if "intensity" in on else 0), on


def _twin_batch(batch0, gathers, seed, draw_shift=0):
    """batch0 with every dataset row of the image key replaced by its model-augmented frame, by recorded membership"""
    twin = _clone(batch0)
    slab = batch0["obs"]["obs"].cpu().numpy()
    flat = slab.reshape((E * (T + 1),) + IMG)
    out = flat.copy()
    for rec in gathers:
        d = rec["rows"]
        rows = d + d // T
        out[rows] = frame_ops.augment_frames(flat[rows], seed, rec["draw_id"] + draw_shift, d // rec["recurrence"], **rec["ops"])
    twin["obs"]["obs"].copy_(torch.from_numpy(out.reshape(slab.shape)))
    return twin


def _twin_case(tmp_path, monkeypatch, mix, bit_equal, **over):
    from tests.test_gpu_nn import TIGHT
    from sample_factory_amd import lib
    from sample_factory_amd.model.actor_critic import get_rnn_size
    flags, obs_space = FLAGS[mix], _spaces(False)
    on, env_info = _learner(tmp_path, "on", obs_space, **flags, **over)
    ac = on.actor_critic
    assert on._aug_ops is not None and on._shift_pad == flags.get("augment_random_shift", 0)
    seed = on._shift_seed
    assert seed == frame_ops.random_shift_seed(on.cfg.seed, 0, 0)
    batch0 = _batch(env_info, get_rnn_size(on.cfg) if on.cfg.use_rnn else 1)
    w0 = ac.flat_params.clone()
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    step0 = on.train_step = 41          # a resumed run: the draws continue from the checkpoint's train_step
    gathers, calls = [], []
    _spy_gathers(monkeypatch, gathers)
    _spy_model(ac, calls)
    assert on.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    monkeypatch.undo()
    steps, R = on.cfg.num_batches_per_epoch, on.cfg.recurrence
    assert on.train_step == step0 + steps and len(gathers) == steps
    # ---- every launch against the NumPy model of the slab rows it names
    flat = batch0["obs"]["obs"].cpu().numpy().reshape((E * (T + 1),) + IMG)
    drawn = []
    for i, rec in enumerate(gathers):
        d = rec["rows"]
        want_ops, on_ops = _ops_of_step(flags, seed, step0 + i)
        drawn += on_ops
        assert rec["fn"] == "augment_gather" and rec["ops"] == want_ops, (i, rec["ops"], want_ops)
        assert rec["draw_id"] == step0 + i and rec["seed"] == seed and rec["traj_T"] == T and rec["shape"] == IMG
        assert rec["recurrence"] == R and rec["n"] == on.cfg.batch_size
        want = frame_ops.augment_frames(flat[d + d // T], seed, rec["draw_id"], d // R, **want_ops)
        assert not np.array_equal(want, flat[d + d // T])
        assert rec["out"].cpu().numpy().tobytes() == want.tobytes(), i
        if R > 1:  # one draw per chunk: the rows of a chunk are consecutive and share it
            assert (d.reshape(-1, R) == d[::R, None] + np.arange(R)).all()
    assert len(set(drawn)) >= 2, drawn       # mix=all: cutout and intensity; mix=one: at least two different ops were drawn
    assert mix != "one" or all(len(_ops_of_step(flags, seed, step0 + i)[1]) == 1 for i in range(steps))
    seen = np.concatenate([rec["rows"] for rec in gathers])
    assert np.array_equal(np.sort(seen), np.arange(E * T))   # every dataset row exactly once
    # ---- forward and backward got the same dense buffers, with the dense addressing
    fwds, bwds = [c for c in calls if c[0] == "fwd"], [c for c in calls if c[0] == "bwd"]
    assert len(fwds) == len(bwds) == steps
    for s, (f, b) in enumerate(zip(fwds, bwds)):
        assert f[1:] == b[1:] and f[3] is None and f[4] == 0 and f[5] == 0 and f[2] == on.cfg.batch_size
        assert f[1]["obs"] == gathers[s]["dst_ptr"]

    # ---- the twins: flags off, same weights, pre-augmented slab
    def run_twin(name, draw_shift):
        off, _ = _learner(tmp_path, name, obs_space, **over)
        assert off._shift_pad == 0 and off._aug_ops is None
        off.actor_critic.flat_params.copy_(w0)
        off.actor_critic.params_changed()
        off.train_step = step0
        none = []
        _spy_gathers(monkeypatch, none)
        mbs = []
        real = off._get_minibatches
        off._get_minibatches = lambda *a: mbs.append(real(*a)) or mbs[-1]
        assert off.train(_twin_batch(batch0, gathers, seed, draw_shift)) is not None
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert not none                                   # flags off: no gather is ever launched
        member = [idx.cpu().numpy() if idx is not None else np.arange(o, o + n) for idx, o, n in mbs[0]]
        for s, rows in enumerate(member):                 # the twin trained on the same minibatches
            assert np.array_equal(rows, gathers[s]["rows"])
        return off
    good = run_twin("off", 0)
    compare_post_train(on, _golden_of(good, before), before, "augment_ops_twin", **TIGHT)
    if bit_equal:
        L0, n = ac.layers[0], on.cfg.batch_size
        same_kernels = not (L0.wt is not None and lib.conv_fwd_t_supported(n, L0.desc)) and lib.conv_fwd_workspace(n, L0.desc) == 0
        print(f"dense and indexed conv1 launches resolve to the same kernels: {same_kernels}")
        assert torch.equal(ac.flat_params, good.actor_critic.flat_params)
        assert torch.equal(on.exp_avg, good.exp_avg) and torch.equal(on.exp_avg_sq, good.exp_avg_sq)
    # ---- negative control: a twin augmented by the NEXT step's draws is a different training step
    wrong = run_twin("wrong", 1)
    with pytest.raises(AssertionError):
        compare_post_train(on, _golden_of(wrong, before), before, "augment_ops_twin_wrong", **TIGHT)


@pytest.mark.parametrize("mix", ["all", "one"])
def test_learner_twin_feed_forward(tmp_path, monkeypatch, mix):
    _twin_case(tmp_path, monkeypatch, mix, True, shuffle_minibatches=True)


def test_learner_twin_recurrent_chunks(tmp_path, monkeypatch):
    _twin_case(tmp_path, monkeypatch, "all", False, **GRU)


# ------------------------------------------------------------------------------------------------ dispatch
def test_the_shift_alone_keeps_its_launch_and_its_timing_keys(tmp_path, monkeypatch):
    from sample_factory_amd import lib
    on, env_info = _learner(tmp_path, "shift", _spaces(False), augment_random_shift=PAD)
    assert on._aug_ops is None and on._shift_pad == PAD
    gathers = []
    _spy_gathers(monkeypatch, gathers)
    monkeypatch.setattr(lib, "PROFILE", {})
    assert on.train(_batch(env_info, 1)) is not None
    torch.cuda.synchronize()
    names = {k[0] for k in lib.PROFILE}
    monkeypatch.undo()
    assert len(gathers) == on.cfg.num_batches_per_epoch and all(r["fn"] == "random_shift_gather" and r["ops"]["pad"] == PAD for r in gathers)
    assert "random_shift_gather" in names and "augment_gather" not in names
    # ... and with a new op on, the key is augment_gather's
    on2, _ = _learner(tmp_path, "ops", _spaces(False), augment_random_shift=PAD, augment_intensity=AMP)
    monkeypatch.setattr(lib, "PROFILE", {})
    assert on2.train(_batch(env_info, 1)) is not None
    torch.cuda.synchronize()
    names = {k[0] for k in lib.PROFILE}
    monkeypatch.undo()
    assert "augment_gather" in names and "random_shift_gather" not in names
    assert "augment" in on2.reuse_stats["last_reason"] and on2.reuse_stats["reused"] == 0


def test_random_fill_on_a_float32_image_key_is_refused_at_init(tmp_path):
    from sample_factory_amd.envs import spaces
    f32 = spaces.Dict({"obs": spaces.Box(0.0, 1.0, IMG, np.float32)})
    with pytest.raises(ValueError, match="augment_cutout_fill=random"):
        _learner(tmp_path, "f32", f32, augment_cutout=list(CUT), augment_cutout_fill="random", obs_scale=1.0)


# ------------------------------------------------------------------------------------------------ DrAC without the shift
def test_drac_with_the_cutout_alone_on_all_zero_frames_is_the_flag_off_step(tmp_path, monkeypatch):
    from sample_factory_amd import lib
    from tests.test_gpu_nn import TIGHT
    over = dict(shuffle_minibatches=True)
    on, env_info = _learner(tmp_path, "on", _spaces(False), augment_cutout=list(CUT), augment_consistency_coeff=ALPHA, **over)
    assert on._cons_coeff == ALPHA and on._shift_pad == 0 and on._aug_ops.enabled == ["cutout"]
    ac = on.actor_critic
    batch0 = _batch(env_info, 1)
    batch0["obs"]["obs"].zero_()         # a zero-filled cutout changes nothing: the augmented half IS the clean half
    w0 = ac.flat_params.clone()
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    gathers, sums = [], []
    _spy_gathers(monkeypatch, gathers)
    real = lib.consistency_loss

    def spy(*a, **kw):
        real(*a, **kw)
        sums.append(a[15].clone())  # sums: {sum KL, sum dv^2, max KL, n_valid}
    monkeypatch.setattr(lib, "consistency_loss", spy)
    assert on.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    monkeypatch.undo()
    n, steps = on.cfg.batch_size, on.cfg.num_batches_per_epoch
    assert len(sums) == steps and len(gathers) == 2 * steps
    for s in sums:
        s = s.cpu().numpy()
        assert s[0] == 0.0 and s[1] == 0.0 and s[2] == 0.0 and s[3] == n, s
    assert on.last_summary["consistency_kl"] == 0.0 and on.last_summary["consistency_value"] == 0.0
    for clean, aug in zip(gathers[0::2], gathers[1::2]):  # rows [0, n) the plain gather, rows [n, 2n) the step's augmentation
        assert clean["fn"] == "random_shift_gather" and clean["ops"]["pad"] == 0
        assert aug["fn"] == "augment_gather" and aug["ops"] == dict(pad=0, cutout=CUT, cutout_fill="zero", intensity=0)
        assert np.array_equal(clean["rows"], aug["rows"]) and aug["dst_ptr"] == clean["dst_ptr"] + n * int(np.prod(IMG))
    off, _ = _learner(tmp_path, "off", _spaces(False), **over)
    off.actor_critic.flat_params.copy_(w0)
    off.actor_critic.params_changed()
    assert off.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    compare_post_train(on, _golden_of(off, before), before, "drac_cutout_zero_frames", **TIGHT)


# ------------------------------------------------------------------------------------------------ the runner
def _count_gathers(monkeypatch):
    from sample_factory_amd import lib
    count = dict(random_shift_gather=0, augment_gather=0)
    for fn in count:
        def counted(*a, _real=getattr(lib, fn), _fn=fn, **kw):
            count[_fn] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(lib, fn, counted)
    return count


@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
def test_runner_trains_pixel_catch_under_the_flags(tmp_path, monkeypatch, async_rl):
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    from sample_factory_amd.train import make_runner
    extra = dict(async_rl=True, serial_mode=False) if async_rl else {}
    count = _count_gathers(monkeypatch)
    flags = dict(FLAGS["one"], augment_cutout_fill="random")
    cfg, runner = make_runner(_runner_cfg(tmp_path, "ops", **flags, **extra))
    assert runner.init() == 0
    try:
        p0 = runner.learner.actor_critic.flat_params.clone()
        for _ in range(3):
            runner.iteration()
        torch.cuda.synchronize()
        learner = runner.learner
        stats = dict(learner.last_summary)
        assert stats and all(np.isfinite(float(v)) for v in stats.values()), stats
        assert torch.isfinite(learner.actor_critic.flat_params).all() and not torch.equal(p0, learner.actor_critic.flat_params)
        assert learner.reuse_stats["reused"] == 0 and "augment" in learner.reuse_stats["last_reason"]
        assert getattr(learner.actor_critic, "_keep", None) is None
        # one gather per SGD step, none from rollouts or bootstrap values
        assert count["augment_gather"] == learner.train_step >= 1 and count["random_shift_gather"] == 0
        saved = json.load(open(tmp_path / "ops" / "config.json"))
        assert {k: saved[k] for k in flags} == flags
        learner.save()
    finally:
        runner.close_envs()
    del runner
    # ---- enjoy reads the flags back from config.json and never gathers
    count.update(random_shift_gather=0, augment_gather=0)
    argv = ["--env=pixel_catch", f"--train_dir={tmp_path}", "--experiment=ops", "--max_num_episodes=8", "--pixel_catch_agents=8"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    pc.add_pixel_catch_args(parser)
    status, avg = enjoy(parse_full_cfg(parser, argv))
    assert status == 0 and np.isfinite(avg) and count == dict(random_shift_gather=0, augment_gather=0)


def test_runner_with_the_flags_off_never_gathers(tmp_path, monkeypatch):
    from sample_factory_amd.train import make_runner
    count = _count_gathers(monkeypatch)
    cfg, runner = make_runner(_runner_cfg(tmp_path, "plain"))
    assert runner.init() == 0
    try:
        for _ in range(2):
            runner.iteration()
        torch.cuda.synchronize()
        assert count == dict(random_shift_gather=0, augment_gather=0) and runner.learner.train_step >= 1
        assert runner.learner._aug_ops is None and runner.learner._shift_pad == 0
        saved = json.load(open(tmp_path / "plain" / "config.json"))
        assert (saved["augment_cutout"], saved["augment_cutout_fill"], saved["augment_intensity"], saved["augment_mix"]) == \
            ([], "zero", 0, "all")
    finally:
        runner.close_envs()
