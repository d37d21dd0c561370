"""--hwc_observations end to end: the host-frame env serves its ring channel-last ([H, W, C]) and the Runner transposes
every frame on the device — alone (sf_hwc_to_chw) or inside the frame stack's launch (sf_framestack_step_hwc).  The run must
be bit-identical to one with the flag off on the channel-first env of the same seed: every slab tensor after each rollout,
and the flat parameter buffer after training.

Frames are (3, 20, 20): the smallest square frame convnet_impala (8x8 / 4, then 4x4 / 2) still maps to a 1x1 feature map.
Both runs issue the same learner launches on the same bytes, so the comparison holds at the default learning rate; only the
async run trains at rate 0, where the policy lag of a rollout (a matter of timing) cannot reach its actions."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd.envs import spaces  # noqa: E402

pytestmark = pytest.mark.gpu

K, T, N = 4, 4, 8
SHAPE = (3, 20, 20)   # what the engine sees per frame; the channel-last env delivers (20, 20, 3)
FIELDS = ("actions", "action_logits", "log_prob_actions", "rewards", "dones", "time_outs")


class HostFrameDictEnv:
    """the host-frame env with a vector key beside the image: vec[i] = (agent, step, ring slot)"""

    def __init__(self, env):
        self.env, self.num_agents, self.action_space = env, env.num_agents, env.action_space
        self.observation_space = spaces.Dict(dict(env.observation_space.spaces, vec=spaces.Box(-1e6, 1e6, (3,), np.float32)))

    def _out(self, o):
        s = self.env.step_count
        vec = np.stack([np.array([i, s, s % len(self.env.ring)], np.float32) for i in range(self.num_agents)])
        return dict(o, vec=vec)

    def reset(self, **kwargs):
        o, info = self.env.reset(**kwargs)
        return self._out(o), info

    def step(self, actions):
        o, rew, te, tr, info = self.env.step(actions)
        return self._out(o), rew, te, tr, info

    def close(self):
        self.env.close()


def make_dict_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    from sample_factory_amd.envs.synthetic import make_host_frame_env
    return HostFrameDictEnv(make_host_frame_env(full_env_name, cfg, env_config, render_mode))


def _transposed(sampler):
    """the keys whose route goes through the transpose kernels"""
    return [k for k, r in sampler.routes.items() if r.key.hwc and r.key.resize is None]


def _stacked(sampler):
    """key -> channels of one frame, for the keys the device stacks"""
    return {k: r.key.frame_shape[0] for k, r in sampler.routes.items() if r.key.k > 1}


def _cfg(hwc: bool, **kw):
    """hwc: the env serves channel-last frames AND the engine is told so; off: the channel-first env, the parent's path"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_host_frame_env
    register_env("hwc_host_frames", make_host_frame_env)
    register_env("hwc_host_frames_dict", make_dict_env)
    base = dict(env="hwc_host_frames", use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_impala", encoder_conv_mlp_layers=[32], encoder_mlp_layers=[16],
                rollout=T, batch_size=N * T, num_batches_per_epoch=1, num_epochs=1, num_workers=1, num_envs_per_worker=1,
                worker_num_splits=1, async_rl=False, serial_mode=True, seed=11, env_gpu_observations=False,
                env_gpu_actions=False, env_workers_mode="inline", synthetic_num_agents=N, host_env_obs_shape=list(SHAPE),
                host_env_hwc=hwc, hwc_observations=hwc)
    base.update(kw)
    return default_cfg(**base)


def _snapshot(rows):
    snap = {f: rows[f].cpu().numpy().copy() for f in FIELDS}
    snap["values"] = rows["values"][:, :T].cpu().numpy().copy()
    for k, v in rows["obs"].items():
        snap["obs." + k] = v.cpu().numpy().copy()
    return snap


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for f in a:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


def run(hwc: bool, iters=2, **kw):
    """sync mode: (one snapshot of every env instance's slab rows per iteration, parameters at the start and at the end,
    runner).  Worker processes are stopped before this returns."""
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_cfg(hwc, **kw))
    assert runner.init() == 0
    try:
        p0 = runner.learner.actor_critic.flat_params.clone()
        snaps = []
        for _ in range(iters):
            assert runner.iteration() is not None
            torch.cuda.synchronize()
            snaps.append([_snapshot(rows) for rows in runner._prev_rows])
        # (closing the workers un-registers their pages: note first whether the DMA could read them in place)
        runner.pages_were_registered = [bool(getattr(sm.env, "pages_registered", False)) for sm in runner.samplers]
        return snaps, p0, runner.learner.actor_critic.flat_params.clone(), runner
    finally:
        runner.close_envs()


def _ring(env_id: int, n: int):
    """the channel-first ring [slots, n, C, H, W] of the env instance with this id"""
    from sample_factory_amd.envs.synthetic import HostFrameVecEnv
    return HostFrameVecEnv(num_agents=n, obs_shape=SHAPE, seed=11 + env_id).ring


# ------------------------------------------------------------------------------------------------ equal runs, inline
@pytest.mark.parametrize("k", [1, K], ids=["frames", "device_framestack_4"])
def test_run_on_the_channel_last_env_equals_the_run_on_the_channel_first_env(k, tmp_path):
    a, pa0, pa, ra = run(True, device_framestack=k, train_dir=str(tmp_path / "hwc"))
    b, pb0, pb, rb = run(False, device_framestack=k, train_dir=str(tmp_path / "chw"))
    # what the env delivers and what the engine is built from
    assert ra.env.observation_space["obs"].shape == SHAPE[1:] + SHAPE[:1] and rb.env.observation_space["obs"].shape == SHAPE
    assert ra.env_info.obs_space["obs"].shape == rb.env_info.obs_space["obs"].shape == (k * SHAPE[0],) + SHAPE[1:]
    sm = ra.sampler
    assert _transposed(sm) == ["obs"] and sm.routes["obs"].stage.shape == (N,) + SHAPE[1:] + SHAPE[:1]
    assert not _transposed(rb.sampler)
    assert sm.host_env and _stacked(sm) == ({"obs": SHAPE[0]} if k > 1 else {})
    for r, (sa, sb) in enumerate(zip(a, b)):
        _same(sa[0], sb[0], f"rollout {r}")
    # the frames are the ring's (k = 1: column t of rollout r is ring slot (r T + t) % 4; stacked: its last C planes)
    ring = _ring(0, N)
    for r, snap in enumerate(a):
        for t in range(T + 1):
            assert np.array_equal(snap[0]["obs.obs"][:, t, -SHAPE[0]:], ring[(r * T + t) % len(ring)]), (r, t)
    assert torch.equal(pa0, pb0) and torch.equal(pa, pb) and not torch.equal(pa, pa0)
    assert np.abs(a[-1][0]["values"]).max() > 0 and np.isfinite(a[-1][0]["log_prob_actions"]).all()
    # one frame per agent and step went over the bus in either layout; the record half still replays as a program
    assert ra.sampler.h2d_bytes == rb.sampler.h2d_bytes == (2 * T + 1) * N * int(np.prod(SHAPE)) + 2 * T * N * 6


def test_launch_programs_replay_the_stack_launch():
    """rollouts 3 and 4 replay recorded programs; the frame stack's launch reads the ONE staging buffer at a fixed address"""
    from sample_factory_amd import lib
    a, _, _, ra = run(True, iters=4, device_framestack=K, learning_rate=0.0)
    b, _, _, rb = run(False, iters=4, device_framestack=K, learning_rate=0.0)
    if lib.LAUNCH_PROGRAMS:
        assert ra.sampler.program_replays > 0 and ra.sampler.program_replays == rb.sampler.program_replays
        progs = [p for key, p in ra.sampler._progs.items() if key[0] == "record" and isinstance(p, lib.LaunchProgram)]
        assert progs and all(p.unsafe is None and "sf_framestack_step_hwc" in [c[2] for c in p.calls] for p in progs)
    for r, (sa, sb) in enumerate(zip(a, b)):
        _same(sa[0], sb[0], f"rollout {r}")


# ------------------------------------------------------------------------------------------------ worker processes
W, I, n = 2, 2, 4


def _workers(**kw):
    return dict(num_workers=W, num_envs_per_worker=I, worker_num_splits=2, serial_mode=False, env_workers_mode="auto",
                synthetic_num_agents=n, batch_size=W * I * n * T // 2, num_batches_per_epoch=2, **kw)


def test_env_worker_processes_two_splits_sync(tmp_path):
    """2 workers x 2 instances x 4 agents dealt to 2 splits; the channel-last frames leave the workers' shared pages by DMA
    into the staging buffer of their split"""
    a, _, pa, ra = run(True, device_framestack=K, train_dir=str(tmp_path / "hwc"), **_workers())
    b, _, pb, rb = run(False, device_framestack=K, train_dir=str(tmp_path / "chw"), **_workers())
    assert len(ra.samplers) == 2 and all(s.async_env and s.host_env and _transposed(s) == ["obs"] for s in ra.samplers)
    # the workers' pages hold [rows, H, W, C] as the env's own space says: where the runtime registered them, the DMA into
    # the staging buffer reads them in place, no host copy touches a frame
    assert all(bool(s._direct_ok.get("obs")) == reg for s, reg in zip(ra.samplers, ra.pages_were_registered))
    assert ra.samplers[0].env.observation_space["obs"].shape == SHAPE[1:] + SHAPE[:1]
    for r, (sa, sb) in enumerate(zip(a, b)):
        for split in range(2):
            _same(sa[split], sb[split], f"rollout {r} split {split}")
    for split in range(2):  # rows of a split: (worker, agent) of instance `split` of every worker; env_id = w * I + split
        ring = np.concatenate([_ring(w * I + split, n) for w in range(W)], 1)
        for t in range(T + 1):
            assert np.array_equal(a[-1][split]["obs.obs"][:, t, -SHAPE[0]:], ring[(T + t) % len(ring)]), (split, t)
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("threaded", [False, True], ids=["stream_overlap", "sampler_thread"])
def test_env_worker_processes_async(threaded):
    """async mode at learning rate 0.  Without the sampler thread the rounds are issued in program order and the two runs
    are compared slab for slab; with it the number of finished rounds is a matter of timing, so the last rollout of every
    split is held against the env's own ring instead"""
    from sample_factory_amd.train import make_runner
    out = []
    for hwc in ([True, False] if not threaded else [True]):
        cfg, runner = make_runner(_cfg(hwc, async_rl=True, sampler_thread=threaded, learning_rate=0.0,
                                       **_workers()))
        assert runner.init() == 0
        try:
            assert runner.threaded == threaded
            trained = 0
            for _ in range(4):
                trained += runner.iteration() is not None
            runner.stop_sampler_thread()
            torch.cuda.synchronize()
            assert trained >= 2
            out.append(([_snapshot(rows) for rows in runner._prev_rows], runner.sampling_rounds))
        finally:
            runner.close_envs()
    (a, rounds) = out[0]
    for split in range(2):
        ring = np.concatenate([_ring(w * I + split, n) for w in range(W)], 1)
        for t in range(T + 1):
            assert np.array_equal(a[split]["obs.obs"][:, t], ring[((rounds - 1) * T + t) % len(ring)]), (split, t)
    if not threaded:
        assert out[1][1] == rounds
        for split in range(2):
            _same(a[split], out[1][0][split], f"split {split}")


# ------------------------------------------------------------------------------------------------ a dict env
@pytest.mark.parametrize("k", [1, K], ids=["frames", "device_framestack_4"])
def test_dict_env_transposes_the_image_key_only(k):
    a, _, pa, ra = run(True, env="hwc_host_frames_dict", device_framestack=k)
    b, _, pb, rb = run(False, env="hwc_host_frames_dict", device_framestack=k)
    assert ra.sampler.multi_key and _transposed(ra.sampler) == ["obs"]
    assert ra.env_info.obs_space["obs"].shape == (k * SHAPE[0],) + SHAPE[1:] and ra.env_info.obs_space["vec"].shape == (3,)
    assert ra.env.observation_space["obs"].shape == SHAPE[1:] + SHAPE[:1]
    for r, (sa, sb) in enumerate(zip(a, b)):
        assert sa[0]["obs.vec"].shape == (N, T + 1, 3) and sa[0]["obs.vec"][3, 2].tolist() == [3.0, r * T + 2, (r * T + 2) % 4]
        _same(sa[0], sb[0], f"rollout {r}")
    assert torch.equal(pa, pb)


# ------------------------------------------------------------------------------------------------ a device-tensor env
class DeviceFrameEnv:
    """the host-frame env handing out CUDA tensors (a device env without step_into).  layout: "tight" = rows back to back,
    "pitched" = contiguous rows 16 bytes apart from each other, "strided" = rows that are no contiguous blocks"""

    def __init__(self, env, layout):
        self.env, self.num_agents, self.action_space, self.layout = env, env.num_agents, env.action_space, layout
        self.observation_space = env.observation_space
        shape = env.observation_space["obs"].shape
        n, fb = env.num_agents, int(np.prod(shape))
        if layout == "pitched":
            self.out = torch.zeros((n, fb + 16), dtype=torch.uint8, device="cuda")[:, :fb].view((n,) + shape)
        elif layout == "strided":
            self.out = torch.zeros((n,) + shape[:-1] + (2 * shape[-1],), dtype=torch.uint8, device="cuda")[..., ::2]
        else:
            self.out = torch.zeros((n,) + shape, dtype=torch.uint8, device="cuda")

    def _out(self, o):
        self.out.copy_(torch.from_numpy(o["obs"]).cuda())
        return {"obs": self.out}

    def reset(self, **kwargs):
        o, info = self.env.reset(**kwargs)
        return self._out(o), info

    def step(self, actions):
        o, rew, te, tr, info = self.env.step(actions.cpu().numpy())
        return self._out(o), rew, te, tr, info

    def close(self):
        self.env.close()


def make_device_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    from sample_factory_amd.envs.synthetic import make_host_frame_env
    return DeviceFrameEnv(make_host_frame_env(full_env_name, cfg, env_config, render_mode), cfg.hwc_test_layout)


@pytest.mark.parametrize("layout", ["tight", "pitched", "strided"])
@pytest.mark.parametrize("k", [1, K], ids=["frames", "device_framestack_4"])
def test_device_tensor_env_is_read_in_place_when_its_rows_are_contiguous(k, layout):
    from sample_factory_amd.envs.env_utils import register_env
    register_env("hwc_device_frames", make_device_env)
    a, _, pa, ra = run(True, env="hwc_device_frames", device_framestack=k, hwc_test_layout=layout)
    b, _, pb, rb = run(False, env="hwc_device_frames", device_framestack=k, hwc_test_layout="tight")
    sm = ra.sampler
    assert not sm.host_env and not sm.zero_copy and _transposed(sm) == ["obs"]
    in_place = sm.routes["obs"].frame.data_ptr() == ra.env.out.data_ptr()
    assert in_place == (layout != "strided") and (in_place or sm.routes["obs"].frame is sm.routes["obs"].stage)
    for r, (sa, sb) in enumerate(zip(a, b)):
        _same(sa[0], sb[0], f"rollout {r}")
    assert torch.equal(pa, pb)


# ------------------------------------------------------------------------------------------------ enjoy
def test_enjoy_rebuilds_the_pipeline_from_the_saved_config(tmp_path):
    from sample_factory_amd.cfg.arguments import load_from_checkpoint, parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    _, _, _, runner = run(True, iters=1, device_framestack=K, train_dir=str(tmp_path), experiment="hwc_enjoy")
    conv1 = next(v for v in runner.learner.actor_critic.state_dict().values() if v.dim() == 4)
    assert conv1.shape[1] == K * SHAPE[0]  # conv1 reads C k planes
    runner.learner.save()
    del runner
    argv = ["--env=hwc_host_frames", f"--train_dir={tmp_path}", "--experiment=hwc_enjoy", "--max_num_frames=8"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    ecfg = parse_full_cfg(parser, argv)
    assert ecfg.hwc_observations is False and ecfg.device_framestack == 1  # not given here: they come from config.json
    loaded = load_from_checkpoint(parse_full_cfg(parser, argv))
    assert loaded.hwc_observations is True and loaded.device_framestack == K and loaded.host_env_hwc is True
    status, avg = enjoy(ecfg)  # (loading the checkpoint into a model with any other conv1 would raise)
    assert status == 0 and 0.0 <= avg <= 3 * T + 1


# ------------------------------------------------------------------------------------------------ refusals
def test_set_up_refusals():
    from sample_factory_amd.envs.cartpole import make_cartpole_env
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.train import make_runner
    register_env("hwc_cartpole_vec", make_cartpole_env)
    with pytest.raises(ValueError, match="three dimensions"):
        make_runner(_cfg(True, env="hwc_cartpole_vec", cartpole_num_agents=N))[1].init()
    register_env("hwc_synthetic_atari", make_synthetic_env)
    with pytest.raises(NotImplementedError, match="step_into"):
        make_runner(_cfg(True, env="hwc_synthetic_atari"))[1].init()
