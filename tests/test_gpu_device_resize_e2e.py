"""--device_resize / --device_grayscale end to end: a scripted HOST vector env serves native u8 frames of 90 x 64 x 3 whose
pixels encode (agent, episode, step); with the flags the Runner resizes / grey-scales every frame on the device
(sf_frame_resize) into the slab.  The run must be bit-identical — every slab tensor after each rollout, and the flat
parameter buffer after training — to one where the SAME env preprocesses with envs/frame_ops.py on the host and delivers
the small channel-first frames with the flags off.

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

from sample_factory_amd.envs import frame_ops, spaces  # noqa: E402

pytestmark = pytest.mark.gpu

K, T, N = 4, 4, 8
NATIVE, OUT = (90, 64, 3), (36, 36)       # H, W, C as the env renders; OH, OW
NATIVE_BYTES = int(np.prod(NATIVE))
_IDX = np.arange(NATIVE_BYTES).reshape(NATIVE)
FIELDS = ("actions", "action_logits", "log_prob_actions", "rewards", "dones", "time_outs")
GRAY_STACK = dict(hwc=True, device_resize=list(OUT), device_grayscale=True, device_framestack=K)
COLOUR_NEAREST = dict(hwc=False, device_resize=list(OUT), device_resize_interpolation="nearest")


def frame_of(agent: int, episode: int, step: int) -> np.ndarray:
    """[H, W, C] u8"""
    f = ((_IDX * 5 + (_IDX // 192) * 31 + agent * 7 + episode * 13 + step * 29) % 251).astype(np.uint8)
    f[0, 0] = (agent, episode, step)
    return f


def flags_of(agent: int, s: int):
    """(terminated, truncated) of env step s: episodes end at the first and at the last step of a rollout, some by
    truncation alone (the stack is refilled there)"""
    return (s + agent) % 4 == 0, (s + 3 * agent) % 7 == 6


class ScriptedRawFrameVecEnv:
    """auto-resetting host vector env; nothing depends on the actions.  layout: the native frames leave as [H, W, C]
    ("hwc") or [C, H, W] ("chw"); host = (OH, OW, interpolation, grayscale): the env preprocesses them itself, with the
    NumPy model, and delivers [C', OH, OW] — what a user's wrapper stack does without the flags"""

    def __init__(self, num_agents, agent0, layout, host=None):
        self.num_agents, self.agent0, self.layout, self.host = int(num_agents), int(agent0), layout, host
        h, w, c = NATIVE
        shape = NATIVE if layout == "hwc" else (c, h, w)
        if host is not None:
            shape = (1 if host[3] else c, host[0], host[1])
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 255, shape, np.uint8)})
        self.action_space = spaces.Discrete(3)
        self.is_multiagent = True

    def _obs(self):
        ids = range(self.agent0, self.agent0 + self.num_agents)
        f = np.stack([frame_of(a, e, t) for a, e, t in zip(ids, self.episode, self.step_in_ep)])   # [n, H, W, C]
        if self.host is not None:
            return {"obs": frame_ops.preprocess_frames(f, "hwc", *self.host)}
        return {"obs": f if self.layout == "hwc" else np.ascontiguousarray(f.transpose(0, 3, 1, 2))}

    def reset(self, **kwargs):
        self.episode, self.step_in_ep, self.s = [0] * self.num_agents, [0] * self.num_agents, 0
        return self._obs(), {}

    def step(self, actions):
        assert np.asarray(actions).shape == (self.num_agents,)
        fl = [flags_of(self.agent0 + i, self.s) for i in range(self.num_agents)]
        for i, (te, tr) in enumerate(fl):
            self.episode[i], self.step_in_ep[i] = (self.episode[i] + 1, 0) if (te or tr) else \
                (self.episode[i], self.step_in_ep[i] + 1)
        self.s += 1
        rew = np.array([((self.agent0 + i + self.s) % 5) * 0.25 for i in range(self.num_agents)], np.float32)
        return self._obs(), rew, np.array([f[0] for f in fl]), np.array([f[1] for f in fl]), {}

    def close(self):
        pass


def make_raw_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = int(getattr(cfg, "rs_test_agents", N))
    env_id = int(getattr(env_config, "env_id", 0) or 0)
    host = getattr(cfg, "rs_test_host", None)
    return ScriptedRawFrameVecEnv(n, env_id * n, getattr(cfg, "rs_test_layout", "hwc"), tuple(host) if host else None)


def _cfg(on: bool, hwc=True, device_resize=(), device_resize_interpolation="area", device_grayscale=False, **kw):
    """on: the env serves native frames and the engine preprocesses them; off: the env preprocesses on the host with the
    same settings and the three flags stay at their defaults"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    register_env("rs_raw_frames", make_raw_env)
    base = dict(env="rs_raw_frames", use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_impala", encoder_conv_mlp_layers=[32], encoder_mlp_layers=[16],
                rollout=T, batch_size=N * T, num_batches_per_epoch=1, num_epochs=1, num_workers=1, num_envs_per_worker=1,
                worker_num_splits=1, async_rl=False, serial_mode=True, seed=11, env_gpu_observations=False,
                env_gpu_actions=False, env_workers_mode="inline", rs_test_agents=N)
    if on:
        base.update(hwc_observations=bool(hwc), rs_test_layout="hwc" if hwc else "chw", device_resize=list(device_resize),
                    device_resize_interpolation=device_resize_interpolation, device_grayscale=device_grayscale)
    else:
        size = list(device_resize) or list(NATIVE[:2])
        base.update(rs_test_host=[size[0], size[1], device_resize_interpolation, bool(device_grayscale)])
    base.update(kw)
    return default_cfg(**base)


def _preprocessed(sampler):
    """the keys whose route goes through sf_frame_resize"""
    return [k for k, r in sampler.routes.items() if r.key.resize is not None]


def _stacked(sampler):
    """key -> channels of one frame, for the keys the device stacks"""
    return {k: r.key.frame_shape[0] for k, r in sampler.routes.items() if r.key.k > 1}


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


def run(on: bool, iters=2, **kw):
    """sync mode: (one snapshot of every env instance's slab rows per iteration, parameters at the start and at the end,
    runner).  Worker processes are stopped before this returns."""
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_cfg(on, **kw))
    assert runner.init() == 0
    try:
        p0 = runner.learner.actor_critic.flat_params.clone()
        snaps = []
        for _ in range(iters):
            assert runner.iteration() is not None
            torch.cuda.synchronize()
            snaps.append([_snapshot(rows) for rows in runner._prev_rows])
        return snaps, p0, runner.learner.actor_critic.flat_params.clone(), runner
    finally:
        runner.close_envs()


def _expected_last_frames(agents, steps, interp, gray):
    """[len(agents), steps + 1, C', OH, OW]: the preprocessed frame the env shows after s steps"""
    out = []
    for a in agents:
        episode, step, frames = 0, 0, [frame_of(a, 0, 0)]
        for s in range(steps):
            episode, step = (episode + 1, 0) if any(flags_of(a, s)) else (episode, step + 1)
            frames.append(frame_of(a, episode, step))
        out.append(frame_ops.preprocess_frames(np.stack(frames), "hwc", OUT[0], OUT[1], interp, gray))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ equal runs, inline
def test_grey_area_stacked_run_on_native_hwc_frames_equals_the_host_preprocessed_run(tmp_path):
    a, pa0, pa, ra = run(True, train_dir=str(tmp_path / "dev"), **GRAY_STACK)
    b, pb0, pb, rb = run(False, train_dir=str(tmp_path / "host"), **GRAY_STACK)
    # what the env delivers and what the engine is built from
    assert ra.env.observation_space["obs"].shape == NATIVE and rb.env.observation_space["obs"].shape == (1,) + OUT
    assert ra.env_info.obs_space["obs"].shape == rb.env_info.obs_space["obs"].shape == (K,) + OUT
    sm = ra.sampler
    assert _preprocessed(sm) == ["obs"] and sm.routes["obs"].stage.shape == (N,) + NATIVE and not _preprocessed(rb.sampler)
    assert sm.routes["obs"].key.hwc and not [k for k, r in sm.routes.items() if r.key.hwc and r.key.resize is None]
    assert sm.host_env and _stacked(sm) == {"obs": 1}                      # the resize launch reads HWC itself
    for r, (sa, sb) in enumerate(zip(a, b)):
        _same(sa[0], sb[0], f"rollout {r}")
    want = _expected_last_frames(range(N), 2 * T, "area", True)
    for r, snap in enumerate(a):
        for t in range(T + 1):   # the newest slot of every column is the frame the env showed then, preprocessed
            assert np.array_equal(snap[0]["obs.obs"][:, t, K - 1:], want[:, r * T + t]), (r, t)
    assert torch.equal(pa0, pb0) and torch.equal(pa, pb) and not torch.equal(pa, pa0)
    assert np.abs(a[-1][0]["values"]).max() > 0 and np.isfinite(a[-1][0]["log_prob_actions"]).all()
    # h2d_bytes counts the native bytes: one native frame per agent and step (and the reset), plus rewards and flags
    other = 2 * T * N * 6
    assert ra.sampler.h2d_bytes == (2 * T + 1) * N * NATIVE_BYTES + other
    assert rb.sampler.h2d_bytes == (2 * T + 1) * N * OUT[0] * OUT[1] + other


def test_colour_nearest_run_on_native_chw_frames_without_a_stack(tmp_path):
    a, _, pa, ra = run(True, train_dir=str(tmp_path / "dev"), **COLOUR_NEAREST)
    b, _, pb, rb = run(False, train_dir=str(tmp_path / "host"), **COLOUR_NEAREST)
    assert ra.env.observation_space["obs"].shape == (3, 90, 64) and ra.env_info.obs_space["obs"].shape == (3,) + OUT
    assert ra.sampler.routes["obs"].stage.shape == (N, 3, 90, 64) and not _stacked(ra.sampler)
    assert _preprocessed(ra.sampler) == ["obs"] and not ra.sampler.routes["obs"].key.hwc
    for r, (sa, sb) in enumerate(zip(a, b)):
        _same(sa[0], sb[0], f"rollout {r}")
    want = _expected_last_frames(range(N), 2 * T, "nearest", False)
    for r, snap in enumerate(a):
        assert np.array_equal(snap[0]["obs.obs"], want[:, r * T:r * T + T + 1]), r
    assert torch.equal(pa, pb)
    assert ra.sampler.h2d_bytes == (2 * T + 1) * N * NATIVE_BYTES + 2 * T * N * 6


def test_grey_scale_alone_keeps_the_size():
    kw = dict(hwc=True, device_grayscale=True, iters=1)
    a, _, pa, ra = run(True, **kw)
    b, _, pb, rb = run(False, **kw)
    assert ra.env_info.obs_space["obs"].shape == (1,) + NATIVE[:2]
    _same(a[0][0], b[0][0], "rollout 0")
    assert torch.equal(pa, pb)


def test_launch_programs_still_replay_around_the_resize_launch():
    """rollouts 3 and 4 replay recorded programs; the resize launch sits outside the recorded halves, the stack's launch
    inside the record half, and reads the slab slot sf_frame_resize wrote"""
    from sample_factory_amd import lib
    a, _, _, ra = run(True, iters=4, learning_rate=0.0, **GRAY_STACK)
    b, _, _, rb = run(False, iters=4, learning_rate=0.0, **GRAY_STACK)
    if lib.LAUNCH_PROGRAMS:
        assert ra.sampler.program_replays > 0 and ra.sampler.program_replays == rb.sampler.program_replays
        progs = [p for key, p in ra.sampler._progs.items() if key[0] == "record" and isinstance(p, lib.LaunchProgram)]
        names = [[c[2] for c in p.calls] for p in progs]
        assert progs and all(p.unsafe is None for p in progs)
        assert all("sf_framestack_step" in n and "sf_frame_resize" not in n for n in names)
    for r, (sa, sb) in enumerate(zip(a, b)):
        _same(sa[0], sb[0], f"rollout {r}")


# ------------------------------------------------------------------------------------------------ worker processes
W, I, n = 2, 2, 4


def _workers(**kw):
    return dict(num_workers=W, num_envs_per_worker=I, worker_num_splits=2, serial_mode=False, env_workers_mode="auto",
                rs_test_agents=n, batch_size=W * I * n * T // 2, num_batches_per_epoch=2, **kw)


def test_env_worker_processes_two_splits_sync(tmp_path):
    """2 workers x 2 instances x 4 agents dealt to 2 splits; the native frames leave the workers' shared pages by DMA into
    the staging buffer of their split"""
    a, _, pa, ra = run(True, train_dir=str(tmp_path / "dev"), **_workers(**GRAY_STACK))
    b, _, pb, rb = run(False, train_dir=str(tmp_path / "host"), **_workers(**GRAY_STACK))
    assert len(ra.samplers) == 2 and all(s.async_env and s.host_env and _preprocessed(s) == ["obs"] for s in ra.samplers)
    assert ra.samplers[0].env.observation_space["obs"].shape == NATIVE
    assert all(s.routes["obs"].stage.shape == (W * n,) + NATIVE for s in ra.samplers)
    for r, (sa, sb) in enumerate(zip(a, b)):
        for split in range(2):
            _same(sa[split], sb[split], f"rollout {r} split {split}")
    for split in range(2):  # rows of a split: (worker, agent) of instance `split` of every worker; env_id = w * I + split
        agents = [(w * I + split) * n + i for w in range(W) for i in range(n)]
        want = _expected_last_frames(agents, 2 * T, "area", True)
        for t in range(T + 1):
            assert np.array_equal(a[-1][split]["obs.obs"][:, t, K - 1:], want[:, T + t]), (split, t)
    assert torch.equal(pa, pb)
    assert sum(s.h2d_bytes for s in ra.samplers) == 2 * W * n * ((2 * T + 1) * NATIVE_BYTES + 2 * T * 6)


def test_env_worker_processes_async():
    """async mode at learning rate 0, no sampler thread: the rounds are issued in program order and the two runs are compared
    slab for slab"""
    from sample_factory_amd.train import make_runner
    out = []
    for on in (True, False):
        cfg, runner = make_runner(_cfg(on, async_rl=True, sampler_thread=False, learning_rate=0.0, **_workers(**GRAY_STACK)))
        assert runner.init() == 0
        try:
            assert not runner.threaded
            trained = 0
            for _ in range(4):
                trained += runner.iteration() is not None
            runner.stop_sampler_thread()
            torch.cuda.synchronize()
            assert trained >= 2
            out.append(([_snapshot(rows) for rows in runner._prev_rows], runner.sampling_rounds))
        finally:
            runner.close_envs()
    (a, rounds), (b, rounds_b) = out
    assert rounds == rounds_b
    for split in range(2):
        _same(a[split], b[split], f"split {split}")
        agents = [(w * I + split) * n + i for w in range(W) for i in range(n)]
        want = _expected_last_frames(agents, rounds * T, "area", True)
        for t in range(T + 1):
            assert np.array_equal(a[split]["obs.obs"][:, t, K - 1:], want[:, (rounds - 1) * T + t]), (split, t)


# ------------------------------------------------------------------------------------------------ enjoy
def test_enjoy_picks_the_three_flags_up_from_the_saved_config(tmp_path):
    from sample_factory_amd.cfg.arguments import load_from_checkpoint, parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    _, _, _, runner = run(True, iters=1, train_dir=str(tmp_path), experiment="rs_enjoy",
                          device_resize_interpolation="nearest", **GRAY_STACK)
    conv1 = next(v for v in runner.learner.actor_critic.state_dict().values() if v.dim() == 4)
    assert conv1.shape[1] == K  # conv1 reads k grey planes
    runner.learner.save()
    del runner
    argv = ["--env=rs_raw_frames", f"--train_dir={tmp_path}", "--experiment=rs_enjoy", "--max_num_episodes=2"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    ecfg = parse_full_cfg(parser, argv)
    assert ecfg.device_resize == [] and ecfg.device_grayscale is False and ecfg.device_resize_interpolation == "area"
    loaded = load_from_checkpoint(parse_full_cfg(parser, argv))   # not given here: they come from config.json
    assert loaded.device_resize == list(OUT) and loaded.device_grayscale is True
    assert loaded.device_resize_interpolation == "nearest" and loaded.hwc_observations is True and loaded.device_framestack == K
    status, avg = enjoy(ecfg)  # (loading the checkpoint into a model built for native 90 x 64 x 3 frames would raise)
    # the reward script pays ((agent + s) % 5) / 4 per step: any finished episode has a return in [0, 4 * 1.0]
    assert status == 0 and 0.0 <= avg <= 4.0


# ------------------------------------------------------------------------------------------------ refusals
def test_set_up_refusals():
    from sample_factory_amd.envs.cartpole import make_cartpole_env
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.train import make_runner
    with pytest.raises(ValueError, match="device_resize"):
        make_runner(_cfg(True, device_resize=[36]))[1].init()
    with pytest.raises(ValueError, match="only shrinks"):
        make_runner(_cfg(True, device_resize=[100, 64]))[1].init()
    with pytest.raises(ValueError, match="3 \\(R, G, B\\)"):
        make_runner(_cfg(True, hwc=False, device_grayscale=True, rs_test_host=[36, 36, "area", True]))[1].init()   # one plane
    register_env("rs_cartpole_vec", make_cartpole_env)
    with pytest.raises(ValueError, match="three dimensions"):
        make_runner(_cfg(True, hwc=False, env="rs_cartpole_vec", cartpole_num_agents=N, device_resize=[8, 8]))[1].init()
    register_env("rs_synthetic_atari", make_synthetic_env)
    with pytest.raises(NotImplementedError, match="step_into"):
        make_runner(_cfg(True, hwc=False, env="rs_synthetic_atari", synthetic_num_agents=N, device_resize=[42, 42]))[1].init()
