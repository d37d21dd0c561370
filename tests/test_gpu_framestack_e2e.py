"""--device_framestack end to end: a scripted HOST vector env delivers ONE u8 frame per step whose pixels encode (agent,
episode, step); the Runner keeps the 4-frame stack in the slab.  Every column of every rollout must equal a numpy deque
reference, and the run must be bit-identical to one where the env stacks on the host and the flag is 1.

Frames are (1, 20, 20): the smallest square frame convnet_impala (8x8 / 4, then 4x4 / 2) still maps to a 1x1 feature map.
The learning rate is 0, so that the weights — and with them actions, log-probs and values of later rollouts — do not depend
on the summation order of the weight-gradient kernels; the learner still runs every launch of its step."""
import os
import subprocess
import sys
from collections import deque

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd.envs import spaces  # noqa: E402

pytestmark = pytest.mark.gpu

K, T, N = 4, 4, 8
SHAPE = (1, 20, 20)
_IDX = np.arange(int(np.prod(SHAPE))).reshape(SHAPE)


# ------------------------------------------------------------------------------------------------ the script
def frame_of(agent: int, episode: int, step: int) -> np.ndarray:
    f = ((_IDX * 3 + agent * 7 + episode * 13 + step * 29) % 251).astype(np.uint8)
    f[0, 0, :3] = (agent, episode, step)
    return f


def flags_of(agent: int, s: int):
    """(terminated, truncated) of the env step with global index s (0 = the first step after reset).  With T = 4: agents 0
    and 4 end at step 0 of every rollout, agents 1 and 5 at the last step (agent 1 at s = 3 by both flags), agent 2 at
    s = 7 by truncation alone"""
    return (s + agent) % 4 == 0, (s + 3 * agent) % 7 == 6


def vec_of(agent, episode, step):
    return np.array([agent, episode, step], np.float32)


def reference(agents, steps):
    """deque reference: (stacks [len(agents), steps + 1, K * C, H, W], vectors [.., steps + 1, 3]); index s = the
    observation after s env steps (0: the reset observation)"""
    stacks = np.zeros((len(agents), steps + 1, K * SHAPE[0]) + SHAPE[1:], np.uint8)
    vecs = np.zeros((len(agents), steps + 1, 3), np.float32)
    for i, a in enumerate(agents):
        episode, step = 0, 0
        d = deque([frame_of(a, 0, 0)] * K, maxlen=K)
        stacks[i, 0], vecs[i, 0] = np.concatenate(list(d)), vec_of(a, 0, 0)
        for s in range(steps):
            done = any(flags_of(a, s))
            episode, step = (episode + 1, 0) if done else (episode, step + 1)
            for _ in range(K if done else 1):
                d.append(frame_of(a, episode, step))
            stacks[i, s + 1], vecs[i, s + 1] = np.concatenate(list(d)), vec_of(a, episode, step)
    return stacks, vecs


# ------------------------------------------------------------------------------------------------ the env
class ScriptedFrameVecEnv:
    """auto-resetting host vector env; nothing depends on the actions"""

    def __init__(self, num_agents, agent0, dict_obs=False):
        self.num_agents, self.agent0, self.dict_obs = int(num_agents), int(agent0), bool(dict_obs)
        sp = {"obs": spaces.Box(0, 255, SHAPE, np.uint8)}
        if dict_obs:
            sp["vec"] = spaces.Box(-1e6, 1e6, (3,), np.float32)
        self.observation_space = spaces.Dict(sp)
        self.action_space = spaces.Discrete(3)
        self.is_multiagent = True

    def _obs(self):
        ids = range(self.agent0, self.agent0 + self.num_agents)
        o = {"obs": np.stack([frame_of(a, e, t) for a, e, t in zip(ids, self.episode, self.step_in_ep)])}
        if self.dict_obs:
            o["vec"] = np.stack([vec_of(a, e, t) for a, e, t in zip(ids, self.episode, self.step_in_ep)])
        return o

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


class HostStacker:
    """what gym.wrappers.FrameStack does around an auto-resetting vector env, in numpy: the parent's pipeline"""

    def __init__(self, env, k):
        self.env, self.k, self.num_agents, self.is_multiagent = env, k, env.num_agents, True
        sp = dict(env.observation_space.spaces)
        c, h, w = sp["obs"].shape
        sp["obs"] = spaces.Box(0, 255, (k * c, h, w), np.uint8)
        self.observation_space, self.action_space = spaces.Dict(sp), env.action_space

    def _out(self, o):
        return dict(o, obs=np.stack([np.concatenate(list(d)) for d in self.d]))

    def reset(self, **kwargs):
        o, info = self.env.reset(**kwargs)
        self.d = [deque([f] * self.k, maxlen=self.k) for f in o["obs"]]
        return self._out(o), info

    def step(self, actions):
        o, rew, te, tr, info = self.env.step(actions)
        for d, f, done in zip(self.d, o["obs"], te | tr):
            for _ in range(self.k if done else 1):
                d.append(f)
        return self._out(o), rew, te, tr, info

    def close(self):
        self.env.close()


def make_scripted_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = int(getattr(cfg, "fs_test_agents", N))
    env_id = int(getattr(env_config, "env_id", 0) or 0)
    env = ScriptedFrameVecEnv(n, env_id * n, dict_obs=full_env_name.endswith("_dict"))
    k = int(getattr(cfg, "fs_test_host_stack", 1))
    return HostStacker(env, k) if k > 1 else env


def _stacked(sampler):
    """key -> channels of one frame, for the keys the device stacks"""
    return {k: r.key.frame_shape[0] for k, r in sampler.routes.items() if r.key.k > 1}


def _cfg(**kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    register_env("fs_scripted", make_scripted_env)
    register_env("fs_scripted_dict", make_scripted_env)
    base = dict(env="fs_scripted", use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_impala", encoder_conv_mlp_layers=[32], encoder_mlp_layers=[16],
                rollout=T, batch_size=N * T, num_batches_per_epoch=1, num_epochs=1, num_workers=1, num_envs_per_worker=1,
                worker_num_splits=1, async_rl=False, serial_mode=True, seed=11, env_gpu_observations=False,
                env_gpu_actions=False, env_workers_mode="inline", learning_rate=0.0, device_framestack=K, fs_test_agents=N)
    base.update(kw)
    return default_cfg(**base)


FIELDS = ("actions", "action_logits", "log_prob_actions", "rewards", "dones", "time_outs")


def _snapshot(rows):
    snap = {f: rows[f].cpu().numpy().copy() for f in FIELDS}
    snap["values"] = rows["values"][:, :T].cpu().numpy().copy()
    for k, v in rows["obs"].items():
        snap["obs." + k] = v.cpu().numpy().copy()
    return snap


def run_inline(iters=4, **kw):
    """sync mode, the env in this process: (one slab snapshot per iteration, h2d bytes, program replays, runner)"""
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_cfg(**kw))
    assert runner.init() == 0
    # stacked on the device or by the env: the slab, the model and the learner see K frames per observation
    assert runner.env_info.obs_space["obs"].shape == (K * SHAPE[0],) + SHAPE[1:]
    assert runner.traj["obs"]["obs"].shape[2:] == (K * SHAPE[0],) + SHAPE[1:]
    snaps = []
    for _ in range(iters):
        assert runner.iteration() is not None
        torch.cuda.synchronize()
        snaps.append(_snapshot(runner._prev_rows[0]))
    return snaps, sum(sm.h2d_bytes for sm in runner.samplers), sum(sm.program_replays for sm in runner.samplers), runner


@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    snaps, h2d, replays, runner = run_inline(train_dir=str(tmp_path_factory.mktemp("fs_device")))
    return snaps, h2d, replays


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    snaps, h2d, replays, runner = run_inline(device_framestack=1, fs_test_host_stack=K,
                                             train_dir=str(tmp_path_factory.mktemp("fs_host")))
    return snaps, h2d, replays


# ------------------------------------------------------------------------------------------------ (a) (b) (c)
def test_every_column_of_every_rollout_equals_the_deque_reference(device_run):
    snaps, _, _ = device_run
    want, _ = reference(range(N), len(snaps) * T)
    assert snaps[0]["obs.obs"].shape == (N, T + 1, K * SHAPE[0]) + SHAPE[1:]
    for r, snap in enumerate(snaps):
        for t in range(T + 1):  # t = 0 of rollouts 1.. is the carried column
            np.testing.assert_array_equal(snap["obs.obs"][:, t], want[:, r * T + t], err_msg=f"rollout {r} column {t}")
        te, tr = np.array([[flags_of(a, r * T + t) for t in range(T)] for a in range(N)]).transpose(2, 0, 1)
        np.testing.assert_array_equal(snap["dones"], te | tr)
        np.testing.assert_array_equal(snap["time_outs"], tr)
    # the script does what the docstring of flags_of says: ends at step 0 and at the last step of a rollout, one by
    # truncation alone
    assert flags_of(0, 0)[0] and flags_of(4, 4)[0] and flags_of(1, 3) == (True, True) and flags_of(2, 7) == (False, True)


def test_slabs_are_bit_identical_to_stacking_on_the_host(device_run, host_run):
    dev, host = device_run[0], host_run[0]
    assert len(dev) == len(host)
    for r, (a, b) in enumerate(zip(dev, host)):
        assert sorted(a) == sorted(b)
        for f in a:
            assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f"rollout {r}: {f} differs"
    assert np.abs(dev[-1]["values"]).max() > 0 and np.isfinite(dev[-1]["log_prob_actions"]).all()


def test_the_obs_share_of_the_h2d_bytes_is_a_quarter(device_run, host_run):
    steps = len(device_run[0]) * T
    other = steps * N * (4 + 1 + 1)             # rewards f32, terminated, truncated of every step; same in both runs
    frame = int(np.prod(SHAPE))
    assert device_run[1] - other == (steps + 1) * N * frame          # one frame per agent and step, and the reset
    assert host_run[1] - other == (steps + 1) * N * K * frame
    assert 4 * (device_run[1] - other) == host_run[1] - other


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
def test_env_worker_processes_two_splits(async_rl):
    """2 workers x 2 instances x 4 agents dealt to 2 splits (rows ordered split; worker, instance, agent); the frames come
    out of the workers' shared pages by DMA into the last slot of the column"""
    from sample_factory_amd.train import make_runner
    W, I, n = 2, 2, 4
    cfg, runner = make_runner(_cfg(num_workers=W, num_envs_per_worker=I, worker_num_splits=2, serial_mode=False,
                                   env_workers_mode="auto", async_rl=async_rl, fs_test_agents=n, batch_size=W * I * n * T // 2,
                                   num_batches_per_epoch=2))
    assert runner.init() == 0
    try:
        assert runner.parallel_envs is not None and len(runner.envs) == 2 and runner.envs[0].num_agents == W * n
        assert all(sm.async_env and sm.host_env and _stacked(sm) == {"obs": 1} for sm in runner.samplers)
        trained = 0
        for _ in range(4):
            trained += runner.iteration() is not None
        runner.stop_sampler_thread()
        torch.cuda.synchronize()
        assert trained >= 3
        rounds = runner.sampling_rounds
        for split in range(2):
            rows = runner._prev_rows[split]["obs"]["obs"].cpu().numpy()  # the split's last rollout
            assert rows.shape[:3] == (W * n, T + 1, K)
            agents = [(w * I + split) * n + i for w in range(W) for i in range(n)]  # env_id = w * I + split (one per split)
            want, _ = reference(agents, rounds * T)
            for t in range(T + 1):
                np.testing.assert_array_equal(rows[:, t], want[:, (rounds - 1) * T + t], err_msg=f"split {split} column {t}")
        frame = int(np.prod(SHAPE))
        assert sum(sm.h2d_bytes for sm in runner.samplers) == 2 * W * n * ((rounds * T + 1) * frame + rounds * T * 6)
    finally:
        runner.close_envs()


# ------------------------------------------------------------------------------------------------ (e)
def test_launch_programs_off_gives_the_same_bits(device_run, tmp_path):
    """the same run in a fresh process with SF_LAUNCH_PROGRAMS=0; here (programs on) rollouts 3 and 4 replayed theirs"""
    from sample_factory_amd import lib
    snaps, _, replays = device_run
    if lib.LAUNCH_PROGRAMS:
        assert replays > 0
    out = str(tmp_path / "plain.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, SF_LAUNCH_PROGRAMS="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = np.load(out)
    assert int(plain["replays"]) == 0
    for r_, snap in enumerate(snaps):
        for f, v in snap.items():
            assert v.tobytes() == plain[f"{r_}.{f}"].tobytes(), f"rollout {r_}: {f} differs with launch programs off"


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("normalize_input", [False, True], ids=["raw", "normalize_input"])
def test_dict_env_stacks_the_image_key_only(normalize_input):
    snaps, h2d, _, runner = run_inline(iters=2, env="fs_scripted_dict", normalize_input=normalize_input)
    assert runner.sampler.multi_key and _stacked(runner.sampler) == {"obs": 1}
    assert runner.env_info.obs_space["obs"].shape == (K,) + SHAPE[1:] and runner.env_info.obs_space["vec"].shape == (3,)
    assert runner.env.observation_space["obs"].shape == SHAPE
    stacks, vecs = reference(range(N), 2 * T)
    for r, snap in enumerate(snaps):
        assert snap["obs.vec"].shape == (N, T + 1, 3)
        np.testing.assert_array_equal(snap["obs.obs"], stacks[:, r * T:r * T + T + 1])
        np.testing.assert_array_equal(snap["obs.vec"], vecs[:, r * T:r * T + T + 1])
    assert h2d == (2 * T + 1) * N * (int(np.prod(SHAPE)) + 12) + 2 * T * N * 6


# ------------------------------------------------------------------------------------------------ (g)
def test_enjoy_rebuilds_the_pipeline_from_the_saved_config(tmp_path):
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    _, _, _, runner = run_inline(iters=1, train_dir=str(tmp_path), experiment="fs_enjoy")
    runner.learner.save()
    del runner
    argv = ["--env=fs_scripted", f"--train_dir={tmp_path}", "--experiment=fs_enjoy", "--max_num_episodes=2"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    ecfg = parse_full_cfg(parser, argv)
    assert ecfg.device_framestack == 1  # not given here: it comes from config.json (the policy's conv1 has K input channels)
    status, avg = enjoy(ecfg)
    # the reward script pays ((agent + s) % 5) / 4 per step: any finished episode has a return in [0, 4 * 1.0]
    assert status == 0 and 0.0 <= avg <= 4.0


# ------------------------------------------------------------------------------------------------ (h)
def test_set_up_refusals():
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.envs.cartpole import make_cartpole_env
    from sample_factory_amd.train import make_runner
    with pytest.raises(ValueError, match="device_framestack=0"):
        make_runner(_cfg(device_framestack=0))[1].init()
    register_env("fs_cartpole_vec", make_cartpole_env)
    with pytest.raises(ValueError, match="three dimensions"):
        make_runner(_cfg(env="fs_cartpole_vec", cartpole_num_agents=N, device_framestack=2))[1].init()
    register_env("fs_synthetic_atari", make_synthetic_env)
    with pytest.raises(NotImplementedError, match="step_into"):
        make_runner(_cfg(env="fs_synthetic_atari", synthetic_num_agents=N, device_framestack=2))[1].init()


if __name__ == "__main__":  # child of test_launch_programs_off_gives_the_same_bits
    snaps_, _, replays_, _ = run_inline(train_dir=os.path.join(os.path.dirname(sys.argv[1]), "train_dir"))
    np.savez(sys.argv[1], replays=replays_, **{f"{r}.{f}": v for r, s in enumerate(snaps_) for f, v in s.items()})
