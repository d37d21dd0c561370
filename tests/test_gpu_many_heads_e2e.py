"""Tuple action spaces of more than eight members through the whole engine: env -> policy forward -> sampler -> slab ->
Learner.train (V-trace, sf_ppo_loss_heads, heads gradients) -> Adam; replayed launch programs; host envs in worker
processes; the deterministic rollout of enjoy.  Seventeen Discrete(5) members (85 logits: the lane-per-sample kernels)
and seventeen Discrete(11) (187 logits, a discretised Humanoid: the wave-per-row kernels)."""
import numpy as np
import pytest
import torch

from sample_factory_amd.envs import spaces

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def _tuple_cfg(head_sizes, **over):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_tuple_env
    register_env("synthetic_tuple", make_synthetic_tuple_env)
    kw = dict(env="synthetic_tuple", use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
              encoder_conv_architecture="convnet_atari", rollout=8, recurrence=8, batch_size=256, num_batches_per_epoch=2,
              num_epochs=1, num_workers=1, num_envs_per_worker=1, async_rl=False, seed=2, serial_mode=True,
              synthetic_num_agents=64, kl_loss_coeff=0.05, synthetic_head_sizes=head_sizes,
              normalize_returns=False, shuffle_minibatches=False)
    kw.update(over)
    return default_cfg(**kw)


def check_recorded_logp(tr, n_members, n):
    """recorded log-prob = float64 sum of the members' log-softmax at the recorded actions, to the members' logp_tol"""
    from test_gpu_action_heads import logp_tol
    a = tr["actions"]
    lg = tr["action_logits"].double().view(a.shape[0], a.shape[1], n_members, n)
    lp_h = torch.log_softmax(lg, -1).gather(-1, a.long().unsqueeze(-1)).squeeze(-1).cpu().numpy()
    tol = logp_tol(lp_h, n).sum(-1)
    err = np.abs(lp_h.sum(-1) - tr["log_prob_actions"].double().cpu().numpy())
    assert np.all(err < tol), (err.max(), tol.min())


@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
@pytest.mark.parametrize("with_vtrace", [False, True], ids=["gae", "vtrace"])
@pytest.mark.parametrize("n", [5, 11])
def test_seventeen_head_tuple_end_to_end(lib, n, with_vtrace, async_rl):
    """the assertions of test_eight_head_tuple_with_vtrace_end_to_end on seventeen members: actions integral and in
    range, everything finite, the parameters change, the state_dict round-trips"""
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_tuple_cfg((n,) * 17, with_vtrace=with_vtrace, async_rl=async_rl, serial_mode=not async_rl))
    runner.init()
    ac = runner.learner.actor_critic
    assert runner.learner._head_sizes == [n] * 17 and runner.learner.loss_cfg.num_heads == 0
    assert ac.num_action_params == 17 * n and runner.traj["actions"].shape[1:] == (8, 17)
    p0 = ac.flat_params.clone()
    stats, trained = None, 0
    for _ in range(5):  # (async_rl: the first round only samples)
        out = runner.iteration()
        stats, trained = (out, trained + 1) if out is not None else (stats, trained)
    if async_rl:
        runner.stop_sampler_thread()
    torch.cuda.synchronize()
    assert trained >= 3
    tr = runner.traj
    a = tr["actions"]
    assert ((a >= 0) & (a < n) & (a == a.round())).all()
    assert torch.isfinite(tr["log_prob_actions"]).all() and torch.isfinite(tr["action_logits"]).all()
    assert torch.isfinite(tr["values"]).all()
    assert np.isfinite(stats["train"]["loss"]) and stats["train"]["kl_divergence"] >= -1e-6
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(p0, ac.flat_params)
    check_recorded_logp(tr, 17, n)
    sd = {k: v.clone() for k, v in ac.state_dict().items()}
    flat = ac.flat_params.clone()
    ac.flat_params.zero_()
    ac.load_state_dict(sd)
    assert torch.equal(flat, ac.flat_params)
    sd2 = ac.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_replayed_rollouts_equal_the_wrapper_path_with_seventeen_heads():
    """5 iterations with launch programs against the same run through the wrappers: every slab leaf, the parameters and
    the episode statistics bit for bit (the pattern of tests/test_gpu_launch_programs.py; the recorded sampler call holds
    the converted 17-entry head array)"""
    import ctypes as C
    from sample_factory_amd import lib
    from test_gpu_launch_programs import _run, _same_run
    over = dict(synthetic_head_sizes=(5,) * 17)
    plain = _run("conv_tuple_mixed", False, 5, **over)
    prog = _run("conv_tuple_mixed", True, 5, **over)
    _same_run(plain, prog)
    for s in prog["samplers"]:
        assert s.heads == [5] * 17 and s.program_replays >= s.T
        pol = [p for k, p in s._progs.items() if isinstance(p, lib.LaunchProgram) and k[0] == "policy"]
        assert pol and all(p.unsafe is None for p in pol)
        for p in pol:
            fn, args, name, _ = p.calls[-1]
            assert name == "sf_sample_write_step_tuple"
            assert [list(x) for x in args if isinstance(x, C.Array)] == [[5] * 17]
    assert prog["slabs"][-1]["actions"].shape[-1] == 17


class HostTupleVecEnv:
    """HOST vector env with a ten-member Tuple(Discrete(3)) action space: the observation of step t + 1 spells out the
    action array step t received — [sum over the members, member 0, member 9, step count] — so the slab shows whether
    the [agents, 10] int32 rows reached the env instance of every slab row"""

    def __init__(self, num_agents=16, seed=0):
        self.num_agents = int(num_agents)
        self.observation_space = spaces.Dict({"obs": spaces.Box(-1e6, 1e6, (4,), np.float32)})
        self.action_space = spaces.Tuple([spaces.Discrete(3) for _ in range(10)])
        self.step_count = 0

    def reset(self, **kwargs):
        self.step_count = 0
        return {"obs": np.zeros((self.num_agents, 4), np.float32)}, {}

    def step(self, actions):
        a = np.asarray(actions)
        assert a.shape == (self.num_agents, 10) and a.dtype == np.int32, (a.shape, a.dtype)
        self.step_count += 1
        obs = np.stack([a.sum(1), a[:, 0], a[:, 9], np.full(self.num_agents, self.step_count)], 1).astype(np.float32)
        rew = (a[:, 0] == self.step_count % 3).astype(np.float32)
        return {"obs": obs}, rew, np.zeros(self.num_agents, bool), np.zeros(self.num_agents, bool), {}

    def close(self):
        pass


def make_host_tuple_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    return HostTupleVecEnv(num_agents=16, seed=int(getattr(env_config, "env_id", 0) or 0))


def test_ten_member_host_env_through_worker_processes(lib):
    """2 worker processes x 2 instances x 16 agents, two splits: the workers' shared action arrays are [agents, 10] int32;
    every observation in the slab is the one its env instance built from the action row recorded one step earlier"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.train import make_runner
    register_env("host_tuple10", make_host_tuple_env)
    T = 8
    cfg = default_cfg(env="host_tuple10", use_rnn=False, nonlinearity="tanh", normalize_input=False,
                      encoder_mlp_layers=[32], rollout=T, batch_size=256, num_batches_per_epoch=2, num_epochs=1,
                      num_workers=2, num_envs_per_worker=2, worker_num_splits=2, async_rl=False, serial_mode=False, seed=4,
                      env_gpu_observations=False, env_gpu_actions=False)
    cfg, runner = make_runner(cfg)
    runner.init()
    try:
        assert runner.parallel_envs is not None and runner.parallel_envs.heads == [3] * 10
        assert all(sm.async_env and sm.host_env and sm.heads == [3] * 10 for sm in runner.samplers)
        trained = 0
        for _ in range(3):
            trained += runner.iteration() is not None
        runner.stop_sampler_thread()
        torch.cuda.synchronize()
        assert trained >= 2 and torch.isfinite(runner.learner.actor_critic.flat_params).all()
        for split in range(2):
            rows = runner._prev_rows[split]
            obs, a = rows["obs"]["obs"].cpu().numpy(), rows["actions"].cpu().numpy()
            assert a.shape == (32, T, 10) and obs.shape == (32, T + 1, 4)
            assert np.all((a >= 0) & (a < 3) & (a == np.round(a)))
            np.testing.assert_array_equal(obs[:, 1:, 0], a.sum(-1))
            np.testing.assert_array_equal(obs[:, 1:, 1], a[:, :, 0])
            np.testing.assert_array_equal(obs[:, 1:, 2], a[:, :, 9])
            assert len(np.unique(a)) == 3
    finally:
        runner.close_envs()


def test_deterministic_rollout_with_seventeen_heads(lib):
    """rollout(deterministic=True) after a training step: every member's recorded action is the arg-max of its recorded
    logits, the recorded log-prob the float64 sum of the members' maxima of the log-softmax"""
    from sample_factory_amd.train import make_runner
    from test_gpu_action_heads import logp_tol
    cfg, runner = make_runner(_tuple_cfg((5,) * 17, seed=3))
    runner.init()
    runner.iteration()  # one training step: logits that are no longer the initial near-ties
    runner.sampler.rollout(deterministic=True)
    torch.cuda.synchronize()
    tr = runner.traj
    a = tr["actions"]
    lg = tr["action_logits"].view(a.shape[0], 8, 17, 5)
    assert torch.equal(a.long(), lg.argmax(-1))
    lp = torch.log_softmax(lg.double(), -1).max(-1).values.cpu().numpy()
    err = np.abs(lp.sum(-1) - tr["log_prob_actions"].double().cpu().numpy())
    assert np.all(err < logp_tol(lp, 5).sum(-1))


def test_enjoy_deterministic_with_seventeen_heads(lib, tmp_path):
    """enjoy() with --eval_deterministic on a saved 17-member policy: the evaluation loop runs the deterministic sampler"""
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    from sample_factory_amd.train import make_runner
    # (a list: config.json, which enjoy reads the env's head sizes back from, keeps JSON types)
    cfg = _tuple_cfg([5] * 17, train_dir=str(tmp_path), experiment="many_heads", train_for_env_steps=64 * 8 * 2,
                     save_every_sec=100000)
    cfg, runner = make_runner(cfg)
    assert runner.init() == 0 and runner.run() == 0
    del runner
    argv = ["--env=synthetic_tuple", f"--train_dir={tmp_path}", "--experiment=many_heads", "--eval_deterministic=True",
            "--max_num_frames=16", "--max_num_episodes=1000000"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    status, avg = enjoy(parse_full_cfg(parser, argv))
    assert status == 0 and np.isfinite(avg)
