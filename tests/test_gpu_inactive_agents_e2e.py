"""--track_inactive_agents through the whole engine: the scripted TurnBasedMaskedBanditEnv (3 games x 2
agents, rollout 8, GRU-32 MLP policy) -> infos -> sf_traj_write_env_step_active / sf_rnn_store_state_held -> slab ->
Learner.train.  The env reports script[k % 5] with step k, so global step s is recorded with policy_id -1 exactly where
s > 0 and script[(s - 1) % 5] is False: the reference's one-step delay, across rollout boundaries and episode ends."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, GAMES, AGENTS, H, EP_LEN = 8, 3, 6, 32, 5
SCRIPT = np.array([[1, 0, 1, 1, 0, 1],
                   [0, 1, 1, 0, 1, 1],
                   [1, 1, 0, 1, 1, 0],     # reported with step 7: rules step 0 of the second rollout
                   [1, 1, 1, 1, 1, 1],
                   [0, 0, 1, 1, 1, 0]],    # reported with step 4, the step every episode ends at
                  dtype=bool)


def inactive_at(s, rows=AGENTS):
    """bool [rows]: which slab rows record global step s with policy_id -1 (rows repeat per env instance)"""
    one = np.zeros(AGENTS, bool) if s == 0 else ~SCRIPT[(s - 1) % len(SCRIPT)]
    return np.tile(one, rows // AGENTS)


def _cfg(**kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_masked_bandit_env, make_turn_based_masked_bandit_env
    register_env("turn_based_masked_bandit", make_turn_based_masked_bandit_env)
    register_env("masked_bandit", make_masked_bandit_env)
    base = dict(env="turn_based_masked_bandit", use_rnn=True, rnn_type="gru", rnn_size=H, recurrence=T, nonlinearity="tanh",
                normalize_input=False, normalize_returns=False, encoder_mlp_layers=[32], rollout=T, batch_size=AGENTS * T,
                num_batches_per_epoch=1, num_epochs=2, num_workers=1, num_envs_per_worker=1, worker_num_splits=1,
                async_rl=False, serial_mode=True, env_workers_mode="inline", seed=7, learning_rate=1e-2, gamma=0.9,
                env_gpu_observations=False, env_gpu_actions=False, synthetic_num_games=GAMES, synthetic_episode_len=EP_LEN,
                synthetic_active_script=SCRIPT.tolist(), track_inactive_agents=True)
    base.update(kw)
    return default_cfg(**base)


def _flat(td, prefix=""):
    out = {}
    for k, v in td.items():
        if isinstance(v, torch.Tensor):
            out[prefix + k] = v.cpu().numpy().copy()
        else:
            out.update(_flat(v, prefix + k + "."))
    return out


def _snapshot(runner):
    torch.cuda.synchronize()
    ln = runner.learner
    snap = _flat(runner._prev_rows[0])
    snap["~params"] = ln.actor_critic.flat_params.cpu().numpy().copy()
    snap["~exp_avg"], snap["~exp_avg_sq"] = ln.exp_avg.cpu().numpy().copy(), ln.exp_avg_sq.cpu().numpy().copy()
    snap["~num_invalids"] = np.array([ln._global_invalids])
    return snap


def run(iters=2, before_rollouts=None, before_train=None, **kw):
    """sync mode, the env in this process: one snapshot (slab, parameters, Adam moments, num_invalids) per iteration"""
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_cfg(**kw))
    assert runner.init() == 0
    if before_rollouts is not None:
        before_rollouts(runner)
    if before_train is not None:
        real = runner._train_dataset

        def train(ds):
            before_train(runner, ds)
            return real(ds)
        runner._train_dataset = train
    snaps = []
    for _ in range(iters):
        assert runner.iteration() is not None
        snaps.append(_snapshot(runner))
    return snaps, runner


def _same(a, b, skip=()):
    assert sorted(a) == sorted(b)
    return [k for k in a if k not in skip and (a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes())]


@pytest.fixture(scope="module")
def on_run(tmp_path_factory):
    snaps, runner = run(train_dir=str(tmp_path_factory.mktemp("ia_on")))
    return snaps, runner


# ------------------------------------------------------------------------------------------------ (a)
def _check_pattern_and_hold(rows_pid, rows_state, rows_done, s0):
    """one rollout's policy_id / rnn_states / dones columns, first global step s0"""
    n = rows_pid.shape[0]
    held_nonzero = moved = 0
    for t in range(T):
        ina = inactive_at(s0 + t, n)
        np.testing.assert_array_equal(rows_pid[:, t], np.where(ina, -1, 0), err_msg=f"global step {s0 + t}")
        want = np.where(rows_done[:, t, None], np.float32(0.0), rows_state[:, t])
        # (values, not bytes: the torch-model path multiplies by 1 - done and may leave -0.0 where the kernel stores 0.0)
        assert np.array_equal(rows_state[ina, t + 1], want[ina]), f"state not held at global step {s0 + t}"
        held_nonzero += int(np.abs(rows_state[ina, t + 1]).sum() > 0)
        act = ~ina & ~rows_done[:, t]
        moved += int((rows_state[act, t + 1] != rows_state[act, t]).any(1).all())
        assert (rows_state[rows_done[:, t], t + 1] == 0).all()
    return held_nonzero, moved


def test_sync_inline_policy_id_and_held_state_follow_the_script(on_run):
    snaps, runner = on_run
    sm = runner.sampler
    assert sm.track_active and sm.host_env and not sm.async_env and sm.masked and sm.B == AGENTS
    assert runner.parallel_envs is None and runner.learner.actor_critic.new_rnn_parts_of(sm.tag) is not None  # native model
    total = 0
    for r, snap in enumerate(snaps):
        held, moved = _check_pattern_and_hold(snap["policy_id"], snap["rnn_states"], snap["dones"], r * T)
        assert held >= 3 and moved == T
        total += int((snap["policy_id"] == -1).sum())
        assert int(snap["~num_invalids"][0]) == int((snap["policy_id"] == -1).sum())
        assert np.isfinite(snap["~params"]).all()
    assert total == sum(int(inactive_at(s).sum()) for s in range(2 * T)) and total > 0
    # the one-step delay: step 0 is recorded active for everybody, whatever the env thinks
    assert (snaps[0]["policy_id"][:, 0] == 0).all() and (snaps[0]["policy_id"][:, 1] == np.where(SCRIPT[0], 0, -1)).all()
    # the carry across the rollout boundary: the state bytes outlive the rollout, the recurrent state is carried over
    assert (snaps[1]["policy_id"][:, 0] == np.where(SCRIPT[(T - 1) % 5], 0, -1)).all() and not SCRIPT[(T - 1) % 5].all()
    assert snaps[1]["rnn_states"][:, 0].tobytes() == snaps[0]["rnn_states"][:, T].tobytes()
    # a done does not reset the flags: every episode ends at step 4, step 5 still follows the report of step 4
    assert snaps[0]["dones"][:, EP_LEN - 1].all() and (snaps[0]["policy_id"][:, EP_LEN] == np.where(SCRIPT[4], 0, -1)).all()
    # rewards, dones and the sampled fields are written for inactive rows as for the others
    assert np.isfinite(snaps[0]["log_prob_actions"]).all() and snaps[0]["dones"].sum() == AGENTS * (T // EP_LEN)
    # the state is the runner's: the device bytes now hold the report of the last step
    np.testing.assert_array_equal(sm._active.cpu().numpy(), SCRIPT[(2 * T - 1) % 5].astype(np.uint8))


# ------------------------------------------------------------------------------------------------ (b)
def test_env_worker_processes_async_two_splits():
    """2 workers x 2 instances (one per split) x 6 agents, async mode: the flags travel through the shared "active" array,
    every split has its own state bytes, and they survive the switches between slabs"""
    from sample_factory_amd.train import make_runner
    W, I = 2, 2
    cfg, runner = make_runner(_cfg(num_workers=W, num_envs_per_worker=I, worker_num_splits=2, serial_mode=False,
                                   env_workers_mode="process", async_rl=True, batch_size=W * I * AGENTS * T // 2,
                                   num_batches_per_epoch=2, num_epochs=1))
    assert runner.init() == 0
    try:
        assert runner.parallel_envs is not None and len(runner.samplers) == 2
        assert all(sm.async_env and sm.host_env and sm.track_active and sm.B == W * AGENTS for sm in runner.samplers)
        assert runner.samplers[0]._active.data_ptr() != runner.samplers[1]._active.data_ptr()
        assert all("active" in a for a in runner.parallel_envs.arrays)
        slabs = [set(), set()]
        trained = 0
        for _ in range(4):
            trained += runner.iteration() is not None
            for e in range(2):
                slabs[e].add(runner._prev_rows[e]["rewards"].data_ptr())
        runner.stop_sampler_thread()
        torch.cuda.synchronize()
        assert trained >= 3 and runner._thread_error is None
        rounds = runner.sampling_rounds
        assert rounds >= 3
        for e, sm in enumerate(runner.samplers):
            assert sm.global_step == rounds * T
            rows = _flat(runner._prev_rows[e])  # the split's last rollout
            held, moved = _check_pattern_and_hold(rows["policy_id"], rows["rnn_states"], rows["dones"], (rounds - 1) * T)
            assert held >= 3 and moved == T
            np.testing.assert_array_equal(sm._active.cpu().numpy(),
                                          np.tile(SCRIPT[(rounds * T - 1) % 5], W).astype(np.uint8))
        assert max(len(s) for s in slabs) >= 2  # the rollouts moved between slabs
    finally:
        runner.close_envs()


# ------------------------------------------------------------------------------------------------ (c)
def test_record_step_replay_gives_the_bits_of_the_plain_calls_with_as_many_launches(monkeypatch):
    from sample_factory_amd import lib
    monkeypatch.setattr(lib, "LAUNCH_PROGRAMS", True)
    snaps, runner = run(iters=4)  # rollout 1 runs plainly, 2 records, 3 and 4 replay
    sm = runner.sampler
    assert sm.program_replays > 0
    progs = {k: p for k, p in sm._progs.items() if k[0] == "record" and not isinstance(p, bool)}
    assert len(progs) == T and all(p.unsafe is None for p in progs.values())
    for p in progs.values():
        assert [c[2] for c in p.calls] == ["sf_traj_write_env_step_active", "sf_rnn_store_state_held"]
    _, off = run(iters=3, track_inactive_agents=False)
    progs_off = {k: p for k, p in off.sampler._progs.items() if k[0] == "record" and not isinstance(p, bool)}
    assert len(progs_off) == T
    for p in progs_off.values():  # the same number of launches, the parent's
        assert [c[2] for c in p.calls] == ["sf_traj_write_env_step", "sf_rnn_store_state"]
    monkeypatch.setattr(lib, "LAUNCH_PROGRAMS", False)
    plain, runner_plain = run(iters=4)
    assert runner_plain.sampler.program_replays == 0 and not runner_plain.sampler._progs
    for r in range(4):
        assert _same(snaps[r], plain[r]) == [], f"rollout {r}"
        _check_pattern_and_hold(snaps[r]["policy_id"], snaps[r]["rnn_states"], snaps[r]["dones"], r * T)


# ------------------------------------------------------------------------------------------------ (d)
def _patch_by_hand(runner):
    """flag-off runner: after every recorded step, write the policy_id column and the held state of the scripted rows with
    torch indexing — what the two kernels do, done by hand"""
    sm = runner.sampler
    assert not sm.track_active and not hasattr(sm, "_active")
    real = sm._env_step_and_record

    def step(t, env_actions):
        s = sm.global_step
        real(t, env_actions)
        idx = torch.as_tensor(np.flatnonzero(inactive_at(s)), device="cuda")
        if idx.numel():
            tr = sm.traj
            tr["policy_id"][idx, t] = -1
            prev, done = tr["rnn_states"][idx, t], tr["dones"][idx, t].unsqueeze(1)
            tr["rnn_states"][idx, t + 1] = torch.where(done, torch.zeros_like(prev), prev)
    sm._env_step_and_record = step


def test_learner_trains_on_the_slab_as_on_one_patched_by_hand(on_run):
    """Learner.train on the flag-on slab against a flag-off run whose policy_id column and held states are patched by hand,
    step by step, to the same pattern: slab, parameters, Adam moments and num_invalids bit-identical after each of two
    iterations (the second rollout is sampled with the parameters the first update produced).  A third run scrambles
    actions, log-probs and logits of the inactive steps before every update: the same parameters again."""
    snaps, _ = on_run
    by_hand, _ = run(track_inactive_agents=False, before_rollouts=_patch_by_hand)
    for r in range(2):
        assert _same(snaps[r], by_hand[r]) == [], f"iteration {r}"
    assert int(snaps[1]["~num_invalids"][0]) > 0 and np.abs(snaps[1]["~exp_avg"]).max() > 0
    assert snaps[0]["~params"].tobytes() != snaps[1]["~params"].tobytes()

    def scramble(runner, ds):
        tr = runner.traj[ds]
        bad = tr["policy_id"] < 0
        assert bad.any()
        g = torch.Generator(device="cuda")
        g.manual_seed(int(runner.learner.train_step) + 1)
        for k, scale in (("actions", 50.0), ("log_prob_actions", 30.0), ("action_logits", 100.0)):
            x = tr[k]
            noise = torch.randn(x.shape, generator=g, device="cuda") * scale
            m = bad if x.dim() == 2 else bad.unsqueeze(-1)
            x.copy_(torch.where(m, noise.to(x.dtype), x))
    scrambled, _ = run(before_train=scramble)
    for r in range(2):
        ina = snaps[r]["policy_id"] < 0
        diff = _same(snaps[r], scrambled[r], skip=("action_logits",))
        assert diff == [], f"iteration {r}: {diff}"
        a, b = snaps[r]["action_logits"], scrambled[r]["action_logits"]
        assert a[~ina].tobytes() == b[~ina].tobytes() and (a[ina] != b[ina]).any()  # (the scramble was there)


# ------------------------------------------------------------------------------------------------ (e)
def test_flag_off_records_every_step_as_today():
    snaps, runner = run(track_inactive_agents=False)
    assert not runner.sampler.track_active
    for snap in snaps:
        assert (snap["policy_id"] == 0).all() and int(snap["~num_invalids"][0]) == 0


# ------------------------------------------------------------------------------------------------ device env, torch model
class ReportingDictBandit:
    """device env with two vector observation keys (so the torch model can serve it) that reports is_active as a CUDA
    tensor in an infos dict: a contextual bandit on `measurements`, `obs` is noise; episodes of three steps"""

    def __init__(self, num_agents, num_actions=4, seed=0, device="cuda"):
        from sample_factory_amd.envs import spaces
        self.num_agents, self.A, self.device = int(num_agents), int(num_actions), torch.device(device)
        self.is_multiagent = True
        self.observation_space = spaces.Dict({"obs": spaces.Box(-1, 1, (5,), np.float32),
                                              "measurements": spaces.Box(0, 1, (self.A,), np.float32)})
        self.action_space = spaces.Discrete(self.A)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        self.pattern = torch.as_tensor(np.tile(SCRIPT, (1, self.num_agents // AGENTS)), device=self.device)
        self.k = 0

    def _out(self):
        self.target = torch.randint(0, self.A, (self.num_agents,), generator=self.gen, device=self.device)
        return {"obs": torch.rand((self.num_agents, 5), generator=self.gen, device=self.device) * 2 - 1,
                "measurements": torch.nn.functional.one_hot(self.target, self.A).float()}

    def reset(self, **kwargs):
        self.k = 0
        return self._out(), {}

    def step(self, actions):
        rew = (torch.as_tensor(actions, device=self.device).reshape(-1).long() == self.target).float()
        flags = self.pattern[self.k % len(SCRIPT)]
        self.k += 1
        term = torch.full((self.num_agents,), self.k % 3 == 0, dtype=torch.bool, device=self.device)
        return self._out(), rew, term, torch.zeros_like(term), {"is_active": flags}

    def close(self):
        pass


def make_reporting_dict_bandit(full_env_name, cfg=None, env_config=None, render_mode=None):
    return ReportingDictBandit(num_agents=int(cfg.synthetic_num_agents), seed=cfg.seed)


@pytest.mark.parametrize("native", [False, True], ids=["torch_model", "native_multikey"])
def test_device_env_reports_a_cuda_tensor_and_the_torch_model_path_holds_the_state(native, monkeypatch):
    from sample_factory_amd import lib
    from sample_factory_amd.envs.env_utils import register_env
    monkeypatch.setenv("SF_NATIVE_MULTIKEY", "1" if native else "0")
    register_env("reporting_dict_bandit", make_reporting_dict_bandit)
    n = 10 * AGENTS
    seen = []
    real = lib.traj_write_env_step_active

    def spy(*a):
        seen.append(a[-2].data_ptr())
        return real(*a)
    monkeypatch.setattr(lib, "traj_write_env_step_active", spy)
    snaps, runner = run(env="reporting_dict_bandit", synthetic_num_agents=n, batch_size=n * T, env_gpu_observations=True,
                        env_gpu_actions=True, gamma=0.0, learning_rate=3e-3)
    sm, ac = runner.sampler, runner.learner.actor_critic
    assert type(ac).__name__ == ("MultiKeyActorCritic" if native else "TorchPolicyAdapter") and ac.rnn_kind == 0
    assert (ac.new_rnn_parts_of(sm.tag) is None) == (not native)
    assert sm.multi_key and sm.host_env is False and sm.track_active
    # the env's own tensor went into the launch: no copy, no upload
    base = runner.env.pattern.data_ptr()
    assert seen == [base + (s % len(SCRIPT)) * n for s in range(2 * T)]
    for r, snap in enumerate(snaps):
        held, moved = _check_pattern_and_hold(snap["policy_id"], snap["rnn_states"], snap["dones"], r * T)
        assert held >= 2 and moved == T
        assert int(snap["~num_invalids"][0]) == int((snap["policy_id"] == -1).sum()) > 0


# ------------------------------------------------------------------------------------------------ (f)
def test_flag_on_over_an_env_that_never_reports_equals_flag_off():
    """MaskedBanditEnv (a device env; its infos are empty): the new launches run with every flag set"""
    from sample_factory_amd import lib
    kw = dict(env="masked_bandit", synthetic_num_agents=70, batch_size=70 * T, env_gpu_observations=True, env_gpu_actions=True)
    calls = []
    real = lib.traj_write_env_step_active

    def spy(*a):
        calls.append(bool(a[-2].all()))
        return real(*a)
    lib.traj_write_env_step_active = spy
    try:
        on, runner = run(**kw)
    finally:
        lib.traj_write_env_step_active = real
    assert runner.sampler.track_active and runner.sampler.host_env is False and len(calls) == 2 * T and all(calls)
    off, _ = run(track_inactive_agents=False, **kw)
    for r in range(2):
        assert _same(on[r], off[r]) == [], f"iteration {r}"
        assert (on[r]["policy_id"] == 0).all()
    assert on[0]["~params"].tobytes() != on[1]["~params"].tobytes()


# ------------------------------------------------------------------------------------------------ enjoy
def test_enjoy_takes_the_flag_from_config_json(tmp_path, monkeypatch):
    """enjoy shares the runner: with the flag read back from config.json (it is not on the command line) the evaluation
    rollouts go through the two launches, so a waiting agent's recurrent state is held there too"""
    from sample_factory_amd import lib
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    _, runner = run(iters=1, train_dir=str(tmp_path), experiment="ia_enjoy")
    runner.learner.save()
    del runner
    calls = dict(write=0, held=0, plain=0)

    def spy(name, real):
        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f
    monkeypatch.setattr(lib, "traj_write_env_step_active", spy("write", lib.traj_write_env_step_active))
    monkeypatch.setattr(lib, "rnn_store_state_held", spy("held", lib.rnn_store_state_held))
    monkeypatch.setattr(lib, "traj_write_env_step", spy("plain", lib.traj_write_env_step))
    argv = ["--env=turn_based_masked_bandit", f"--train_dir={tmp_path}", "--experiment=ia_enjoy", "--max_num_episodes=2"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    ecfg = parse_full_cfg(parser, argv)
    assert ecfg.track_inactive_agents is False  # not given here: it comes from config.json
    status, avg = enjoy(ecfg)
    assert status == 0 and 0.0 <= avg <= EP_LEN
    assert calls["write"] >= T and calls["held"] == calls["write"] and calls["plain"] == 0
