"""Statistics an env defines itself, through the runner: the two envs of envs/synthetic.py that report
true_objective and episode_extra_stats — as a dict of device tensors, and as per-agent dicts on the host — in sync mode, in
async mode with the sampler thread, inline and behind two env worker processes.

The check is the envs' own ledger of finished episodes.  A report carries, per key, the MEAN over the episodes since the
previous report and their count (under episodes, or episodes_<key> where it differs), so mean x count is that report's
sum up to one rounding of the division and one of the product (relative 2^-52 each).  Every statistic of these envs is an
integer far below 2^40: rounding mean x count to the nearest integer gives the report's sum EXACTLY, and the device path
is compared with == on those integers.  The host path is held to 1e-9 relative on the unrounded products.

A run of synthetic_atari, whose env reports nothing, emits the keys it always emitted and never calls the new launch."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

T = 8
KEYS = ("true_objective", "first_action", "len_parity")


def _cfg(tmp_path, env, agents, **kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import (make_episode_stats_host_env, make_episode_stats_vec_env,
                                                   make_synthetic_env)
    register_env("episode_stats_vec", make_episode_stats_vec_env)
    register_env("episode_stats_host", make_episode_stats_host_env)
    register_env("synthetic_atari", make_synthetic_env)
    base = dict(env=env, use_rnn=False, nonlinearity="tanh", normalize_input=False, normalize_returns=False,
                encoder_mlp_layers=[32], rollout=T, batch_size=agents * T, num_batches_per_epoch=1, num_epochs=1,
                num_workers=1, num_envs_per_worker=1, worker_num_splits=1, async_rl=False, serial_mode=True, seed=3,
                synthetic_num_agents=agents, train_dir=str(tmp_path), experiment="eps", save_best_after=0)
    base.update(kw)
    return default_cfg(**base)


def _count(monkeypatch, name):
    from sample_factory_amd import lib
    real, count = getattr(lib, name), [0]

    def counted(*a, **kw):
        count[0] += 1
        return real(*a, **kw)
    monkeypatch.setattr(lib, name, counted)
    return count


def _run(cfg, iters, emit_every=2):
    """the runner after `iters` iterations and every EPISODIC message it processed on the way (reports in between, one at
    the end after the sampler thread has stopped)"""
    from sample_factory_amd.algo.utils.misc import EPISODIC
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(cfg)
    msgs = []
    runner.register_episodic_stats_handler(lambda r, msg, pid: msgs.append(dict(msg[EPISODIC])))
    assert runner.init() == 0
    try:
        for i in range(iters):
            runner.iteration()
            if (i + 1) % emit_every == 0:
                runner._emit_episodic_stats()
        runner.stop_sampler_thread()
        torch.cuda.synchronize()
        runner._emit_episodic_stats()
    except BaseException:
        runner.close_envs()
        raise
    return runner, msgs


def _totals(msgs):
    """key -> [sum over reports of mean x count (each product as it is, and rounded to an integer), sum of counts]"""
    tot = {}
    for m in msgs:
        for k, mean in m.items():
            if k.startswith("episodes"):
                continue
            n = m.get(f"episodes_{k}", m.get("episodes", 0.0))
            s = tot.setdefault(k, [0.0, 0, 0.0])
            s[0] += mean * n
            s[1] += int(round(mean * n))
            s[2] += n
    return tot


def _ledger_totals(pairs):
    tot = {}
    for k, v in pairs:
        s = tot.setdefault(k, [0.0, 0.0])
        s[0] += v
        s[1] += 1
    return tot


def _check(msgs, want, exact):
    got = _totals(msgs)
    assert set(got) == {"reward", "len"} | set(KEYS), sorted(got)
    for k in sorted(got):
        print(f"{k}: reported sum {got[k][0]!r} (rounded {got[k][1]}), count {got[k][2]}; ledger {want[k]}")
    for k in got:
        assert got[k][2] == want[k][1] > 0, (k, got[k], want[k])
        if exact:
            assert got[k][1] == want[k][0], (k, got[k], want[k])
        assert abs(got[k][0] - want[k][0]) <= 1e-9 * max(1.0, abs(want[k][0])), (k, got[k], want[k])
    # every key finished with every episode here: no per-key counts in the messages
    assert not any(k.startswith("episodes_") for m in msgs for k in m)
    assert sum(m.get("episodes", 0) for m in msgs) == want["len"][1]


@pytest.mark.parametrize("mode", ["sync", "async_thread"])
def test_device_env_dict_infos(tmp_path, monkeypatch, mode):
    extra = dict(async_rl=True, serial_mode=False, sampler_thread=True) if mode == "async_thread" else {}
    adds = _count(monkeypatch, "episode_stats_add")
    runner, msgs = _run(_cfg(tmp_path, "episode_stats_vec", 48, env_gpu_observations=True, env_gpu_actions=True, **extra), 5)
    try:
        sm = runner.sampler
        assert sm.host_env is False and not sm.zero_copy and runner.threaded == (mode == "async_thread")
        assert sm._stat_dev == ["true_objective", "episode_extra_stats/first_action", "episode_extra_stats/len_parity"]
        assert adds[0] == sm.global_step >= 2 * T  # one launch per env step, whatever the number of channels
        want = _ledger_totals(runner.env.ledger)
        _check(msgs, want, exact=True)
        assert "junk" not in runner.policy_avg_stats and "true_objective" in runner.policy_avg_stats
    finally:
        runner.close_envs()


def test_host_env_list_infos_inline(tmp_path, monkeypatch):
    adds = _count(monkeypatch, "episode_stats_add")
    runner, msgs = _run(_cfg(tmp_path, "episode_stats_host", 16, env_gpu_observations=False, env_gpu_actions=False), 5)
    try:
        assert runner.sampler.host_env is True and runner.parallel_envs is None and adds[0] == 0
        _check(msgs, _ledger_totals(runner.env.ledger), exact=False)
    finally:
        runner.close_envs()


def test_host_env_two_worker_processes(tmp_path, monkeypatch):
    adds = _count(monkeypatch, "episode_stats_add")
    led = tmp_path / "ledgers"
    led.mkdir()
    runner, msgs = _run(_cfg(tmp_path, "episode_stats_host", 16, num_workers=2, serial_mode=False, env_workers_mode="process",
                             env_gpu_observations=False, env_gpu_actions=False, batch_size=2 * 16 * T,
                             synthetic_ledger_dir=str(led)), 5)
    try:
        assert runner.parallel_envs is not None and runner.sampler.async_env and runner.sampler.B == 32 and adds[0] == 0
    finally:
        runner.close_envs()
    files = sorted(glob.glob(str(led / "ledger_*.jsonl")))
    assert [os.path.basename(f) for f in files] == ["ledger_0.jsonl", "ledger_1.jsonl"]
    pairs = [kv for f in files for line in open(f) for kv in json.loads(line).items()]
    _check(msgs, _ledger_totals(pairs), exact=False)


def test_an_env_that_reports_nothing_emits_what_it_emitted_and_launches_nothing(tmp_path, monkeypatch):
    adds = _count(monkeypatch, "episode_stats_add")
    cfg = _cfg(tmp_path, "synthetic_atari", 1024, nonlinearity="relu", obs_scale=255.0,
               encoder_conv_architecture="convnet_atari", batch_size=1024 * T // 4, num_batches_per_epoch=4)
    runner, msgs = _run(cfg, 2)
    try:
        sm = runner.sampler
        assert sm.zero_copy and adds[0] == 0 and sm._stat_dev is None and not sm.host_stats
        assert msgs, "1024 agents x 16 steps at a termination rate of 1/1024: some episode has ended"
        assert all(set(m) == {"reward", "len", "episodes"} for m in msgs), msgs
        assert set(runner.policy_avg_stats) == {"reward", "len", "episodes"}
        # ep_stats is still the 3 doubles the record launch adds to, at the front of the one read-back buffer
        assert sm.ep_stats.shape == (3,) and sm.ep_stats.data_ptr() == sm._stats_all.data_ptr()
    finally:
        runner.close_envs()


def test_save_best_metric_takes_a_reported_key_and_enjoy_reports_true_objective(tmp_path, capsys):
    from sample_factory_amd import enjoy as enjoy_mod
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    runner, msgs = _run(_cfg(tmp_path, "episode_stats_vec", 32, env_gpu_observations=True, env_gpu_actions=True,
                             save_best_metric="first_action"), 3)
    try:
        runner._save_best_policy()
        best = glob.glob(str(tmp_path / "eps" / "checkpoint_p0" / "best_*"))
        assert len(best) == 1 and "first_action" in os.path.basename(best[0]), best
        avg = float(np.mean(runner.policy_avg_stats["first_action"][0]))
        assert f"first_action_{avg:.3f}" in os.path.basename(best[0])
        runner._write_summaries(0.0)
        rec = json.loads(open(tmp_path / "eps" / ".summary" / "0" / "summaries.jsonl").read().splitlines()[-1])
        for k in KEYS:
            assert rec[f"policy_stats/avg_{k}"] == float(np.mean(runner.policy_avg_stats[k][0]))
        runner.learner.save()
    finally:
        runner.close_envs()
    del runner
    argv = ["--env=episode_stats_vec", f"--train_dir={tmp_path}", "--experiment=eps", "--max_num_episodes=40"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    capsys.readouterr()
    status, avg_reward = enjoy_mod.enjoy(parse_full_cfg(parser, argv))
    out = capsys.readouterr().out
    stats = enjoy_mod.last_env_stats
    assert status == 0 and set(stats) == set(KEYS)
    assert f"Avg true_objective: {stats['true_objective']:.3f}" in out
    # true_objective = 2 x return + 1 for every episode, so the averages obey it as well
    assert abs(stats["true_objective"] - (2.0 * avg_reward + 1.0)) <= 1e-9 * max(1.0, stats["true_objective"])
