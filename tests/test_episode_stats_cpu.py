"""Statistics an env defines itself, the host side: the entry point's declaration, the host accumulator
against a hand-written table, the merge of worker replies (in process and through real worker processes), the key
flattening against names recorded from the reference, the EPISODIC message, and what Runner._save_best_policy does with a
reported key, with true_objective when nobody reports it, and with a metric nobody ever reports."""
import json
import logging
import os
import re
import sys
import types
from collections import deque

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd.algo.sampling import episode_stats as es  # noqa: E402


# ------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_is_declared_listed_and_exported():
    import ctypes
    from sample_factory_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+sf_episode_stats_add\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m, "include/sf_hip.h does not declare sf_episode_stats_add"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const sf_epstat_channels *h_ch", "int K", "const uint8_t *terminated", "const uint8_t *truncated",
                    "const uint8_t *active", "int64_t B", "double *acc", "void *stream"]
    assert "#define SF_EPSTAT_MAX_CHANNELS 16" in code and lib.EPSTAT_MAX_CHANNELS == 16
    for name, val in (("F32", 0), ("F64", 1), ("I32", 2), ("I64", 3), ("U8", 4)):
        assert re.search(rf"#define SF_EPSTAT_{name} {val}\b", code) and getattr(lib, f"EPSTAT_{name}") == val
    assert "sf_episode_stats_add" in lib.SYMBOLS and callable(lib.episode_stats_add)
    # the ctypes mirror has the header's layout: 16 pointers, 16 int64 strides, 16 int32 codes
    assert ctypes.sizeof(lib.sf_epstat_channels) == 16 * 8 + 16 * 8 + 16 * 4
    assert [f[0] for f in lib.sf_epstat_channels._fields_] == ["ptr", "stride", "dtype"]
    L = lib.load()
    assert hasattr(L, "sf_episode_stats_add") and L.sf_abi_version() == 19
    src = open(os.path.join(ROOT, "sample_factory_amd", "csrc", "sf_rl.hip")).read()
    assert "sf_abi_version(void) { return 19; }" in src


def test_refusals_need_no_device():
    """every refusal happens before a launch, so the library answers them on a machine without a GPU as well"""
    import ctypes as C
    from sample_factory_amd import lib
    L = lib.load()
    ch = lib.sf_epstat_channels()
    ch.ptr[0], ch.stride[0], ch.dtype[0] = 4096, 1, lib.EPSTAT_F32
    p = C.c_void_p(4096)  # never dereferenced: every call below is refused, or has B == 0
    call = lambda ch_, K, term=p, trunc=p, B=4, acc=p: L.sf_episode_stats_add(  # noqa: E731
        C.byref(ch_) if ch_ is not None else None, K, term, trunc, None, C.c_int64(B), acc, None)
    assert call(ch, 1, B=0) == 0  # B == 0: SF_OK, nothing launched
    assert call(ch, 0) == -1 and call(ch, -3) == -1 and call(ch, 17) == -1
    assert b"K = 17" in L.sf_last_error()
    assert call(None, 1) == -1 and call(ch, 1, term=None) == -1 and call(ch, 1, trunc=None) == -1
    assert call(ch, 1, acc=None) == -1 and call(ch, 1, B=-1) == -1
    assert call(ch, 2) == -1  # channel 1 has a null pointer
    for field, bad in (("stride", 0), ("stride", -2), ("dtype", 5), ("dtype", -1)):
        c2 = lib.sf_epstat_channels()
        c2.ptr[0], c2.stride[0], c2.dtype[0] = 4096, 1, lib.EPSTAT_F32
        getattr(c2, field)[0] = bad
        assert call(c2, 1, B=0) == -1, (field, bad)  # refused even where B == 0 would launch nothing


# ------------------------------------------------------------------------------------------------ the host accumulator
def _agent(obj=None, **extra):
    d = {}
    if obj is not None:
        d["true_objective"] = obj
    if extra:
        d["episode_extra_stats"] = extra
    return d


# (infos of one step: one dict per agent, done flags) per step -> the dictionary the steps leave behind
TABLE = [
    ("done and not-done steps",
     [([_agent(3.0, kills=2), _agent(9.0, kills=7)], [True, False]),
      ([_agent(100.0, kills=50), _agent(5.0, kills=1)], [False, True])],
     {"true_objective": [8.0, 2], "kills": [3.0, 2]}),
    ("several agents at one step",
     [([_agent(1.5, kills=1), _agent(2.5, kills=2), _agent(4.0, kills=4)], [True, True, True])],
     {"true_objective": [8.0, 3], "kills": [7.0, 3]}),
    ("missing keys: counts are per key",
     [([_agent(2.0), _agent(None, dist=0.5), {}], [True, True, True]),
      ([_agent(4.0, dist=1.5), {}, None], [True, True, True])],
     {"true_objective": [6.0, 2], "dist": [2.0, 2]}),
    ("non-numeric values are ignored",
     [([{"true_objective": "high", "episode_extra_stats": {"name": "x", "ok": 1, "arr": np.arange(3), "none": None,
                                                           "lst": [1, 2], "flag": True, "np": np.float32(0.25),
                                                           "zero_d": np.array(2)}}], [True])],
     {"ok": [1.0, 1], "flag": [1.0, 1], "np": [0.25, 1], "zero_d": [2.0, 1]}),
    ("nested episode_extra_stats",
     [([{"episode_extra_stats": {"a": {"b": 1, "c": {"d": 2}}, "e": 3}}], [True])],
     {"a/b": [1.0, 1], "a/c/d": [2.0, 1], "e": [3.0, 1]}),
    ("true_objective absent",
     [([_agent(None, kills=1), _agent(None, kills=3)], [True, True])],
     {"kills": [4.0, 2]}),
    ("nobody done: nothing",
     [([_agent(1.0, kills=1)] * 2, [False, False])],
     {}),
    ("other keys of the info dict are not statistics",
     [([{"true_objective": 1.0, "is_active": False, "lives": 3, "episode_extra_stats": {"x": 2}}], [True])],
     {"true_objective": [1.0, 1], "x": [2.0, 1]}),
]


@pytest.mark.parametrize("name,steps,want", TABLE, ids=[t[0] for t in TABLE])
def test_host_accumulator_table(name, steps, want):
    acc = es.HostEpisodeStats()
    for infos, done in steps:
        acc.add_list_infos(infos, np.asarray(done))
    got = acc.pop()
    assert got == {k: [float(s), float(c)] for k, (s, c) in want.items()}
    assert acc.pop() == {} and not acc  # pop() clears


def test_host_accumulator_dict_infos_of_host_arrays():
    acc = es.HostEpisodeStats()
    infos = {"true_objective": np.array([1.0, 2.0, 4.0, 8.0]), "is_active": np.array([True] * 4),
             "episode_extra_stats": {"wins": np.array([1, 0, 1, 1], np.int64), "flag": np.array([True, True, False, True])},
             "junk": np.zeros((4, 3)), "text": np.array(["a", "b", "c", "d"]), "scalar": 3.0}
    acc.add_dict_infos(infos, np.array([True, False, False, True]))
    assert acc.pop() == {"true_objective": [9.0, 2.0], "wins": [2.0, 2.0], "flag": [2.0, 2.0]}
    acc.add_dict_infos(infos, np.array([False, True, True, False]), keys={"true_objective"})  # the fixed channel set
    assert acc.pop() == {"true_objective": [6.0, 2.0]}
    acc.add_dict_infos(infos, np.zeros(4, bool))
    assert acc.pop() == {}
    # a single-agent env's info dict, as the instance stepper hands it over
    acc.add_single(_agent(5.0, kills=2), False)
    acc.add_single(_agent(7.0, kills=3), True)
    assert acc.pop() == {"true_objective": [7.0, 1.0], "kills": [3.0, 1.0]}


# ------------------------------------------------------------------------------------------------ worker replies
def test_worker_reply_merge():
    a = es.HostEpisodeStats()
    a.add("kills", 3.0, 2)
    a.merge({"kills": [4.0, 1.0], "true_objective": [10.0, 4.0]})
    a.merge({})
    a.merge(None)
    a.merge({"true_objective": [0.5, 1.0]})
    assert a.sums == {"kills": [7.0, 3.0], "true_objective": [10.5, 5.0]}
    into = {"kills": [1.0, 1.0]}
    assert es.merge_sums(into, a.pop()) is into and into == {"kills": [8.0, 4.0], "true_objective": [10.5, 5.0]}


def _ledger(paths):
    tot = {}
    for p in paths:
        for line in open(p):
            for k, v in json.loads(line).items():
                s = tot.setdefault(k, [0.0, 0.0])
                s[0] += v
                s[1] += 1
    return tot


@pytest.mark.parametrize("inline", [True, False], ids=["inline", "processes"])
def test_env_instances_report_through_the_view(tmp_path, inline):
    """2 workers x 2 instances of the host env, dealt to 2 splits: what the views pop is what the instances' own ledgers
    hold, split by split; a reply travels only when something finished"""
    from sample_factory_amd.algo.sampling.parallel_env import ParallelHostEnvs
    from sample_factory_amd.envs.synthetic import make_episode_stats_host_env
    cfg = types.SimpleNamespace(synthetic_num_agents=3, synthetic_ledger_dir=str(tmp_path), seed=0,
                                env_worker_start_timeout=120.0, env_worker_step_timeout=120.0)
    envs = ParallelHostEnvs(cfg, "episode_stats_host", make_episode_stats_host_env, 2, 2, num_splits=2, inline=inline)
    try:
        views = envs.views
        assert views[0].num_agents == 6
        for v in views:
            v.reset()
        got = [{}, {}]
        rng = np.random.default_rng(0)
        for step in range(11):
            for s, v in enumerate(views):
                v.step(rng.integers(0, 4, v.num_agents).astype(np.int32))
                popped = v.pop_episode_stats()
                if step < 2:
                    assert popped == {}, "the shortest episode has 3 steps"
                es.merge_sums(got[s], popped)
    finally:
        envs.close()
    # instance env_id = worker * 2 + vector_index; vector_index 0 -> split 0, 1 -> split 1
    for s in (0, 1):
        want = _ledger([tmp_path / f"ledger_{w * 2 + s}.jsonl" for w in (0, 1)])
        assert set(got[s]) == {"true_objective", "first_action", "len_parity"}
        for k in got[s]:
            assert got[s][k][1] == want[k][1] > 0 and abs(got[s][k][0] - want[k][0]) <= 1e-9 * max(1.0, abs(want[k][0])), (s, k)


# ------------------------------------------------------------------------------------------------ key flattening
def test_flattened_keys_are_the_reference_names():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "episode_stats_flat_keys.json")))
    assert [k for k, _ in es.flatten_infos(g["infos"])] == g["keys"]
    assert any("/" in k for k in g["keys"]) and len(g["keys"]) >= 8
    # reported names: an entry x of episode_extra_stats is x, as the per-agent form reports it; the rest keeps its key
    assert es.stat_key("episode_extra_stats/first_action") == "first_action"
    assert es.stat_key("episode_extra_stats/nested/deep") == "nested/deep"
    assert es.stat_key("true_objective") == "true_objective" and es.stat_key("a/b/c") == "a/b/c"
    assert es.stat_key("episode_extra_stats") == "episode_extra_stats"


# ------------------------------------------------------------------------------------------------ the message
def test_episodic_message():
    assert es.episodic_message(0.0, 0.0, 0.0, {}) is None
    assert es.episodic_message(6.0, 30.0, 3.0, {}) == dict(reward=2.0, len=10.0, episodes=3.0)  # what it was before
    m = es.episodic_message(6.0, 30.0, 3.0, {"true_objective": [9.0, 3.0], "kills": [4.0, 2.0], "never": [0.0, 0.0]})
    assert m == dict(reward=2.0, len=10.0, episodes=3.0, true_objective=3.0, kills=2.0, episodes_kills=2.0)
    m = es.episodic_message(0.0, 0.0, 0.0, {"kills": [4.0, 2.0]})
    assert m == dict(kills=2.0, episodes_kills=2.0)


# ------------------------------------------------------------------------------------------------ best checkpoint
class _FakeLearner:
    def __init__(self, env_steps):
        self.env_steps, self.saved = env_steps, []

    def save_best(self, policy_id, metric, value):
        self.saved.append((policy_id, metric, value))
        return True


def _runner(metric, env_steps=1000, after=100):
    from sample_factory_amd.train import Runner
    cfg = types.SimpleNamespace(save_best_metric=metric, save_best_after=after, stats_avg=100, num_policies=1)
    r = Runner(cfg)
    r.rank, r.learner = 0, _FakeLearner(env_steps)
    return r


def _report(r, **stats):
    from sample_factory_amd.algo.utils.misc import EPISODIC, POLICY_ID_KEY
    r._process_msg({EPISODIC: dict(stats), POLICY_ID_KEY: 0})


def test_save_best_policy_picks_up_a_reported_key(caplog):
    r = _runner("first_action")
    _report(r, reward=1.0, len=5.0, episodes=2.0, first_action=3.0, true_objective=7.0)
    _report(r, reward=3.0, len=5.0, episodes=2.0, first_action=1.0, true_objective=9.0)
    assert list(r.policy_avg_stats["first_action"][0]) == [3.0, 1.0]
    r._save_best_policy()
    assert r.learner.saved == [(0, "first_action", 2.0)]
    r2 = _runner("true_objective")
    _report(r2, reward=1.0, len=5.0, episodes=2.0, true_objective=7.0)
    r2._save_best_policy()
    assert r2.learner.saved == [(0, "true_objective", 7.0)]
    early = _runner("first_action", env_steps=50)
    _report(early, reward=1.0, first_action=3.0)
    early._save_best_policy()
    assert early.learner.saved == []  # save_best_after still rules


def test_true_objective_falls_back_to_reward_with_one_line(caplog):
    r = _runner("true_objective")
    with caplog.at_level(logging.INFO):
        r._save_best_policy()  # nothing finished yet: nothing to save, nothing to say
        assert r.learner.saved == []
        _report(r, reward=2.0, len=5.0, episodes=1.0)
        _report(r, reward=4.0, len=5.0, episodes=1.0)
        r._save_best_policy()
        r._save_best_policy()
    assert r.learner.saved == [(0, "true_objective", 3.0)] * 2  # the reward's value, under the metric's name
    assert "fallback" in r._best_metric_notes and len(r._best_metric_notes) == 1
    # once an env does report it, its own values rule
    _report(r, reward=4.0, len=5.0, episodes=1.0, true_objective=11.0)
    r._save_best_policy()
    assert r.learner.saved[-1] == (0, "true_objective", 11.0)


def test_a_metric_nobody_reports_warns_once():
    r = _runner("kills")
    notes = []
    from sample_factory_amd import train
    real = train.log.warning
    train.log.warning = lambda msg, *a, **k: notes.append(str(msg))
    try:
        r._save_best_policy()          # no episode has finished at all: still silent
        assert notes == []
        _report(r, reward=2.0, len=5.0, episodes=1.0)
        for _ in range(3):
            r._save_best_policy()
    finally:
        train.log.warning = real
    assert r.learner.saved == [] and len(notes) == 1 and "kills" in notes[0]
    quiet = _runner("kills", env_steps=50)
    _report(quiet, reward=2.0)
    quiet._save_best_policy()          # before save_best_after: not yet
    assert "missing" not in quiet._best_metric_notes


def test_summaries_carry_the_reference_names(tmp_path):
    from sample_factory_amd.train import Runner
    cfg = types.SimpleNamespace(save_best_metric="reward", save_best_after=0, stats_avg=100, num_policies=1,
                                train_dir=str(tmp_path), experiment="x")
    r = Runner(cfg)
    r.rank = 0
    r.learner = types.SimpleNamespace(env_steps=10, train_step=1, last_summary={})
    _report(r, reward=1.0, len=5.0, episodes=2.0, first_action=3.0, true_objective=7.0)
    r._write_summaries(123.0)
    rec = json.loads(open(tmp_path / "x" / ".summary" / "0" / "summaries.jsonl").read().splitlines()[-1])
    assert rec["policy_stats/avg_true_objective"] == 7.0 and rec["policy_stats/avg_first_action"] == 3.0
    assert rec["policy_stats/avg_reward"] == 1.0
    assert isinstance(r.policy_avg_stats["first_action"][0], deque)
