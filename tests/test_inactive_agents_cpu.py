"""--track_inactive_agents as far as it can be checked without a GPU: the two entry points' place in the
C ABI and every host refusal of theirs (all before any launch), the engine flag and its way through config.json, the
zero-copy refusal, the env workers' shared "active" array and the turn-based test env."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITE, STORE = "sf_traj_write_env_step_active", "sf_rnn_store_state_held"


def test_entry_points_are_declared_listed_and_exported_and_the_abi_version_stays():
    from sample_factory_amd import lib
    L = lib.load()
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    for e in (WRITE, STORE):
        assert e in lib.SYMBOLS and re.search(r"\bint\s+" + e + r"\s*\(", text) and hasattr(L, e)
    assert callable(lib.traj_write_env_step_active) and callable(lib.rnn_store_state_held)
    assert L.sf_abi_version() == 19


def _p(a):
    return None if a is None else C.c_void_p(a)


def _write(L, rewards=64, terminated=128, truncated=192, B=8, T=5, t=0, traj_rewards=1024, traj_dones=2048,
           traj_time_outs=3072, traj_policy_id=4096, ep_return=None, ep_len=None, ep_stats=None, active_in=8192,
           active_state=8448):
    return getattr(L, WRITE)(_p(rewards), _p(terminated), _p(truncated), B, T, t, C.c_float(1.0), C.c_float(10.0), 0,
                             _p(traj_rewards), _p(traj_dones), _p(traj_time_outs), _p(traj_policy_id), _p(ep_return),
                             _p(ep_len), _p(ep_stats), _p(active_in), _p(active_state), None)


def test_the_write_kernel_refuses_on_the_host():
    """made-up non-null addresses: each call must return -1 (SF_ERR_ARG) on a machine with no GPU"""
    from sample_factory_amd import lib
    L = lib.load()
    bad = [
        dict(active_in=None), dict(active_state=None),                    # the two new arguments
        dict(active_in=8448), dict(active_in=8448 + 7), dict(active_in=8448 - 7),   # B = 8 bytes each: they share a byte
        dict(rewards=None), dict(terminated=None), dict(traj_rewards=None), dict(traj_dones=None),
        dict(traj_time_outs=None), dict(traj_policy_id=None),             # what sf_traj_write_env_step refuses
        dict(B=0), dict(T=0), dict(t=-1), dict(t=5),
        dict(ep_return=512), dict(ep_len=512),                            # one without the other
    ]
    for kw in bad:
        assert _write(L, **kw) == -1, kw
        assert WRITE in L.sf_last_error().decode(), (kw, L.sf_last_error())
    for kw in (dict(active_in=8448 + 8), dict(active_in=8448 - 8), dict(truncated=None)):  # neighbours / optional: accepted
        assert _write(L, **kw) != -1, kw


def _store(L, h=64, c=None, dones=128, done_stride=5, prev=1 << 20, prev_stride=6 * 64, policy_id=256, pid_stride=5,
           out=(1 << 20) + 4 * 64, out_stride=6 * 64, B=8, H=32):
    i64 = C.c_int64
    return getattr(L, STORE)(_p(h), _p(c), _p(dones), i64(done_stride), _p(prev), i64(prev_stride), _p(policy_id),
                             i64(pid_stride), _p(out), i64(out_stride), i64(B), H, None)


def test_the_state_store_refuses_on_the_host():
    """defaults: columns t and t + 1 of a [8, 6, 64] f32 slab, the first of two stacked 32-wide layers"""
    from sample_factory_amd import lib
    L = lib.load()
    base = 1 << 20
    bad = [
        dict(h=None), dict(dones=None), dict(out=None), dict(B=0), dict(H=0),     # what sf_rnn_store_state refuses
        dict(prev=None), dict(policy_id=None),
        dict(prev_stride=31), dict(out_stride=31), dict(c=512, out_stride=63),    # rows narrower than [h] / [h | c]
        dict(out=base), dict(out=base + 4 * 31), dict(out=base - 4 * 31),         # the same rows / one float shared
        dict(out=base + 4 * (6 * 64 + 10)),                                       # next row of the same column, shifted
        dict(out=base + 4 * (7 * 6 * 64 + 31)),                                   # last row of prev only
        dict(c=512, out=base + 4 * 32),                                           # LSTM rows are 64 wide: layer 1 meets layer 0
        dict(out=base + 4 * 100, out_stride=6 * 64 + 4),                          # other stride inside prev's extent
        dict(out=base + 2),                                                       # not a float address
    ]
    for kw in bad:
        assert _store(L, **kw) == -1, kw
        assert STORE in L.sf_last_error().decode(), (kw, L.sf_last_error())
    ok = [dict(), dict(out=base + 4 * 32), dict(out=base - 4 * 32), dict(c=512), dict(out=base - 4 * 64, c=512),
          dict(out=base + 4 * 8 * 6 * 64, out_stride=40)]                          # behind prev's extent, another stride
    for kw in ok:
        assert _store(L, **kw) != -1, (kw, L.sf_last_error())


def test_flag_defaults_to_off_and_parses():
    from sample_factory_amd.cfg.arguments import ENGINE_FLAGS, FLAGS, default_cfg, parse_full_cfg, parse_sf_args
    assert ("track_inactive_agents", False) in [(f[0], f[2]) for f in ENGINE_FLAGS]
    assert "track_inactive_agents" not in [f[0] for f in FLAGS]
    assert default_cfg(env="x").track_inactive_agents is False
    parser, _ = parse_sf_args(["--env=x", "--track_inactive_agents=True"])
    assert parse_full_cfg(parser, ["--env=x", "--track_inactive_agents=True"]).track_inactive_agents is True
    assert parse_full_cfg(parser, ["--env=x"]).track_inactive_agents is False


def test_flag_round_trips_through_config_json(tmp_path):
    from sample_factory_amd.cfg.arguments import cfg_dict, load_from_checkpoint, parse_full_cfg, parse_sf_args
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=ia", "--track_inactive_agents=True"]
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    os.makedirs(tmp_path / "ia")
    with open(tmp_path / "ia" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    assert json.load(open(tmp_path / "ia" / "config.json"))["track_inactive_agents"] is True
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=ia"]  # enjoy: the flag is not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).track_inactive_agents is True
    argv.append("--track_inactive_agents=False")  # ... and the command line still overrides the file
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).track_inactive_agents is False


def test_zero_copy_envs_are_refused_at_set_up():
    from sample_factory_amd.algo.sampling.batched_sampling import tracks_inactive_agents
    from sample_factory_amd.cfg.arguments import default_cfg
    on, off = default_cfg(env="x", track_inactive_agents=True), default_cfg(env="x")
    zero_copy, host = types.SimpleNamespace(step_into=lambda *a: None), types.SimpleNamespace()
    with pytest.raises(NotImplementedError, match="step_into"):
        tracks_inactive_agents(on, zero_copy)
    assert tracks_inactive_agents(off, zero_copy) is False and tracks_inactive_agents(off, host) is False
    assert tracks_inactive_agents(on, host) is True
    assert tracks_inactive_agents(on, zero_copy, multi_key=True) is True  # stepped through step(): it has infos


def test_infos_are_read_in_every_form():
    from sample_factory_amd.algo.sampling.parallel_env import infos_is_active
    assert infos_is_active({}, 3) is None and infos_is_active(None, 3) is None and infos_is_active([{}, {}, {}], 3) is None
    got = infos_is_active([{"is_active": False}, {}, {"is_active": True, "x": 1}], 3)
    assert got.dtype == np.bool_ and got.tolist() == [False, True, True]
    assert infos_is_active(({"is_active": 0}, {"is_active": 1}), 2).tolist() == [False, True]
    assert infos_is_active({"is_active": np.array([1, 0, 1], np.uint8)}, 3).tolist() == [True, False, True]
    assert infos_is_active({"is_active": False}, 1).tolist() == [False]  # a single-agent env's own info dict
    with pytest.raises(ValueError):
        infos_is_active({"is_active": np.ones(4, bool)}, 3)


class _TwoAgentEnv:
    """batched host env of two agents: agent 0 reports is_active = (step is even), agent 1 never reports"""
    num_agents, is_multiagent = 2, True

    def __init__(self):
        from sample_factory_amd.envs import spaces
        self.observation_space = spaces.Dict({"obs": spaces.Box(-1, 1, (3,), np.float32)})
        self.action_space = spaces.Discrete(2)
        self.k = 0

    def reset(self, **kw):
        self.k = 0
        return {"obs": np.zeros((2, 3), np.float32)}, [{}, {}]

    def step(self, actions):
        self.k += 1
        z = np.zeros(2, bool)
        return {"obs": np.full((2, 3), self.k, np.float32)}, np.ones(2, np.float32), z, z, [{"is_active": self.k % 2 == 0}, {}]

    def close(self):
        pass


class _OneAgentEnv(_TwoAgentEnv):
    """single-agent gym-style env: one info dict per step"""
    num_agents, is_multiagent = 1, False

    def reset(self, **kw):
        return np.zeros(3, np.float32), {}

    def step(self, action):
        self.k += 1
        return np.zeros(3, np.float32), 1.0, False, False, ({"is_active": False} if self.k == 2 else {})


def _make(name, cfg, env_config, render_mode=None):
    return _OneAgentEnv() if name == "one" else _TwoAgentEnv()


def test_the_worker_stepper_fills_the_shared_active_array():
    from sample_factory_amd.algo.sampling.parallel_env import CMD_RESET, CMD_STEP, _InstanceStepper
    arrays = {0: {"obs.obs": np.zeros((3, 3), np.float32), "rew": np.zeros(3, np.float32), "term": np.zeros(3, bool),
                  "trunc": np.zeros(3, bool), "act": np.zeros(3, np.int32), "active": np.zeros(3, bool)}}
    two = _InstanceStepper(_make, "two", None, 0, [(0, 0, 0, 0, 2)], arrays, [2], False)   # rows 0, 1
    one = _InstanceStepper(_make, "one", None, 0, [(0, 1, 1, 2, 1)], arrays, [2], False)   # row 2
    for st in (two, one):
        st.run(CMD_RESET, 0)
    seen = []
    for _ in range(3):
        arrays[0]["active"][:] = False  # whatever was there: every step writes every row
        for st in (two, one):
            st.run(CMD_STEP, 0)
        seen.append(arrays[0]["active"].tolist())
    assert seen == [[False, True, True], [True, True, False], [False, True, True]]  # a missing key means active
    assert arrays[0]["rew"].tolist() == [1.0, 1.0, 1.0]
    # arrays without the slot (the flag is off): the stepper leaves the infos alone
    plain = {0: {k: v.copy() for k, v in arrays[0].items() if k != "active"}}
    st = _InstanceStepper(_make, "two", None, 0, [(0, 0, 0, 0, 2)], plain, [2], False)
    st.run(CMD_RESET, 0)
    st.run(CMD_STEP, 0)
    assert "active" not in plain[0]


def test_the_view_hands_the_flags_back_in_the_infos_slot():
    from sample_factory_amd.algo.sampling.parallel_env import ParallelHostEnvs
    from sample_factory_amd.cfg.arguments import default_cfg
    for on in (True, False):
        envs = ParallelHostEnvs(default_cfg(env="two", track_inactive_agents=on), "two", _make, 2, 1, inline=True)
        v = envs.views[0]
        v.reset()
        infos = [v.step(np.zeros(4, np.int32))[4] for _ in range(2)]
        if on:
            assert infos[1]["is_active"] is envs.arrays[0]["active"] and infos[1]["is_active"].tolist() == [True] * 4
            v.step(np.zeros(4, np.int32))
            assert envs.arrays[0]["active"].tolist() == [False, True, False, True]
        else:
            assert infos == [{}, {}] and "active" not in envs.arrays[0]
        envs.close()


def test_the_turn_based_env_emits_the_pattern_it_promises():
    from sample_factory_amd.envs.synthetic import TurnBasedMaskedBanditEnv, make_turn_based_masked_bandit_env
    env = TurnBasedMaskedBanditEnv(num_games=3, num_actions=4, episode_len=5, seed=3)
    assert env.num_agents == 6 and env.observation_space["action_mask"].shape == (4,)
    o, infos = env.reset()
    assert o["obs"].shape == (6, 4) and o["action_mask"].dtype == np.uint8 and len(infos) == 6
    for k in range(12):
        target = env.target.copy()
        assert (o["action_mask"][np.arange(6), target] == 1).all() and (o["obs"].argmax(1) == target).all()
        o, rew, term, trunc, infos = env.step(target)  # everybody plays the rewarded action ...
        movers = np.array([(a % 2) == ((k + a // 2) % 2) for a in range(6)])
        assert rew.tolist() == movers.astype(np.float32).tolist()  # ... the mover alone is paid
        assert movers.reshape(3, 2).sum(1).tolist() == [1, 1, 1]
        # the waiting agent's info says so; the agent to move next leaves the key out
        assert [i.get("is_active", True) for i in infos] == (~movers).tolist()
        assert all(("is_active" in i) == (not f) for i, f in zip(infos, (~movers).tolist()))
        assert term.tolist() == [(k + 1) % 5 == 0] * 6 and not trunc.any()
    # scripted: the infos of step k carry script[k % period], as per-agent dicts or as one array
    script = [[True, False, True, True, False, True], [False, False, True, True, True, True], [True] * 6]
    cfg = types.SimpleNamespace(synthetic_num_games=3, synthetic_active_script=script, seed=0)
    for dict_infos in (False, True):
        cfg.synthetic_dict_infos = dict_infos
        env = make_turn_based_masked_bandit_env("turn_based_masked_bandit", cfg, types.SimpleNamespace(env_id=2))
        env.reset()
        for k in range(7):
            infos = env.step(np.zeros(6, np.int32))[4]
            got = infos["is_active"].tolist() if dict_infos else [i.get("is_active", True) for i in infos]
            assert got == script[k % 3], (k, dict_infos)
            assert env.active_after(k).tolist() == script[k % 3]
