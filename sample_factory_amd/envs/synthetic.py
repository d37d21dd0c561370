"""Synthetic device-resident vector env (SURVEY.md §8d "C2 synthetic inputs"): N agents, u8 [C,H,W] frames from a
counter-based Philox4x32-10 stream, reward 1 when action == (step + env_id) % num_actions, Bernoulli(1/1024)
termination.  To Sample Factory it looks like the reference's GPU envs (brax / isaacgym: `num_agents=N`, tensors on
the device, auto-reset; sf_examples/brax/train_brax.py:160-204).  Additionally it implements the zero-copy hook
`step_into(actions, obs_out)`: the frame generator writes straight into slot t+1 of the trajectory slab (K1).
"""
from __future__ import annotations

import numpy as np
import torch

from sample_factory_amd import lib
from sample_factory_amd.envs import spaces


class SyntheticVecEnv:
    def __init__(self, num_agents=4096, obs_shape=(4, 84, 84), num_actions=6, seed=0, env0=0, device="cuda"):
        self.num_agents = int(num_agents)
        self.obs_shape = tuple(obs_shape)
        self.obs_bytes = int(np.prod(obs_shape))
        assert self.obs_bytes % 16 == 0, "frame size must be a multiple of 16 bytes"
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 255, self.obs_shape, np.uint8)})
        self.action_space = spaces.Discrete(num_actions)
        self.num_actions = num_actions
        self.seed_, self.env0 = int(seed), int(env0)
        self.device = torch.device(device)
        self.step_count = 0
        self._rew = torch.zeros(self.num_agents, dtype=torch.float32, device=self.device)
        self._term = torch.zeros(self.num_agents, dtype=torch.bool, device=self.device)
        self._trunc = torch.zeros(self.num_agents, dtype=torch.bool, device=self.device)
        self._obs = None

    # -- zero-copy interface used by the native rollout runner
    def write_obs(self, obs_out: torch.Tensor) -> None:
        """obs_out: [N, C, H, W] u8 view (possibly strided over dim 0, e.g. slab[:, t])."""
        assert obs_out.dtype == torch.uint8 and obs_out.is_cuda and obs_out.shape[0] == self.num_agents
        assert obs_out[0].is_contiguous()
        lib.synth_obs(obs_out.data_ptr(), obs_out.stride(0), self.num_agents, self.env0, self.obs_bytes, self.seed_,
                      self.step_count)

    def reset_into(self, obs_out: torch.Tensor) -> None:
        self.step_count = 0
        self.write_obs(obs_out)

    def step_into(self, actions: torch.Tensor, obs_out: torch.Tensor):
        """actions int32 [N] on device. Returns (rewards f32, terminated bool, truncated bool) device tensors."""
        lib.synth_step(actions, self.env0, self.num_actions, self.seed_, self.step_count, self._rew, self._term)
        self.step_count += 1
        self.write_obs(obs_out)
        return self._rew, self._term, self._trunc

    # -- gymnasium-style interface (what a stock Sample Factory runner would call; make_env.py:147-237)
    def reset(self, **kwargs):
        if self._obs is None:
            self._obs = torch.empty((self.num_agents,) + self.obs_shape, dtype=torch.uint8, device=self.device)
        self.reset_into(self._obs)
        return {"obs": self._obs}, {}

    def step(self, actions):
        if self._obs is None:
            self.reset()
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).reshape(-1).contiguous()
        rew, term, trunc = self.step_into(a, self._obs)
        return {"obs": self._obs}, rew, term, trunc, {}

    def close(self):
        pass


class SyntheticContinuousEnv:
    """Ant-shaped device-resident env (SURVEY.md §8d C5 stand-in): f32 vector observations, Box actions.  One HIP
    launch per step (sf_synth_vec_step, counter-based Philox noise keyed by the global env id): obs' = 0.9*obs +
    0.1*noise, reward = -mean(action^2) + 0.1*obs[:,0], termination ~ Bernoulli(1/256) with auto-reset.  Like the image
    env it offers the zero-copy hooks reset_into / step_into (the next observation lands in slot t+1 of the slab) next to
    the gymnasium-style reset / step."""

    def __init__(self, num_agents=2048, obs_dim=27, act_dim=8, seed=0, env0=0, device="cuda"):
        self.num_agents, self.obs_dim, self.act_dim = int(num_agents), int(obs_dim), int(act_dim)
        self.observation_space = spaces.Dict({"obs": spaces.Box(-np.inf, np.inf, (obs_dim,), np.float32)})
        self.action_space = spaces.Box(-1.0, 1.0, (act_dim,), np.float32)
        self.device = torch.device(device)
        self.seed_, self.env0, self.step_count = int(seed), int(env0), 0
        self.state = torch.zeros((self.num_agents, obs_dim), dtype=torch.float32, device=self.device)
        self._obs = torch.zeros_like(self.state)
        self._rew = torch.zeros(self.num_agents, dtype=torch.float32, device=self.device)
        self._term = torch.zeros(self.num_agents, dtype=torch.bool, device=self.device)
        self._trunc = torch.zeros(self.num_agents, dtype=torch.bool, device=self.device)

    def reset_into(self, obs_out: torch.Tensor) -> None:
        self.step_count = 0
        lib.synth_vec_step(self.state, None, obs_out, self.env0, self.seed_, 0xFFFFFFFF, True, self._rew, self._term)

    def step_into(self, actions: torch.Tensor, obs_out: torch.Tensor):
        """actions f32 [N, act_dim] device view (e.g. traj.actions[:, t]); returns (rewards, terminated, truncated)"""
        lib.synth_vec_step(self.state, actions, obs_out, self.env0, self.seed_, self.step_count, False, self._rew, self._term)
        self.step_count += 1
        return self._rew, self._term, self._trunc

    def reset(self, **kwargs):
        self.reset_into(self._obs)
        return {"obs": self._obs}, {}

    def step(self, actions):
        a = torch.as_tensor(actions, device=self.device, dtype=torch.float32).reshape(self.num_agents, self.act_dim).contiguous()
        rew, term, trunc = self.step_into(a, self._obs)
        return {"obs": self._obs}, rew, term, trunc, {}

    def close(self):
        pass


class HostFrameVecEnv:
    """Atari-shaped HOST vector env (BASELINE configs[2] stand-in: envpool is not installed on the boxes): N agents,
    u8 [4,84,84] frames living in ordinary host memory, returned as numpy arrays exactly as envpool hands over its own
    buffers (batched_sampling.py:62-82) — so every step costs the real ingest path: host array -> pinned staging ->
    pitched H2D DMA into the slab, and a D2H of the int32 actions.  Frames come from a small pre-generated ring (the
    simulator's own cost is not what is being measured); rewards follow the synthetic env's rule."""

    def __init__(self, num_agents=1024, obs_shape=(4, 84, 84), num_actions=6, seed=0, ring=4, sim_ms=0.0, hwc=False):
        self.num_agents, self.obs_shape, self.num_actions = int(num_agents), tuple(obs_shape), int(num_actions)
        self.action_space = spaces.Discrete(num_actions)
        rng = np.random.default_rng(seed)
        self.ring = rng.integers(0, 256, size=(ring, self.num_agents) + self.obs_shape, dtype=np.uint8)
        self.hwc = bool(hwc)
        if self.hwc:  # the same ring served channel-last, as most pixel envs do (--hwc_observations): frame for frame the
            # same pixels as [ring, N, H, W, C], transposed once, here; obs_shape stays the (C, H, W) it was asked for
            self.ring = np.ascontiguousarray(self.ring.transpose(0, 1, 3, 4, 2))
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 255, self.ring.shape[2:], np.uint8)})
        self.step_count = 0
        self.sim_ms = float(sim_ms)  # optional simulated emulator time per step (host sleep)
        self._ids = np.arange(self.num_agents)
        self._rng = rng

    def reset(self, **kwargs):
        self.step_count = 0
        return {"obs": self.ring[0]}, {}

    def step(self, actions):
        a = np.asarray(actions).reshape(-1)
        rew = (a == (self.step_count + self._ids) % self.num_actions).astype(np.float32)
        term = self._rng.random(self.num_agents) < (1.0 / 1024.0)
        self.step_count += 1
        if self.sim_ms > 0:
            import time
            time.sleep(self.sim_ms * 1e-3)
        return {"obs": self.ring[self.step_count % len(self.ring)]}, rew, term, np.zeros(self.num_agents, bool), {}

    def close(self):
        pass


def make_host_frame_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = getattr(cfg, "synthetic_num_agents", 1024) if cfg is not None else 1024
    seed = ((getattr(cfg, "seed", None) or 0) if cfg is not None else 0) + int(getattr(env_config, "env_id", 0) or 0)
    # cfg.host_env_obs_shape: e.g. (1, 84, 84) — single frames, stacked on the device with --device_framestack
    shape = tuple(getattr(cfg, "host_env_obs_shape", None) or (4, 84, 84)) if cfg is not None else (4, 84, 84)
    # cfg.host_env_hwc: the frames leave the env as [H, W, C] (obs_shape stays C, H, W): the --hwc_observations test env
    return HostFrameVecEnv(num_agents=n, obs_shape=shape, seed=seed,
                           sim_ms=getattr(cfg, "host_env_sim_ms", 0.0) if cfg is not None else 0.0,
                           hwc=bool(getattr(cfg, "host_env_hwc", False)) if cfg is not None else False)


class SyntheticTupleEnv(SyntheticVecEnv):
    """Multi-head variant (Tuple(Discrete(n0), Discrete(n1), ...), the VizDoom-style action space of
    action_distributions.py:197-287): same frames; the reward rule looks at head 0, the other heads are free.
    A negative entry -D of `head_sizes` is a Box(-1, 1, (D,)) member (a mixed Tuple: the env then receives the list of
    per-member arrays `preprocess_actions` builds, batched_sampling.py:51-59)."""

    def __init__(self, head_sizes=(6, 3), **kw):
        assert int(head_sizes[0]) > 0, "member 0 carries the reward rule: Discrete"
        super().__init__(num_actions=int(head_sizes[0]), **kw)
        self.action_space = spaces.Tuple([spaces.Discrete(int(n)) if int(n) > 0 else
                                          spaces.Box(-1.0, 1.0, (-int(n),), np.float32) for n in head_sizes])
        self.last_actions = None  # what the sampler handed over at the last step (tests look at the format)

    def _head0(self, actions):
        self.last_actions = actions
        if isinstance(actions, (list, tuple)):  # mixed Tuple: one array per member
            return torch.as_tensor(actions[0], device=self.device).to(torch.int32).reshape(self.num_agents).contiguous()
        return torch.as_tensor(actions, device=self.device).to(torch.int32).reshape(self.num_agents, -1)[:, 0].contiguous()

    def step_into(self, actions, obs_out: torch.Tensor):
        return super().step_into(self._head0(actions), obs_out)

    def step(self, actions):
        return super().step(self._head0(actions))


class MaskedBanditEnv:
    """GPU vector env with an action mask in the observation dict (obs["action_mask"], u8 [N, A]): a contextual bandit
    whose rewarded action (obs one-hot) is always allowed while a random subset of the others is masked out."""

    def __init__(self, num_agents=64, num_actions=6, seed=0, device="cuda"):
        self.num_agents, self.A = int(num_agents), int(num_actions)
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 1, (self.A,), np.float32),
                                              "action_mask": spaces.Box(0, 1, (self.A,), np.uint8)})
        self.action_space = spaces.Discrete(self.A)
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        self._draw()

    def _draw(self):
        self.target = torch.randint(0, self.A, (self.num_agents,), generator=self.gen, device=self.device)
        self.mask = (torch.rand((self.num_agents, self.A), generator=self.gen, device=self.device) < 0.5)
        self.mask[torch.arange(self.num_agents, device=self.device), self.target] = True
        self.obs = torch.nn.functional.one_hot(self.target, self.A).float()

    def _out(self):
        return {"obs": self.obs, "action_mask": self.mask.to(torch.uint8)}

    def reset(self, **kwargs):
        self._draw()
        return self._out(), {}

    def step(self, actions):
        a = torch.as_tensor(actions, device=self.device).reshape(-1).long()
        self.last_allowed = self.mask[torch.arange(self.num_agents, device=self.device), a].clone()
        rew = (a == self.target).float()
        term = torch.ones(self.num_agents, dtype=torch.bool, device=self.device)  # one-step episodes, auto-reset
        self._draw()
        return self._out(), rew, term, torch.zeros_like(term), {}

    def close(self):
        pass


class DictObsBanditEnv:
    """GPU vector env whose observation is a dict of SEVERAL keys (the reference's MultiInputEncoder case,
    model/encoder.py:33-69): "obs" = a random u8 image (pure distraction), "measurements" = one-hot of the rewarded
    action.  The policy can only learn the bandit through the vector key."""

    def __init__(self, num_agents=64, num_actions=4, image_shape=(4, 36, 36), seed=0, device="cuda"):
        self.num_agents, self.A, self.image_shape = int(num_agents), int(num_actions), tuple(image_shape)
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 255, self.image_shape, np.uint8),
                                              "measurements": spaces.Box(0, 1, (self.A,), np.float32)})
        self.action_space = spaces.Discrete(self.A)
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        self._draw()

    def _draw(self):
        self.target = torch.randint(0, self.A, (self.num_agents,), generator=self.gen, device=self.device)
        self.img = torch.randint(0, 256, (self.num_agents,) + self.image_shape, generator=self.gen, device=self.device,
                                 dtype=torch.int32).to(torch.uint8)

    def _out(self):
        return {"obs": self.img, "measurements": torch.nn.functional.one_hot(self.target, self.A).float()}

    def reset(self, **kwargs):
        self._draw()
        return self._out(), {}

    def step(self, actions):
        a = torch.as_tensor(actions, device=self.device).reshape(-1).long()
        rew = (a == self.target).float()
        term = torch.ones(self.num_agents, dtype=torch.bool, device=self.device)  # one-step episodes, auto-reset
        self._draw()
        return self._out(), rew, term, torch.zeros_like(term), {}

    def close(self):
        pass


def make_dict_obs_bandit_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = getattr(cfg, "synthetic_num_agents", 64) if cfg is not None else 64
    return DictObsBanditEnv(num_agents=n, seed=(getattr(cfg, "seed", None) or 0) if cfg is not None else 0)


def make_masked_bandit_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = getattr(cfg, "synthetic_num_agents", 64) if cfg is not None else 64
    a = int(getattr(cfg, "synthetic_num_actions", 6) or 6) if cfg is not None else 6
    return MaskedBanditEnv(num_agents=n, num_actions=a, seed=(getattr(cfg, "seed", None) or 0) if cfg is not None else 0)


class TurnBasedMaskedBanditEnv:
    """HOST vector env of `num_games` two-agent turn-based games (row 2 * g + a = agent a of game g): the masked bandit,
    played in turns.  The agents of a game alternate; with every step the env reports, per agent, whether the observation
    it just handed out is that agent's to act on: info["is_active"] = False for the one that now waits (what the
    reference's PettingZoo adapter reports for every agent but the one to move).  The action of a waiting agent is
    ignored and the reward is paid to the mover only; observations carry an "action_mask" that always allows the rewarded
    action.  Episodes last `episode_len` steps, then every row reports `terminated` and the game goes on (auto-reset;
    whose turn it is does not depend on episode boundaries).

    Step k (0-based, counted from reset) is moved by agent (k + g) % 2 of game g, so the infos returned WITH step k name
    agent (k + 1 + g) % 2 as active.  `script` (bool [period, 2 * num_games]) replaces that pattern: the infos of step k
    carry script[k % period].  `dict_infos`: the flags come as one {"is_active": bool array} dict instead of a list of
    per-agent dicts, and agents whose flag is True leave the key out of their dict in the list form (missing = active)."""

    def __init__(self, num_games=3, num_actions=4, episode_len=5, seed=0, script=None, dict_infos=False):
        self.num_games, self.A, self.episode_len = int(num_games), int(num_actions), int(episode_len)
        self.num_agents = 2 * self.num_games
        self.is_multiagent = True
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 1, (self.A,), np.float32),
                                              "action_mask": spaces.Box(0, 1, (self.A,), np.uint8)})
        self.action_space = spaces.Discrete(self.A)
        self.script = None if script is None else np.asarray(script, dtype=np.bool_).reshape(-1, self.num_agents)
        self.dict_infos = bool(dict_infos)
        self._seed = int(seed)
        self._rows = np.arange(self.num_agents)
        self.reset()

    def _draw(self):
        self.target = self._rng.integers(0, self.A, self.num_agents)
        self.mask = self._rng.random((self.num_agents, self.A)) < 0.5
        self.mask[self._rows, self.target] = True

    def _out(self):
        obs = np.zeros((self.num_agents, self.A), np.float32)
        obs[self._rows, self.target] = 1.0
        return {"obs": obs, "action_mask": self.mask.astype(np.uint8)}

    def movers(self, k: int) -> np.ndarray:
        """bool [agents]: who moves at step k"""
        return (self._rows % 2) == ((k + self._rows // 2) % 2)

    def active_after(self, k: int) -> np.ndarray:
        """bool [agents]: the is_active flags the infos of step k carry"""
        return self.script[k % len(self.script)] if self.script is not None else self.movers(k + 1)

    def reset(self, **kwargs):
        self._rng = np.random.default_rng(self._seed)
        self.k = self.ep_step = 0
        self._draw()
        return self._out(), [{} for _ in range(self.num_agents)]

    def step(self, actions):
        a = np.asarray(actions).reshape(-1)
        rew = ((a == self.target) & self.movers(self.k)).astype(np.float32)
        active = self.active_after(self.k)
        self.k += 1
        self.ep_step += 1
        term = np.full(self.num_agents, self.ep_step >= self.episode_len)
        if term[0]:
            self.ep_step = 0
        self._draw()
        infos = {"is_active": active.copy()} if self.dict_infos else \
            [{} if f else {"is_active": False} for f in active.tolist()]
        return self._out(), rew, term, np.zeros(self.num_agents, np.bool_), infos

    def close(self):
        pass


def make_turn_based_masked_bandit_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    """cfg.synthetic_num_games / synthetic_num_actions / synthetic_episode_len size the env; cfg.synthetic_active_script
    (bool [period, agents], nested lists) makes it the scripted variant"""
    g = lambda name, d: (getattr(cfg, name, None) or d) if cfg is not None else d  # noqa: E731
    seed = g("seed", 0) + int(getattr(env_config, "env_id", 0) or 0)
    return TurnBasedMaskedBanditEnv(num_games=int(g("synthetic_num_games", 3)), num_actions=int(g("synthetic_num_actions", 4)),
                                    episode_len=int(g("synthetic_episode_len", 5)), seed=seed,
                                    script=g("synthetic_active_script", None), dict_infos=bool(g("synthetic_dict_infos", False)))


def episode_stats_lengths(ids: np.ndarray) -> np.ndarray:
    """the episode length of the agents with global ids `ids` in the two episode-statistics envs below: 3 .. 7 steps"""
    return 3 + (np.asarray(ids) % 5)


class EpisodeStatsVecEnv:
    """GPU vector env that reports statistics of its own the way the reference's vectorised envs do: its
    step() returns ONE infos dict of device tensors,

        {"true_objective": 2 * return + 1 (f32), "episode_extra_stats": {"first_action": the episode's first action (i32),
         "len_parity": steps so far % 2 (i64)}, "junk": an [N, 3] tensor that is no statistic}

    with one element per agent at EVERY step; only the elements of the agents whose episode ends count.  Episodes have
    deterministic lengths (episode_stats_lengths of the global agent id), the reward is action % 2: every statistic is an
    integer.  `ledger`: (key, value) of every finished episode, in order — kept on the host, so this env synchronises the
    device once per step, which a test env may do."""

    def __init__(self, num_agents=32, num_actions=4, env0=0, device="cuda"):
        self.num_agents, self.A, self.env0 = int(num_agents), int(num_actions), int(env0)
        self.observation_space = spaces.Dict({"obs": spaces.Box(-np.inf, np.inf, (2,), np.float32)})
        self.action_space = spaces.Discrete(self.A)
        self.device = torch.device(device)
        self.length = torch.from_numpy(episode_stats_lengths(self.env0 + np.arange(self.num_agents))).to(torch.int32).to(self.device)
        self.ledger = []
        self._zero()

    def _zero(self):
        n, dev = self.num_agents, self.device
        self.ret = torch.zeros(n, dtype=torch.float32, device=dev)
        self.steps = torch.zeros(n, dtype=torch.int32, device=dev)
        self.first = torch.zeros(n, dtype=torch.int32, device=dev)

    def _obs(self):
        return {"obs": torch.stack([self.steps.float(), self.ret], 1)}

    def reset(self, **kwargs):
        self._zero()
        return self._obs(), {}

    def step(self, actions):
        a = torch.as_tensor(actions, device=self.device).reshape(-1).to(torch.int32)
        self.first = torch.where(self.steps == 0, a, self.first)
        rew = (a % 2).float()
        self.ret = self.ret + rew
        self.steps = self.steps + 1
        term = self.steps >= self.length
        infos = {"true_objective": 2.0 * self.ret + 1.0,
                 "episode_extra_stats": {"first_action": self.first.clone(), "len_parity": (self.steps % 2).long()},
                 "junk": torch.zeros((self.num_agents, 3), device=self.device)}
        idx = term.nonzero().reshape(-1)
        if idx.numel():
            for key, v in (("reward", self.ret), ("len", self.steps), ("true_objective", infos["true_objective"]),
                           ("first_action", self.first), ("len_parity", infos["episode_extra_stats"]["len_parity"])):
                self.ledger.extend((key, float(x)) for x in v[idx].cpu().tolist())
        keep = ~term
        self.ret, self.steps = self.ret * keep, self.steps * keep  # auto-reset
        return self._obs(), rew, term, torch.zeros_like(term), infos

    def close(self):
        pass


class EpisodeStatsHostEnv:
    """the same game on the host, reporting as host envs do: a list with one info dict per agent, which carries
    true_objective and episode_extra_stats (and an entry that is no number) at the step that ends the agent's episode.
    `ledger` as above; with `ledger_path` every finished episode is also appended to that file as a JSON line (an env that
    lives in a worker process has no other way to show its ledger)."""

    def __init__(self, num_agents=16, num_actions=4, env0=0, ledger_path=None):
        self.num_agents, self.A, self.env0 = int(num_agents), int(num_actions), int(env0)
        self.is_multiagent = True
        self.observation_space = spaces.Dict({"obs": spaces.Box(-np.inf, np.inf, (2,), np.float32)})
        self.action_space = spaces.Discrete(self.A)
        self.length = episode_stats_lengths(self.env0 + np.arange(self.num_agents)).astype(np.int32)
        self.ledger, self.ledger_path = [], ledger_path
        self._zero()

    def _zero(self):
        self.ret = np.zeros(self.num_agents, np.float32)
        self.steps = np.zeros(self.num_agents, np.int32)
        self.first = np.zeros(self.num_agents, np.int32)

    def _obs(self):
        return {"obs": np.stack([self.steps.astype(np.float32), self.ret], 1)}

    def reset(self, **kwargs):
        self._zero()
        return self._obs(), [{} for _ in range(self.num_agents)]

    def step(self, actions):
        a = np.asarray(actions).reshape(-1).astype(np.int32)
        self.first = np.where(self.steps == 0, a, self.first)
        rew = (a % 2).astype(np.float32)
        self.ret = self.ret + rew
        self.steps = self.steps + 1
        term = self.steps >= self.length
        infos, lines = [{} for _ in range(self.num_agents)], []
        for i in np.flatnonzero(term).tolist():
            rec = dict(reward=float(self.ret[i]), len=float(self.steps[i]), true_objective=2.0 * float(self.ret[i]) + 1.0,
                       first_action=float(self.first[i]), len_parity=float(self.steps[i] % 2))
            infos[i] = {"true_objective": rec["true_objective"], "note": "episode over",
                        "episode_extra_stats": {"first_action": int(self.first[i]), "len_parity": int(self.steps[i] % 2)}}
            self.ledger.extend(rec.items())
            lines.append(rec)
        if lines and self.ledger_path:
            import json
            with open(self.ledger_path, "a") as f:
                f.writelines(json.dumps(rec) + "\n" for rec in lines)
        self.ret, self.steps = self.ret * ~term, self.steps * ~term  # auto-reset
        return self._obs(), rew, term, np.zeros(self.num_agents, np.bool_), infos

    def close(self):
        pass


def make_episode_stats_vec_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = int(getattr(cfg, "synthetic_num_agents", None) or 32) if cfg is not None else 32
    e = int(getattr(env_config, "env_id", 0) or 0) if env_config is not None else 0
    return EpisodeStatsVecEnv(num_agents=n, env0=e * n)


def make_episode_stats_host_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    """cfg.synthetic_ledger_dir: every instance appends its finished episodes to <dir>/ledger_<env_id>.jsonl"""
    import os
    n = int(getattr(cfg, "synthetic_num_agents", None) or 16) if cfg is not None else 16
    e = int(getattr(env_config, "env_id", 0) or 0) if env_config is not None else 0
    d = getattr(cfg, "synthetic_ledger_dir", None) if cfg is not None else None
    return EpisodeStatsHostEnv(num_agents=n, env0=e * n, ledger_path=os.path.join(d, f"ledger_{e}.jsonl") if d else None)


class MaskedTupleBanditEnv:
    """MaskedBanditEnv on Tuple(Discrete(n_0), Discrete(n_1), ...): obs = the members' rewarded actions as one-hots side
    by side, obs["action_mask"] u8 [N, sum n_i] with one column per distribution parameter (member i owns the columns
    under its own logits).  A member's rewarded action is always allowed and a random half of its other actions is masked
    out; the reward is the fraction of members that took their rewarded action."""

    def __init__(self, num_agents=64, head_sizes=(4, 3), seed=0, device="cuda"):
        self.num_agents, self.head_sizes = int(num_agents), tuple(int(n) for n in head_sizes)
        assert len(self.head_sizes) > 1 and all(n > 0 for n in self.head_sizes), "a Tuple of Discrete members"
        self.A = sum(self.head_sizes)
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 1, (self.A,), np.float32),
                                              "action_mask": spaces.Box(0, 1, (self.A,), np.uint8)})
        self.action_space = spaces.Tuple([spaces.Discrete(n) for n in self.head_sizes])
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        self._rows = torch.arange(self.num_agents, device=self.device)
        self.last_allowed = None  # [N, members] bool: was member i's action of the last step allowed by its mask
        self._draw()

    def _draw(self):
        N = self.num_agents
        self.target = torch.stack([torch.randint(0, n, (N,), generator=self.gen, device=self.device)
                                   for n in self.head_sizes], 1)
        self.mask = torch.rand((N, self.A), generator=self.gen, device=self.device) < 0.5
        obs, off = torch.zeros((N, self.A), device=self.device), 0
        for i, n in enumerate(self.head_sizes):
            self.mask[self._rows, off + self.target[:, i]] = True
            obs[self._rows, off + self.target[:, i]] = 1.0
            off += n
        self.obs = obs

    def _out(self):
        return {"obs": self.obs, "action_mask": self.mask.to(torch.uint8)}

    def reset(self, **kwargs):
        self._draw()
        return self._out(), {}

    def step(self, actions):
        a = torch.as_tensor(actions, device=self.device).reshape(self.num_agents, len(self.head_sizes)).long()
        offs = torch.tensor([sum(self.head_sizes[:i]) for i in range(len(self.head_sizes))], device=self.device)
        self.last_allowed = self.mask.gather(1, a + offs).clone()
        rew = (a == self.target).float().mean(1)
        term = torch.ones(self.num_agents, dtype=torch.bool, device=self.device)  # one-step episodes, auto-reset
        self._draw()
        return self._out(), rew, term, torch.zeros_like(term), {}

    def close(self):
        pass


def make_masked_tuple_bandit_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = getattr(cfg, "synthetic_num_agents", 64) if cfg is not None else 64
    hs = tuple(getattr(cfg, "synthetic_head_sizes", None) or (4, 3)) if cfg is not None else (4, 3)
    return MaskedTupleBanditEnv(num_agents=n, head_sizes=hs, seed=(getattr(cfg, "seed", None) or 0) if cfg is not None else 0)


def make_synthetic_tuple_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = getattr(cfg, "synthetic_num_agents", 4096) if cfg is not None else 4096
    seed = (getattr(cfg, "seed", None) or 0) if cfg is not None else 0
    return SyntheticTupleEnv(head_sizes=getattr(cfg, "synthetic_head_sizes", (6, 3)) if cfg is not None else (6, 3),
                             num_agents=n, seed=seed)


def make_synthetic_continuous_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = getattr(cfg, "synthetic_num_agents", 2048) if cfg is not None else 2048
    env0 = (getattr(cfg, "synthetic_env0", 0) or 0) if cfg is not None else 0
    env0 += int(getattr(env_config, "env_id", 0) or 0) * n if env_config is not None else 0
    return SyntheticContinuousEnv(num_agents=n, seed=(getattr(cfg, "seed", None) or 0) if cfg is not None else 0, env0=env0)


def make_synthetic_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    n = getattr(cfg, "synthetic_num_agents", 4096) if cfg is not None else 4096
    seed = (getattr(cfg, "seed", None) or 0) if cfg is not None else 0
    env0 = getattr(cfg, "synthetic_env0", 0) if cfg is not None else 0
    # instance e of a multi-instance run simulates global envs [env0 + e*n, env0 + (e+1)*n): the union over instances
    # is the env set of ONE instance with E*n agents (bit-identical rollouts, tests/test_gpu_nn.py)
    env0 += int(getattr(env_config, "env_id", 0) or 0) * n if env_config is not None else 0
    return SyntheticVecEnv(num_agents=n, seed=seed, env0=env0)
