"""Statistics an env defines itself: what the reference reports at the end of an episode besides reward
and length —

  * per-agent dicts (non_batched_sampling.py:290-301): info["true_objective"] and every entry of
    info["episode_extra_stats"], at the step where the agent is done;
  * a dict of per-env arrays (batched_sampling.py:235-251): every leaf with one element per agent, at the envs that
    finished, under its flattened key.

Everything here is host arithmetic on `key -> [sum, count]` dictionaries: list infos of host envs, host arrays in dict
infos, the replies of env worker processes.  Device tensors in dict infos never come here: they are summed where they live
(sf_episode_stats_add) and meet these dictionaries once per report.
"""
from __future__ import annotations

import numbers
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np

TRUE_OBJECTIVE, EXTRA_STATS = "true_objective", "episode_extra_stats"
IS_ACTIVE = "is_active"  # consumed by --track_inactive_agents, not a statistic


def flatten_infos(infos: dict, prefix: Tuple[str, ...] = ()) -> Iterator[Tuple[str, object]]:
    """(flattened key, leaf) of a possibly nested infos dict, in the dict's own order: the keys the reference builds in
    batched_sampling.py:237-240 from iterate_recursively_with_prefix (utils/dicts.py:35-49) — "a/b/key"."""
    for k, v in infos.items():
        if isinstance(v, dict):
            yield from flatten_infos(v, prefix + (str(k),))
        else:
            yield "/".join(prefix + (str(k),)), v


def stat_key(flat_key: str) -> str:
    """the name a flattened key is reported under: an entry x of episode_extra_stats is `x` in both shapes of infos (the
    per-agent form reports it as `x`, non_batched_sampling.py:297-301), everything else keeps its flattened key"""
    head = EXTRA_STATS + "/"
    return flat_key[len(head):] if flat_key.startswith(head) and len(flat_key) > len(head) else flat_key


def as_number(v) -> Optional[float]:
    """a numeric scalar as float, anything else (strings, None, arrays of several elements, containers) as None"""
    if isinstance(v, (bool, np.bool_)):
        return float(v)
    if isinstance(v, numbers.Number) and not isinstance(v, complex):
        return float(v)
    if isinstance(v, np.ndarray) or hasattr(v, "numel"):  # a 0-d / one-element array or tensor
        a = np.asarray(v.cpu() if hasattr(v, "cpu") else v)
        if a.size == 1 and (np.issubdtype(a.dtype, np.number) or a.dtype == np.bool_) and \
                not np.issubdtype(a.dtype, np.complexfloating):
            return float(a.reshape(-1)[0])
    return None


def per_env_array(v, n: int) -> Optional[np.ndarray]:
    """a host leaf of dict infos as a flat array if it holds one numeric / bool element per agent, else None"""
    if hasattr(v, "is_cuda"):
        if v.is_cuda:
            return None
        v = v.numpy()
    if not isinstance(v, np.ndarray) or v.size != n or not (np.issubdtype(v.dtype, np.number) or v.dtype == np.bool_) or \
            np.issubdtype(v.dtype, np.complexfloating):
        return None
    return v.reshape(-1)


class HostEpisodeStats:
    """key -> [sum, count] over the episodes that finished since the last pop()"""

    def __init__(self):
        self.sums: Dict[str, List[float]] = {}

    def add(self, key: str, total: float, count: float = 1.0) -> None:
        slot = self.sums.get(key)
        if slot is None:
            self.sums[key] = [float(total), float(count)]
        else:
            slot[0] += float(total)
            slot[1] += float(count)

    def add_agent(self, info) -> None:
        """the report of ONE agent whose episode just ended: true_objective if present and numeric, every numeric scalar
        of episode_extra_stats (nested dicts flattened with "/")"""
        if not isinstance(info, dict):
            return
        v = as_number(info.get(TRUE_OBJECTIVE))
        if v is not None:
            self.add(TRUE_OBJECTIVE, v)
        extra = info.get(EXTRA_STATS)
        if isinstance(extra, dict):
            for key, leaf in flatten_infos(extra):
                v = as_number(leaf)
                if v is not None:
                    self.add(key, v)

    def add_list_infos(self, infos, done) -> None:
        """infos: one dict per agent; done: bool per agent (terminated | truncated of this step)"""
        for i in np.flatnonzero(np.asarray(done).reshape(-1)).tolist():
            if i < len(infos):
                self.add_agent(infos[i])

    def add_single(self, info, done: bool) -> None:
        """a single-agent env: its info dict and whether this step ended the episode"""
        if done:
            self.add_agent(info)

    def add_dict_infos(self, infos: dict, done, keys=None) -> None:
        """dict infos of host arrays: every leaf with one numeric element per agent, taken at the finished envs.
        keys: the fixed channel set (flattened keys) — None takes every leaf that qualifies"""
        done = np.asarray(done).reshape(-1)
        idx = np.flatnonzero(done)
        if idx.size == 0:
            return
        for key, leaf in flatten_infos(infos):
            if key == IS_ACTIVE or (keys is not None and key not in keys):
                continue
            a = per_env_array(leaf, done.size)
            if a is not None:
                self.add(stat_key(key), float(a[idx].astype(np.float64).sum()), float(idx.size))

    def add_infos(self, infos, done) -> None:
        """whatever shape a batched env instance's step returned: a dict of per-agent arrays, or one dict per agent"""
        if isinstance(infos, dict):
            self.add_dict_infos(infos, done)
        elif isinstance(infos, (list, tuple)):
            self.add_list_infos(infos, done)

    def merge(self, other: Optional[Dict[str, List[float]]]) -> None:
        """add a dictionary of the same shape (a worker's reply, another accumulator's pop())"""
        for key, (total, count) in (other or {}).items():
            self.add(key, total, count)

    def pop(self) -> Dict[str, List[float]]:
        out, self.sums = self.sums, {}
        return out

    def __bool__(self) -> bool:
        return bool(self.sums)


def merge_sums(into: Dict[str, List[float]], other: Optional[Dict[str, List[float]]]) -> Dict[str, List[float]]:
    for key, (total, count) in (other or {}).items():
        slot = into.setdefault(key, [0.0, 0.0])
        slot[0] += float(total)
        slot[1] += float(count)
    return into


def episodic_message(reward_sum: float, len_sum: float, episodes: float, sums: Dict[str, List[float]]) -> Optional[dict]:
    """the body of one EPISODIC message: the means since the previous report (the convention of reward / len), a key's own
    count under episodes_<key> only where it differs from `episodes`; None when nothing finished and nothing was reported"""
    msg = {}
    if episodes > 0:
        msg.update(reward=reward_sum / episodes, len=len_sum / episodes, episodes=episodes)
    for key, (total, count) in sums.items():
        if count > 0 and key not in ("reward", "len", "episodes"):
            msg[key] = total / count
            if count != episodes:
                msg[f"episodes_{key}"] = count
    return msg or None
