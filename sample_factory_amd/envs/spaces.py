"""Minimal observation/action space descriptors.

gymnasium is the reference's dependency for these (envs/env_utils.py, algo/utils/action_distributions.py:14-38); it
is not installed on the GPU boxes, so the engine duck-types: anything with `.n` is Discrete, anything with `.shape`
and `.dtype` is a Box, anything with `.spaces` mapping is a Dict.  Real gymnasium spaces work unchanged.
"""
from __future__ import annotations

import numpy as np


class Discrete:
    def __init__(self, n: int):
        self.n = int(n)
        self.shape = ()
        self.dtype = np.dtype(np.int64)

    def __repr__(self):
        return f"Discrete({self.n})"


class Box:
    def __init__(self, low, high, shape, dtype=np.float32):
        self.low, self.high = low, high
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)

    def __repr__(self):
        return f"Box({self.shape}, {self.dtype})"


class Dict:
    def __init__(self, spaces):
        self.spaces = dict(spaces)

    def keys(self):
        return self.spaces.keys()

    def items(self):
        return self.spaces.items()

    def __getitem__(self, k):
        return self.spaces[k]

    def __repr__(self):
        return "Dict(" + ", ".join(f"{k!r}: {v!r}" for k, v in self.spaces.items()) + ")"


class Tuple:
    """gymnasium.spaces.Tuple stand-in (multi-head action spaces, e.g. VizDoom: move / turn / attack)"""

    def __init__(self, spaces):
        self.spaces = tuple(spaces)

    def __iter__(self):
        return iter(self.spaces)

    def __len__(self):
        return len(self.spaces)

    def __getitem__(self, i):
        return self.spaces[i]

    def __repr__(self):
        return f"Tuple({', '.join(repr(s) for s in self.spaces)})"


def is_discrete(space) -> bool:
    return hasattr(space, "n")


MAX_ACTION_HEADS = 64  # SF_MAX_ACTION_HEADS of include/sf_hip.h: the members of a Tuple the native kernels take


def is_tuple(space) -> bool:
    return hasattr(space, "spaces") and not hasattr(space, "keys")


def action_head_sizes(action_space):
    """members of the action distribution as the native loss / sampler kernels take them: [n] for Discrete(n); one entry
    per member of a Tuple — n for Discrete(n), -D for Box(D) (2 D parameters [means | log_std], D action columns;
    action_distributions.py:197-287 composes any members) — at most MAX_ACTION_HEADS; [] for a bare Box"""
    if is_discrete(action_space):
        return [int(action_space.n)]
    if is_tuple(action_space):
        if len(action_space.spaces) > MAX_ACTION_HEADS:
            raise NotImplementedError(f"at most {MAX_ACTION_HEADS} action heads, got {len(action_space.spaces)}")
        out = []
        for sp in action_space.spaces:
            if is_discrete(sp):
                out.append(int(sp.n))
            elif is_box(sp):
                if len(sp.shape) != 1:
                    raise Exception("Non-trivial shape Box action spaces not currently supported. Try to flatten the space.")
                out.append(-int(sp.shape[0]))
            else:
                raise NotImplementedError(f"Tuple member {sp!r}: only Discrete and Box members are supported")
        return out
    return []


def heads_action_cols(heads) -> int:
    """action columns of a head list: one per Discrete member, D per Box(D) member (entry -D)"""
    return sum(1 if h > 0 else -h for h in heads)


def heads_mixed(heads) -> bool:
    """a Tuple with at least one Box member: its actions travel as f32 rows and are split per member for the env"""
    return any(h < 0 for h in heads)


def split_tuple_actions(rows, heads, batched: bool = True):
    """what `preprocess_actions` hands the env for a Tuple with a Box member (batched_sampling.py:51-59): one array per
    member — int32 with the action axis squeezed for a Discrete member, f32 [agents, D] for a Box(D) member.  `rows`:
    [agents, heads_action_cols] f32 (numpy or torch)."""
    out, c = [], 0
    is_torch = hasattr(rows, "dim")
    for h in heads:
        if h > 0:
            col = rows[:, c]
            if is_torch:
                import torch
                col = col.to(torch.int32)
            else:
                col = col.astype(np.int32)
            out.append(col if batched else int(col[0]))
            c += 1
        else:
            blk = rows[:, c:c - h]
            out.append(blk if batched else blk[0])
            c -= h
    return out


def is_box(space) -> bool:
    return not hasattr(space, "n") and hasattr(space, "shape") and getattr(space, "shape", None) is not None and not hasattr(space, "spaces")


def framestack_keys(obs_space, k: int = 2):
    """the observation keys --device_framestack stacks: every key whose space has three dimensions (CHW), never the
    action mask; [] for k == 1"""
    items = obs_space.spaces.items() if hasattr(obs_space, "spaces") else [("obs", obs_space)]
    return [name for name, sp in items if int(k) > 1 and name != "action_mask" and len(getattr(sp, "shape", ()) or ()) == 3]


def stacked_obs_space(obs_space, k: int):
    """the observation space the slab, the model and the learner see under --device_framestack=k: a Dict in which every
    3-D (CHW) key has become Box(k * C, H, W) — low / high tiled along the channel axis, dtype kept — and every other key
    (vectors, the action mask) is the env's own space object.  k == 1: the space as it is."""
    k = int(k)
    if k < 1:
        raise ValueError(f"device_framestack={k}: the frame stack holds at least one frame")
    if k == 1:
        return obs_space
    keys = framestack_keys(obs_space, k)
    if not keys:
        raise ValueError(f"device_framestack={k}: the observation space {obs_space!r} has no key with three dimensions "
                         "(CHW) to stack")
    out = {}
    for name, sp in (obs_space.spaces.items() if hasattr(obs_space, "spaces") else [("obs", obs_space)]):
        if name not in keys:
            out[name] = sp
            continue

        def tiled(b):
            b = np.asarray(b)
            return np.tile(b, (k, 1, 1)) if b.ndim == 3 else (b.item() if b.ndim == 0 else b)  # scalar bounds stay scalar
        c, h, w = sp.shape
        out[name] = Box(tiled(sp.low), tiled(sp.high), (k * int(c), int(h), int(w)), sp.dtype)
    return Dict(out)


def chw_obs_space(obs_space):
    """the observation space the slab, the model and the learner see under --hwc_observations: a Dict in which every 3-D
    key (the keys framestack_keys picks; the env delivers them as [H, W, C]) has become Box(C, H, W) — array bounds
    transposed, scalar bounds scalar, dtype kept — and every other key (vectors, the action mask) is the env's own space
    object"""
    keys = framestack_keys(obs_space)
    if not keys:
        raise ValueError(f"hwc_observations: the observation space {obs_space!r} has no key with three dimensions (HWC) to "
                         "transpose")
    out = {}
    for name, sp in (obs_space.spaces.items() if hasattr(obs_space, "spaces") else [("obs", obs_space)]):
        if name not in keys:
            out[name] = sp
            continue

        def chw(b):
            b = np.asarray(b)
            return np.ascontiguousarray(b.transpose(2, 0, 1)) if b.ndim == 3 else (b.item() if b.ndim == 0 else b)
        h, w, c = sp.shape
        out[name] = Box(chw(sp.low), chw(sp.high), (int(c), int(h), int(w)), sp.dtype)
    return Dict(out)


def resized_obs_space(obs_space, OH: int, OW: int, grayscale: bool):
    """the observation space the slab, the model and the learner see under --device_resize OH OW / --device_grayscale: a
    Dict in which every 3-D key of the CHW space (the keys framestack_keys picks) has become Box(C', OH, OW), C' = 1 under
    grayscale (C must be 3), else C.  The key must be u8.  Scalar bounds are kept; array bounds collapse to their min and
    max (a resized pixel lies between the smallest and the largest bound of the pixels it averages).  Every other key
    (vectors, the action mask) is the env's own space object."""
    OH, OW = int(OH), int(OW)
    if OH < 1 or OW < 1:
        raise ValueError(f"device_resize {OH} {OW}: each at least 1")
    keys = framestack_keys(obs_space)
    if not keys:
        raise ValueError(f"device_resize / device_grayscale: the observation space {obs_space!r} has no key with three "
                         "dimensions (an image) to preprocess")
    out = {}
    for name, sp in (obs_space.spaces.items() if hasattr(obs_space, "spaces") else [("obs", obs_space)]):
        if name not in keys:
            out[name] = sp
            continue
        if np.dtype(sp.dtype) != np.uint8:
            raise ValueError(f"device_resize / device_grayscale: observation key {name!r} is {np.dtype(sp.dtype).name}, only "
                             "uint8 frames are preprocessed on the device")
        c = int(sp.shape[0])
        if grayscale and c != 3:
            raise ValueError(f"device_grayscale: observation key {name!r} has {c} channels, grey-scale needs 3 (R, G, B)")
        low, high = np.asarray(sp.low), np.asarray(sp.high)
        out[name] = Box(low.item() if low.ndim == 0 else low.min().item(), high.item() if high.ndim == 0 else high.max().item(),
                        (1 if grayscale else c, OH, OW), sp.dtype)
    return Dict(out)


def calc_num_actions(action_space) -> int:
    """action_distributions.py:14-26"""
    if is_discrete(action_space):
        return 1
    if is_tuple(action_space):
        return sum(calc_num_actions(a) for a in action_space.spaces)
    if is_box(action_space):
        if len(action_space.shape) != 1:
            raise Exception("Non-trivial shape Box action spaces not currently supported. Try to flatten the space.")
        return action_space.shape[0]
    raise NotImplementedError(f"Action space type {type(action_space)} not supported!")


def calc_num_action_parameters(action_space) -> int:
    """action_distributions.py:29-38"""
    if is_discrete(action_space):
        return action_space.n
    if is_tuple(action_space):
        return sum(calc_num_action_parameters(a) for a in action_space.spaces)
    if is_box(action_space):
        return int(np.prod(action_space.shape)) * 2
    raise NotImplementedError(f"Action space type {type(action_space)} not supported!")
