"""How an env's observation gets into the trajectory slab: one plan per observation key, derived once from the env's
observation space and the flags, and one route per key that carries it out.  The stages, in the only order they run in:

  1. --hwc_observations                         the env delivers image keys [H, W, C]; the slab holds them (C, H, W)
  2. --device_resize H W / --device_grayscale   u8 image keys become (C', OH, OW), C' = 1 under grey-scale (which, alone,
                                                keeps the key's own size): the resize acts on the CHW space
  3. --device_framestack=k                      the slab holds the last k preprocessed frames, oldest first: (k C', H', W')

Image keys are the 3-D keys, never the action mask (envs/spaces.py framestack_keys); every other key is copied into its
slab column as it is.  The slab, the model and the learner are built from `slab_obs_space()`; the env's own EnvInfo keeps
describing the env.  A zero-copy env (`step_into` writes whole observations into the slab) bypasses the routes, so every
stage is refused for it.  Importing this module does not load the native library."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import torch

from sample_factory_amd import lib
from sample_factory_amd.algo.utils.env_info import device_resize_of
from sample_factory_amd.envs.spaces import chw_obs_space, framestack_keys, resized_obs_space, stacked_obs_space


@dataclass(frozen=True)
class KeyIngest:
    """one observation key: what the env delivers and what the slab holds.  A key that is no image has no stage:
    hwc False, resize None, k 1 and frame_shape == slab_shape == native_shape"""
    name: str
    native_shape: Tuple[int, ...]
    dtype: Any
    image: bool = False                       # 3-D and not the action mask
    hwc: bool = False                         # frames arrive [H, W, C]
    resize: Optional[Tuple[int, int]] = None  # (OH, OW) sf_frame_resize writes; grey-scale alone: the key's own size
    interp: str = "area"
    gray: bool = False
    k: int = 1                                # frames in the stack, 1 = none
    frame_shape: Tuple[int, ...] = ()         # (C', H', W') of one preprocessed frame
    slab_shape: Tuple[int, ...] = ()          # (k * C', H', W')


def _shape(space, name) -> Tuple[int, ...]:
    return tuple(int(d) for d in (getattr(space[name] if hasattr(space, "spaces") else space, "shape", None) or ()))


_framestack_warned = False


@dataclass(frozen=True)
class ObsIngestPlan:
    keys: Dict[str, KeyIngest]  # in the space's key order
    identity: bool              # no key is processed
    slab_space: Any

    def slab_obs_space(self):  # what the slab, the model and the learner see; the env's own space for the identity plan
        return self.slab_space

    @classmethod
    def from_cfg(cls, obs_space, cfg, zero_copy: bool) -> "ObsIngestPlan":
        """ValueError: flags and spaces the device stages cannot serve; NotImplementedError: any stage on a zero-copy env"""
        global _framestack_warned
        hwc, k = bool(getattr(cfg, "hwc_observations", False)), int(getattr(cfg, "device_framestack", 1))
        size, interp, gray = device_resize_of(cfg)
        images = framestack_keys(obs_space)
        chw = frames = chw_obs_space(obs_space) if hwc else obs_space  # ValueError: nothing to transpose
        if size is not None or gray:
            if size is None:  # grey-scale alone: every image key keeps its own geometry
                sizes = {_shape(chw, name)[1:] for name in images}
                if len(sizes) > 1:
                    raise ValueError(f"device_grayscale without device_resize: the image keys {images} differ in size "
                                     f"{sorted(sizes)}; give --device_resize H W")
                size = next(iter(sizes)) if sizes else (1, 1)
            frames = resized_obs_space(chw, size[0], size[1], gray)  # ValueError: no image key, not u8, grey of C != 3
            for name in images if interp == "area" else ():
                h, w = _shape(chw, name)[1:]
                if size[0] > h or size[1] > w:
                    raise ValueError(f"device_resize {size[0]} {size[1]} with the area filter enlarges observation key "
                                     f"{name!r} ({h} x {w}): the area filter only shrinks, use "
                                     "--device_resize_interpolation=nearest")
        slab = stacked_obs_space(frames, k)  # ValueError: k < 1, or nothing to stack
        stages = [(hwc, "hwc_observations", "write CHW there, or let the env return its HWC frames from step()"),
                  (size is not None, "device_resize / device_grayscale", "preprocess inside the env, or let it return its "
                   "native frames from step()"),
                  (k > 1, f"device_framestack={k}", "stack inside the env, or let it return single frames from step()")]
        active = [(what, advice) for on, what, advice in stages if on]
        if active and zero_copy:
            raise NotImplementedError("%s with a zero-copy env (step_into writes whole observations into the slab): %s"
                                      % active[0])
        if k > 1 and int(getattr(cfg, "env_framestack", 1) or 1) > 1 and not _framestack_warned:
            from sample_factory_amd.utils.utils import log
            _framestack_warned = True
            log.warning("env_framestack=%d and device_framestack=%d are both set: an env factory that reads env_framestack "
                        "stacks on its own and the device would stack those stacks; set env_framestack=1 unless the factory "
                        "ignores it", int(cfg.env_framestack), k)
        keys = {}
        for name, sp in (obs_space.spaces.items() if hasattr(obs_space, "spaces") else [("obs", obs_space)]):
            native, dtype = _shape(obs_space, name), getattr(sp, "dtype", None)
            keys[name] = KeyIngest(name, native, dtype, True, hwc, size, interp, gray, k, _shape(frames, name),
                                   _shape(slab, name)) if name in images else \
                KeyIngest(name, native, dtype, frame_shape=native, slab_shape=native)
        return cls(keys, not active, slab)


class KeyRoute:
    """one key's way into the slab leaf x = traj["obs"][key] (an argument of every call: the runner switches slabs).
    `stage`: its one device staging buffer, [B, native frame] in the env's own layout, None for a key without a transpose
    or resize.  `frame`: after store(), what the device launch reads — `stage`, or a device env's own tensor in place."""

    def __init__(self, key: KeyIngest, x: torch.Tensor):
        self.key = key
        staged = key.hwc or key.resize is not None
        self.stage = torch.empty((x.shape[0],) + key.native_shape, dtype=x.dtype, device=x.device) if staged else None
        self.frame: Optional[torch.Tensor] = None

    def slot(self, x: torch.Tensor, t: int) -> torch.Tensor:
        """where the newest frame goes in slab column t: the column, or its LAST frame slot (still one pitched DMA)"""
        return x[:, t] if self.key.k == 1 else x[:, t, (self.key.k - 1) * self.key.frame_shape[0]:]

    def store(self, x: torch.Tensor, name: str, src, t: int, to_device) -> None:
        """the env's observation `src` -> slab column t, by the runner's to_device(name, src, dst).  A staged key goes to its
        buffer that way (a device env's tensor with contiguous rows is read where it is) and its kernel follows on the same
        stream: sf_frame_resize into the slot — it reads channel-last frames itself — or sf_hwc_to_chw into the column; a
        stacked channel-last key waits for complete(), which transposes it inside the stack's launch"""
        key, stage = self.key, self.stage
        if stage is None:
            to_device(name, src, self.slot(x, t))
            return
        if isinstance(src, torch.Tensor) and src.is_cuda and src.shape == stage.shape and src.dtype == stage.dtype and \
                src[0].is_contiguous():
            self.frame = src
        else:
            to_device(name, src, stage)
            self.frame = stage
        if key.resize is not None:
            lib.frame_resize(self.slot(x, t), self.frame, key.hwc, key.interp, key.gray)
        elif key.k == 1:
            lib.hwc_to_chw(x[:, t], self.frame)

    def complete(self, x: torch.Tensor, t: int, term, trunc) -> None:
        """complete a stacked key's column t around the frame store() put into its last slot — or, a channel-last key, left
        in `frame`: one launch (term / trunc: the device flags of the step that produced the frame; None, None: a reset)"""
        key = self.key
        if key.k == 1:
            return
        prev = x[:, t - 1 if t > 0 else 1]
        if key.hwc and key.resize is None:
            lib.framestack_step_hwc(x[:, t], prev, key.k, self.frame, term, trunc)
        else:
            lib.framestack_step(x[:, t], prev, key.k, None, term, trunc)
