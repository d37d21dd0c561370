"""Model plugin surface — sample_factory/model/model_factory.py:16-60 + algo/utils/context.py (global_model_factory).

    global_model_factory().register_actor_critic_factory(make_actor_critic_func)   # (cfg, obs_space, action_space) -> nn.Module
    global_model_factory().register_encoder_factory(make_encoder_func)             # (cfg, obs_space) -> Encoder module
    global_model_factory().register_model_core_factory / register_decoder_factory  # (cfg, in_size) -> module

The DEFAULT models run on the native HIP path: `ActorCritic` (model/actor_critic.py) for one observation key,
`MultiKeyActorCritic` (model/actor_critic_multikey.py) for several keys and for cfg.encoder_conv_architecture =
resnet_impala, `SeparateActorCritic` (model/actor_critic_separate.py) for cfg.actor_critic_share_weights=False; every
recurrent depth and u8 or f32 image frames included.  `create_actor_critic` decides which one to try in one place
(`_native_candidate`).  A user-registered part, a configuration the native models do not take (a CPU device for all but the
single-key model, float64 frames, resnet_impala with separate weights, ...) and the SF_NATIVE_RESNET / _MULTIKEY /
_SEPARATE_WEIGHTS / _F32FRAMES=0 switches get the network in torch instead: `TorchPolicyAdapter` (model/torch_policy.py)
drives the module through torch autograd on the GPU while everything around the network — rollout sampling, slab protocol,
GAE, returns normaliser, PPO loss forward/backward, gradient clipping, Adam/Lamb on one flat buffer, data-parallel
all-reduce — stays on the native kernels ("native fast-path only when the factory is the default, otherwise
fall back to autograd through the user module").
"""
from __future__ import annotations

import os
from typing import Callable, Optional

import numpy as np
import torch


class ModelFactory:
    def __init__(self):
        self.make_actor_critic_func: Optional[Callable] = None   # None = the native default
        self.make_model_encoder_func: Optional[Callable] = None
        self.make_model_core_func: Optional[Callable] = None
        self.make_model_decoder_func: Optional[Callable] = None

    def register_actor_critic_factory(self, make_actor_critic_func: Callable):
        """Override the default actor-critic with a custom model: f(cfg, obs_space, action_space) -> nn.Module"""
        self.make_actor_critic_func = make_actor_critic_func

    def register_encoder_factory(self, make_model_encoder_func: Callable):
        """observations -> ENCODER -> core -> decoder -> heads: f(cfg, obs_space) -> module with get_out_size()"""
        self.make_model_encoder_func = make_model_encoder_func

    def register_model_core_factory(self, make_model_core_func: Callable):
        self.make_model_core_func = make_model_core_func

    def register_decoder_factory(self, make_model_decoder_func: Callable):
        self.make_model_decoder_func = make_model_decoder_func

    def is_default(self) -> bool:
        return (self.make_actor_critic_func is None and self.make_model_encoder_func is None and
                self.make_model_core_func is None and self.make_model_decoder_func is None)

    def reset(self):
        self.__init__()


_FACTORY = ModelFactory()


def global_model_factory() -> ModelFactory:
    return _FACTORY


def _native_candidate(cfg, obs_space, device):
    """(the native model class to try for this configuration, None), or (None, why not: None for user-registered parts)"""
    if not global_model_factory().is_default():
        return None, None
    from sample_factory_amd.model.actor_critic import ActorCritic
    from sample_factory_amd.model.actor_critic_multikey import MultiKeyActorCritic
    from sample_factory_amd.model.actor_critic_separate import SeparateActorCritic
    from sample_factory_amd.model.encoder_resnet import uses_resnet
    from sample_factory_amd.model.torch_policy import obs_keys_of

    def off(switch):
        return os.environ.get(switch, "1") == "0"

    keys = obs_keys_of(obs_space)
    multi, separate = len(keys) > 1, not cfg.actor_critic_share_weights
    cuda = torch.device(device).type == "cuda"
    if uses_resnet(cfg, obs_space):  # on any device and frame dtype: the resnet tower refuses what it cannot run
        if off("SF_NATIVE_RESNET"):
            return None, "resnet_impala with SF_NATIVE_RESNET=0"
        if separate:
            return None, "resnet_impala with separate actor / critic weights"
        if multi and off("SF_NATIVE_MULTIKEY"):
            return None, "resnet_impala with several observation keys and SF_NATIVE_MULTIKEY=0"
        return MultiKeyActorCritic, None
    if any(len(obs_space[k].shape) == 3 and np.dtype(obs_space[k].dtype) == np.float32 for k in keys):
        if not cuda:
            return None, "float32 image frames on a CPU device"
        if off("SF_NATIVE_F32FRAMES"):
            return None, "float32 image frames with SF_NATIVE_F32FRAMES=0"
    if not separate and not multi:
        return ActorCritic, None  # on any device
    if not cuda:
        return None, "separate actor / critic weights or several observation keys on a CPU device"
    if multi and off("SF_NATIVE_MULTIKEY"):
        return None, "several observation keys with SF_NATIVE_MULTIKEY=0"
    if separate:
        if off("SF_NATIVE_SEPARATE_WEIGHTS"):
            return None, "separate actor / critic weights with SF_NATIVE_SEPARATE_WEIGHTS=0"
        return SeparateActorCritic, None
    return MultiKeyActorCritic, None


def create_actor_critic(cfg, obs_space, action_space, device, all_reduce=None):
    """model/actor_critic.py:337-342 create_actor_critic: the native model unless the user registered something or the
    native kernels do not take this configuration; then the network in torch (everything around it stays native)"""
    from sample_factory_amd.model.torch_policy import TorchPolicyAdapter, build_torch_actor_critic
    from sample_factory_amd.utils.utils import log
    cls, why_not = _native_candidate(cfg, obs_space, device)
    if cls is not None:
        try:
            return cls(cfg, obs_space, action_space, device, all_reduce=all_reduce)
        except NotImplementedError as e:  # a shape the native model refuses (e.g. float64 frames)
            why_not = f"{cls.__name__}: {e}"
    if why_not is not None:
        log.warning("the network runs in torch: %s", why_not)
    f = global_model_factory()
    if f.make_actor_critic_func is not None:
        module = f.make_actor_critic_func(cfg, obs_space, action_space)
    else:
        module = build_torch_actor_critic(cfg, obs_space, action_space, f)
    return TorchPolicyAdapter(cfg, obs_space, action_space, device, module, all_reduce=all_reduce)
