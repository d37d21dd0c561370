"""Observation dicts with SEVERAL keys on the NATIVE kernels (reference: MultiInputEncoder inside ActorCriticSharedWeights,
sample_factory/model/encoder.py:33-69, model/actor_critic.py:136-196): one encoder per key in sorted key order — an MLP for a
1-D key, the conv stack + its fully connected layers for an image key — their outputs concatenated column-wise, then the
recurrent core, the decoder and the two heads.

A tower composite (model/composite.py) on [encoder of key 0 | encoder of key 1 | ... | trunk]: one tower per key, an
`ActorCritic` in its `part="encoder"` form or a `ResnetImpalaTower`, and one `ActorCritic(part="trunk")` tower (core +
decoder + fused heads on the concatenated feature batch).  The single-key resnet_impala model is this composite with one
encoder tower.  Forward: every encoder tower runs its own kernels on its key's slab leaf (in place: u8 frames, index /
offset / trajectory addressing are the tower's), its [n, f_k] output is copied into columns [o_k, o_k + f_k) of the [n, F] feature batch (sf_copy_rows), the trunk
runs on that.  Backward: the trunk's first data gradient IS d(loss) / d(pre-activation of the encoders' outputs) (the
activation derivative is fused into its epilogue as between any two layers), its column blocks are the encoders' incoming
gradients.  Parameter names and order are the reference's (encoder.encoders.<key>.*, core.*, decoder.*, critic_linear.*,
action_parameterization.*); per-key normalisation rules are normalize.py:24-70's (mean shift / scale on the key "obs" only,
running statistics for the keys in cfg.normalize_input_keys)."""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch

from sample_factory_amd import lib
from sample_factory_amd.envs import spaces
from sample_factory_amd.model.actor_critic import ActorCritic
from sample_factory_amd.model.composite import TowerComposite
from sample_factory_amd.model.encoder_resnet import ResnetImpalaTower, uses_resnet


class _KeyedNormalizers:
    """what the Learner updates once per dataset (learner.py:957-961) when the observation is a dict of several keys"""

    def __init__(self, towers: Dict[str, ActorCritic]):
        self.towers = towers

    def update(self, obs, stride: int, n: int, **_):
        if not isinstance(obs, dict):  # the single-key resnet_impala model is handed its one slab leaf
            obs = {next(iter(self.towers)): obs}
        for k, t in self.towers.items():
            if t.obs_normalizer is not None:
                t.obs_normalizer.update(obs[k], t.obs_elems, n)


class MultiKeyActorCritic(TowerComposite):
    _buf_prefix = "mk"

    def __init__(self, cfg, obs_space, action_space, device="cuda", all_reduce=None):
        self.cfg = cfg
        self.obs_keys = sorted(k for k in obs_space.spaces.keys() if k != "action_mask")
        # an image key under resnet_impala is a ResnetImpalaTower (model/encoder_resnet.py): that tower + the trunk is also
        # how the single-key resnet_impala model runs
        resnet = uses_resnet(cfg, obs_space)
        if len(self.obs_keys) < 2 and not resnet:
            raise NotImplementedError("MultiKeyActorCritic: an observation dict with at least two keys")
        if not cfg.actor_critic_share_weights:
            raise NotImplementedError("separate actor / critic weights with several observation keys")

        def encoder(k):
            if resnet and len(obs_space[k].shape) == 3:
                return ResnetImpalaTower(cfg, obs_space, action_space, device, all_reduce=all_reduce, obs_key=k)
            return ActorCritic(cfg, obs_space, action_space, device, all_reduce=all_reduce, obs_key=k, part="encoder")

        self.encoders: Dict[str, ActorCritic] = {k: encoder(k) for k in self.obs_keys}
        # several keys: the Learner / rollout runner pass {key: slab view} dicts; one key: the bare view (see _keyed)
        self.multi_key = len(self.obs_keys) > 1
        self.feat_of = {k: e.feat for k, e in self.encoders.items()}
        self.col0, F = {}, 0
        for k in self.obs_keys:
            self.col0[k] = F
            F += self.feat_of[k]
        self.F = F
        tspace = spaces.Dict({"obs": spaces.Box(-np.inf, np.inf, (F,), np.float32)})
        self.trunk = ActorCritic(cfg, tspace, action_space, device, all_reduce=all_reduce, part="trunk")
        t = self.trunk
        self.device, self.obs_space, self.action_space = t.device, obs_space, action_space
        self.obs_shapes = {k: e.obs_shape for k, e in self.encoders.items()}
        main = "obs" if "obs" in self.encoders else self.obs_keys[0]
        self.obs_shape, self.obs_elems, self.obs_u8 = (self.encoders[main].obs_shape, self.encoders[main].obs_elems,
                                                       self.encoders[main].obs_u8)
        self.num_action_params, self.heads_ld = t.num_action_params, t.heads_ld
        self.rnn_kind, self.rnn_H, self.rnn_S, self.rnn_L, self.rnn_SL = t.rnn_kind, t.rnn_H, t.rnn_S, t.rnn_L, t.rnn_SL
        self.nonadaptive_std, self.tanh_scale = t.nonadaptive_std, t.tanh_scale
        self._seat_towers([self.encoders[k] for k in self.obs_keys] + [t], lead=t)
        self.returns_normalizer = t.returns_normalizer
        self.obs_normalizer = _KeyedNormalizers(self.encoders) if any(
            e.obs_normalizer is not None for e in self.encoders.values()) else None

    # ------------------------------------------------------------------------------------------ reference surface
    def num_params(self) -> int:
        return sum(tw.num_params() for tw in self.towers)

    def ref_param_shapes(self):
        return [x for tw in self.towers for x in tw.ref_param_shapes()]

    def state_dict(self) -> Dict[str, torch.Tensor]:
        parts = [tw.state_dict() for tw in self.towers]
        sd = {k: v for p in parts for k, v in p.items() if k.startswith(("obs_normalizer.", "returns_normalizer."))}
        for p in parts:  # the parameters in the reference's registration order
            sd.update({k: v for k, v in p.items() if not k.startswith(("obs_normalizer.", "returns_normalizer."))})
        return sd

    def load_state_dict(self, sd, strict=True):
        for tw in self.towers:
            if strict:
                for n, _ in tw.ref_param_shapes():
                    if n not in sd:
                        raise KeyError(n)
            tw.load_state_dict(sd, strict=strict)

    # ---- what a separate-weights composite needs from its towers (model/composite.py)
    @property
    def heads_layer(self):
        return self.trunk.layers[-1]

    def share_normalizers_from(self, other) -> None:
        for k, e in self.encoders.items():
            e.obs_normalizer = other.encoders[k].obs_normalizer
        self.obs_normalizer = other.obs_normalizer
        self.trunk.returns_normalizer = self.returns_normalizer = None

    def share_seq_sync_from(self, other) -> None:
        self.trunk.share_seq_sync_from(other.trunk)

    def _seq_sync_buf(self):
        return self.trunk._seq_sync_buf()

    def share_snapshot_tables_from(self, other) -> None:
        for k, e in self.encoders.items():
            e._snap_tabs = other.encoders[k]._snap_tabs

    def normalizer_state(self) -> Dict[str, torch.Tensor]:
        return {k: v for e in self.encoders.values() for k, v in e.normalizer_state().items()}

    def load_normalizer_state(self, sd) -> None:
        for e in self.encoders.values():
            e.load_normalizer_state(sd)

    # ------------------------------------------------------------------------------------------ forward / backward
    def _keyed(self, obs):
        return obs if isinstance(obs, dict) else {self.obs_keys[0]: obs}

    def _stride_of(self, k, view, traj_T):
        """elements between two samples of key k: the learner addresses whole slab leaves [E, T + 1, ...] by dataset row
        (sf_common.h sample_base: dense frames), a rollout / bootstrap step hands one column view [B, ...] of the slab"""
        return self.encoders[k].obs_elems if (traj_T or view.is_contiguous()) else view.stride(0)

    def forward_heads(self, obs, n: int, *, sample_stride: int = 0, index=None, offset: int = 0, traj_T: int = 0, tag="inf",
                      rnn=None) -> List[torch.Tensor]:
        """obs: {key: view}; returns the trunk's layer outputs (last = heads [n, heads_ld])"""
        cat = self._buf((tag, "features"), (n, self.F))
        obs = self._keyed(obs)
        for k in self.obs_keys:
            e, v = self.encoders[k], obs[k]
            out = e.forward_heads(v, n, sample_stride=self._stride_of(k, v, traj_T), index=index, offset=offset,
                                  traj_T=traj_T, tag=tag)[-1]
            c = self.col0[k]
            if e.out_chw is None:
                lib.copy_rows(cat[:, c:c + e.feat], out.view(n, e.feat))
            else:  # conv output [n][pixel][channel] -> the reference's [channel][pixel] feature order (a torch copy kernel)
                C, HW = e.out_chw[0], e.out_chw[1] * e.out_chw[2]
                lib.recording_unsafe("feature re-ordering of a conv-last encoder is a torch op")
                cat[:, c:c + e.feat].unflatten(1, (C, HW)).copy_(out.view(n, HW, C).transpose(1, 2))
        return self.trunk.forward_heads(cat, n, sample_stride=self.F, tag=tag, rnn=rnn)

    def backward(self, acts, g_heads: torch.Tensor, obs, n: int, *, sample_stride: int = 0, index=None, offset: int = 0,
                 traj_T: int = 0, on_layer_done=None) -> None:
        t = self.trunk
        t.backward(acts, g_heads, None, n, sample_stride=self.F)
        gin = t.g_input  # [n, F]
        obs = self._keyed(obs)
        for k in self.obs_keys:
            e, v, c = self.encoders[k], obs[k], self.col0[k]
            g = e._buf(("g", "out"), (n, e.feat))
            if e.out_chw is None:
                lib.copy_rows(g, gin[:, c:c + e.feat])
            else:
                C, HW = e.out_chw[0], e.out_chw[1] * e.out_chw[2]
                g.view(n, HW, C).copy_(gin[:, c:c + e.feat].unflatten(1, (C, HW)).transpose(1, 2))
            e.backward(None, g, v, n, sample_stride=self._stride_of(k, v, traj_T), index=index, offset=offset, traj_T=traj_T)
