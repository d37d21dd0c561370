"""cfg.actor_critic_share_weights=False on the NATIVE kernels (reference: ActorCriticSeparateWeights,
sample_factory/model/actor_critic.py:198-334): the actor and the critic own an encoder, a recurrent core and a decoder each;
`critic_linear` reads the critic's features, `action_parameterization.distribution_linear` the actor's; the recurrent state of a
sample is [actor state | critic state] (model_utils.py:20-22 doubles its width).

A tower composite (model/composite.py) on [actor | critic]: two `ActorCritic` towers (model/actor_critic.py), or two
`MultiKeyActorCritic` towers for observation dicts with several keys.  Every tower keeps the fused heads GEMM
[features, 1 + A]; the columns a tower does not own (the value column in the actor, the action columns in the critic) have
zero weights, zero bias and — because each tower's backward pass receives the loss gradient with the other tower's columns
zeroed — zero gradients: they never move.  The network kernels, the fused sequence passes and the rollout's one-step path are
the towers' own; this class only splits states / gradients and merges heads.  Parameter names and order are the reference's (actor_encoder.*, actor_core.*, critic_encoder.*, critic_core.*,
actor_decoder.*, critic_decoder.*, critic_linear.*, action_parameterization.*)."""
from __future__ import annotations

import copy
from typing import Dict, List, Optional

import torch

from sample_factory_amd import lib
from sample_factory_amd.model.actor_critic import ActorCritic, get_rnn_size
from sample_factory_amd.model.composite import TowerComposite

_PARTS = ("encoder.", "core.", "decoder.")
_WHO = ("actor", "critic")  # the towers, in the order of the flat buffer


class SeparateActorCritic(TowerComposite):
    _buf_prefix = "sep"

    def __init__(self, cfg, obs_space, action_space, device="cuda", all_reduce=None):
        self.cfg = cfg
        tcfg = copy.copy(cfg)
        tcfg.actor_critic_share_weights = True  # a tower is the shared-weights architecture
        keys = [k for k in obs_space.spaces.keys() if k != "action_mask"]
        if len(keys) > 1:  # observation dicts with several keys: each tower is the multi-key composite (encoder towers + trunk)
            from sample_factory_amd.model.actor_critic_multikey import MultiKeyActorCritic as Tower
        else:
            Tower = ActorCritic
        self.actor = Tower(tcfg, obs_space, action_space, device, all_reduce=all_reduce)
        self.critic = Tower(tcfg, obs_space, action_space, device, all_reduce=all_reduce)
        a, c = self.actor, self.critic
        self.multi_key, self.obs_keys = bool(getattr(a, "multi_key", False)), list(getattr(a, "obs_keys", ["obs"]))
        self.device, self.obs_space, self.action_space = a.device, obs_space, action_space
        self.obs_shape, self.obs_elems, self.obs_u8 = a.obs_shape, a.obs_elems, a.obs_u8
        self.num_action_params, self.heads_ld = a.num_action_params, a.heads_ld
        self.rnn_kind, self.rnn_H = a.rnn_kind, a.rnn_H
        self.rnn_S = get_rnn_size(cfg)
        assert self.rnn_S == a.rnn_S + c.rnn_S
        self._seat_towers([a, c], lead=a)
        # ---- shared: input / return normalisers (actor_critic.py:44-61: they belong to the model, not to a tower), the
        # fused sequence passes' sync words (one sticky abort word for the optimiser's skip flag)
        c.share_normalizers_from(a)
        self.obs_normalizer, self.returns_normalizer = a.obs_normalizer, a.returns_normalizer
        if self.rnn_kind is not None:
            c.share_seq_sync_from(a)
        self._zero_foreign_columns()

    # ------------------------------------------------------------------------------------------ heads bookkeeping
    def _zero_foreign_columns(self) -> None:
        """the value column of the actor's heads and the action columns of the critic's: not parameters of the model"""
        with torch.no_grad():
            Ha, Hc = self.actor.heads_layer, self.critic.heads_layer
            Ha.w[:, 0].zero_()
            Ha.b[0].zero_()
            Hc.w[:, 1:].zero_()
            Hc.b[1:].zero_()
        self.params_changed()

    # ------------------------------------------------------------------------------------------ reference surface
    def num_params(self) -> int:
        return sum(int(torch.Size(s).numel()) for _, s in self.ref_param_shapes())

    @staticmethod
    def _rename(name: str, who: str) -> Optional[str]:
        for p in _PARTS:
            if name.startswith(p):
                return f"{who}_{name}"
        if name.startswith("critic_linear."):
            return name if who == "critic" else None
        if name.startswith("action_parameterization."):
            return name if who == "actor" else None
        return None  # normaliser statistics: handled once, by the model

    def ref_param_shapes(self):
        """(name, shape) in the reference's registration order (actor_critic.py:206-226): actor encoder, actor core, critic
        encoder, critic core, actor decoder, critic decoder, critic_linear, action_parameterization"""
        by = {}
        for who, t in zip(_WHO, self.towers):
            for n, shp in t.ref_param_shapes():
                r = self._rename(n, who)
                if r is not None:
                    by.setdefault((who, n.split(".")[0]), []).append((r, shp))
        order = [("actor", "encoder"), ("actor", "core"), ("critic", "encoder"), ("critic", "core"), ("actor", "decoder"),
                 ("critic", "decoder"), ("critic", "critic_linear"), ("actor", "action_parameterization")]
        return [x for k in order for x in by.get(k, [])]

    def _split_sd(self, sd: Dict, who: str) -> Dict:
        out = {}
        for k, v in sd.items():
            r = self._rename(k, who)
            if r is not None:
                out[r] = v
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = dict(self.actor.normalizer_state())
        if self.returns_normalizer is not None:
            sd.update(self.returns_normalizer.state_dict("returns_normalizer."))
        parts = {who: self._split_sd(t.state_dict(), who) for who, t in zip(_WHO, self.towers)}
        for name, _ in self.ref_param_shapes():
            sd[name] = parts["actor" if name in parts["actor"] else "critic"][name]
        return sd

    def load_state_dict(self, sd, strict=True):
        for who, t in zip(_WHO, self.towers):
            own = t.state_dict()  # the tower's own names; foreign heads entries keep their (zero) values
            for k in list(own):
                r = self._rename(k, who)
                if r is not None:
                    if r in sd:
                        own[k] = sd[r]
                    elif strict:
                        raise KeyError(r)
            for k in [k_ for k_ in own if k_.startswith(("obs_normalizer.", "returns_normalizer."))]:
                del own[k]
            t.load_state_dict(own, strict=False)
        self._zero_foreign_columns()
        self.actor.load_normalizer_state(sd)
        if self.returns_normalizer is not None and "returns_normalizer.running_mean" in sd:
            self.returns_normalizer.load_state_dict(sd, "returns_normalizer.")
        elif strict and self.returns_normalizer is not None:
            raise KeyError("returns_normalizer.* missing from state dict")

    def flat_to_ref(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for who, tw, part in zip(_WHO, self.towers, self._slices(flat)):
            out.update(self._split_sd(tw.flat_to_ref(part), who))
        return {n: out[n] for n, _ in self.ref_param_shapes()}

    def _tower_segment_ids(self, i: int):
        """the heads tensors a tower does not own (critic_linear in the actor, the action parameterisation in the critic)
        count as padding"""
        s, n = self.towers[i].tensor_segment_ids()
        s = s.clone()
        h = n - 4 - (1 if self.actor.nonadaptive_std else 0)  # first heads id: critic w, critic b, dist w, dist b [, stddev]
        if i == 0:
            s[(s == h) | (s == h + 1)] = 255
        else:
            s[(s >= h + 2) & (s != 255)] = 255
        return s, n

    # ------------------------------------------------------------------------------------------ compute plumbing
    def enable_weight_snapshots(self) -> None:
        super().enable_weight_snapshots()
        # one normaliser (per key), one pair of published tables (copied by both towers' publish_weights: the same few KB
        # twice, stream-ordered)
        self.critic.share_snapshot_tables_from(self.actor)

    # ------------------------------------------------------------------------------------------ forward / backward
    def _rnn_of(self, rnn, which: int):
        """a tower's half of the recurrent inputs: state rows / chunk-start states are [actor | critic] column-wise"""
        if rnn is None:
            return None
        half = self.actor.rnn_S
        sl = slice(which * half, (which + 1) * half)
        out = dict(rnn)
        if "states" in rnn:
            out["states"] = rnn["states"][:, sl]
        if "h0" in rnn:
            out["h0"] = rnn["h0"][:, sl]
        return out

    def forward_heads(self, obs, n: int, *, sample_stride: int, index=None, offset: int = 0, traj_T: int = 0, tag="inf",
                      rnn=None) -> List[torch.Tensor]:
        """both towers on the same observations; returns [heads [n, heads_ld]]: column 0 from the critic, the action
        parameters from the actor"""
        ha = self.actor.forward_heads(obs, n, sample_stride=sample_stride, index=index, offset=offset, traj_T=traj_T, tag=tag,
                                      rnn=self._rnn_of(rnn if self.rnn_kind is not None else None, 0))[-1]
        hc = self.critic.forward_heads(obs, n, sample_stride=sample_stride, index=index, offset=offset, traj_T=traj_T, tag=tag,
                                       rnn=self._rnn_of(rnn if self.rnn_kind is not None else None, 1))[-1]
        out = self._buf((tag, "heads"), (n, self.heads_ld))
        lib.copy_rows(out, ha)                    # (library launches, not torch ops: a rollout step of this model is
        lib.copy_rows(out[:, 0:1], hc[:, 0:1])    #  recordable as a launch program, lib.LaunchProgram)
        return [out]

    def backward(self, acts, g_heads: torch.Tensor, obs, n: int, *, sample_stride: int, index=None, offset: int = 0,
                 traj_T: int = 0, on_layer_done=None) -> None:
        """d(loss)/d(heads) split by owner: the actor tower sees the action columns, the critic tower the value column"""
        ga = self._buf(("g", "heads_actor"), (n, self.heads_ld))
        gc = self._zbuf(("g", "heads_critic"), (n, self.heads_ld))
        ga.copy_(g_heads)
        ga[:, 0].zero_()
        gc[:, 0].copy_(g_heads[:, 0])
        self.actor.backward(None, ga, obs, n, sample_stride=sample_stride, index=index, offset=offset, traj_T=traj_T)
        self.critic.backward(None, gc, obs, n, sample_stride=sample_stride, index=index, offset=offset, traj_T=traj_T)

    def new_rnn_parts_of(self, tag: str = "inf"):
        pa, pc = self.actor.new_rnn_parts_of(tag), self.critic.new_rnn_parts_of(tag)
        return None if pa is None or pc is None else list(pa) + list(pc)

    def new_rnn_states_of(self, tag: str = "inf") -> torch.Tensor:
        return torch.cat([self.actor.new_rnn_states_of(tag), self.critic.new_rnn_states_of(tag)], dim=1)

    def _dense_obs(self, normalized_obs_dict):
        if self.multi_key:
            return super()._dense_obs(normalized_obs_dict)
        obs = normalized_obs_dict["obs"] if isinstance(normalized_obs_dict, dict) else normalized_obs_dict
        return obs, obs.shape[0], (self.obs_elems if obs.is_contiguous() else obs.stride(0))
