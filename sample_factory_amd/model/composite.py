"""Native models composed of several towers on ONE flat parameter / gradient buffer, so that clip + Adam / Lamb, the
gradient exchange, checkpoints and the weight snapshots of async mode see a single parameter vector, as for the single-key
model.  `SeparateActorCritic` (model/actor_critic_separate.py) and `MultiKeyActorCritic` (model/actor_critic_multikey.py)
are the two composites; a multi-key composite is itself the tower of a separate-weights one."""
from __future__ import annotations

from typing import List

import torch

from sample_factory_amd.model.actor_critic import NativeModel


class TowerComposite(NativeModel):
    """The tower protocol.  A tower — `ActorCritic`, `ResnetImpalaTower` or a `TowerComposite` — provides:

     * `num_flat` and `seat_flat(flat_params, flat_grads, flat_params_t)`: (re)build its views on slices of the
       composite's buffers, carrying its current values over;
     * `tensor_segment_ids()`, `flat_to_ref(flat)`, `ref_param_shapes()`, `state_dict()`, `load_state_dict(sd, strict)`;
     * `train(mode)`, `params_changed()`, `launch_key(tag)`, `snap_read`, `enable_weight_snapshots()`,
       `publish_weights(slot)`, `_buf` / `_zbuf`, `rnn_abort_word()` / `rnn_abort_clear()` / `rnn_pass_aborted()`,
       `new_rnn_parts_of(tag)` / `new_rnn_states_of(tag)`;
     * `forward_heads(obs, n, ...)` (its layer outputs, the last one its output) and `backward(acts, g, obs, n, ...)`.

    The towers of a separate-weights composite also provide `heads_layer`, `share_normalizers_from`,
    `share_seq_sync_from`, `share_snapshot_tables_from`, `normalizer_state()` and `load_normalizer_state(sd)`.

    This class implements the first three groups for a composite by delegating to its towers: to all of them, or to the
    `lead` tower, which owns the composite's scratch buffers (under the key prefix `_buf_prefix`), its snapshot read index
    and the sticky abort word of the fused recurrent passes.  A subclass builds its towers, then calls
    `_seat_towers(towers, lead)`, and provides `forward_heads`, `backward` and the reference's parameter names."""

    _buf_prefix: str

    def _seat_towers(self, towers: List, lead) -> None:
        """allocate the flat buffers [tower 0 | tower 1 | ...] and seat every tower on its slice"""
        self.towers, self.lead = list(towers), lead
        self._base, off = [], 0
        for tw in self.towers:
            self._base.append(off)
            off += tw.num_flat
        self.num_flat = off
        self.training = True
        self._snap = None
        flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.seat_flat(flat, torch.zeros_like(flat), torch.zeros_like(flat))

    def _slices(self, flat: torch.Tensor) -> List[torch.Tensor]:
        return [flat[o:o + tw.num_flat] for tw, o in zip(self.towers, self._base)]

    def seat_flat(self, flat_params: torch.Tensor, flat_grads: torch.Tensor, flat_params_t: torch.Tensor) -> None:
        for tw, p, g, t in zip(self.towers, self._slices(flat_params), self._slices(flat_grads),
                               self._slices(flat_params_t)):
            tw.seat_flat(p, g, t)  # (every tower carries its current values over)
        self.flat_params, self.flat_grads, self.flat_params_t = flat_params, flat_grads, flat_params_t

    # ------------------------------------------------------------------------------------------ reference surface
    def flat_to_ref(self, flat: torch.Tensor):
        out = {}
        for tw, part in zip(self.towers, self._slices(flat)):
            out.update(tw.flat_to_ref(part))
        return out

    def _tower_segment_ids(self, i: int):
        return self.towers[i].tensor_segment_ids()

    def tensor_segment_ids(self):
        """Lamb's per-tensor statistics (optimizers.py:108-135): the towers' maps side by side"""
        segs, base = [], 0
        for i in range(len(self.towers)):
            s, n = self._tower_segment_ids(i)
            segs.append(torch.where(s == 255, s, s + base))
            base += n
        if base > 64:
            raise NotImplementedError("Lamb with more than 64 parameter tensors")
        return torch.cat(segs), base

    def train(self, mode=True):
        self.training = mode
        for tw in self.towers:
            tw.train(mode)
        return self

    # ------------------------------------------------------------------------------------------ compute plumbing
    def params_changed(self) -> None:
        for tw in self.towers:
            tw.params_changed()

    def _buf(self, key, shape, dtype=torch.float32):
        return self.lead._buf((self._buf_prefix,) + tuple(key), shape, dtype)

    def _zbuf(self, key, shape):
        return self.lead._zbuf((self._buf_prefix,) + tuple(key), shape)

    def launch_key(self, tag: str = "inf"):
        """(the towers' buffer layouts, the snapshot read index)"""
        keys = [tw.launch_key(tag) for tw in self.towers]
        return tuple(k[0] for k in keys), keys[0][1]

    @property
    def snap_read(self):
        return self.lead.snap_read

    @snap_read.setter
    def snap_read(self, v):
        for tw in self.towers:
            tw.snap_read = v

    def enable_weight_snapshots(self) -> None:
        for tw in self.towers:
            tw.enable_weight_snapshots()
        self._snap = True

    def publish_weights(self, slot: int) -> None:
        for tw in self.towers:
            tw.publish_weights(slot)

    def rnn_abort_word(self):
        return self.lead.rnn_abort_word()

    def rnn_abort_clear(self) -> None:
        self.lead.rnn_abort_clear()

    def rnn_pass_aborted(self) -> bool:
        return self.lead.rnn_pass_aborted()

    def new_rnn_parts_of(self, tag: str = "inf"):
        return self.lead.new_rnn_parts_of(tag)

    def new_rnn_states_of(self, tag: str = "inf") -> torch.Tensor:
        return self.lead.new_rnn_states_of(tag)

    @property
    def new_rnn_states(self) -> torch.Tensor:
        return self.new_rnn_states_of("inf")

    # ------------------------------------------------------------------------------------------ forward
    def _dense_obs(self, normalized_obs_dict):
        """(obs, B, sample_stride) for forward_heads from dense per-key batches {key: [B, ...]}"""
        obs = {k: normalized_obs_dict[k].contiguous() for k in self.obs_keys}
        return obs, obs[self.obs_keys[0]].shape[0], 0

    def forward(self, normalized_obs_dict, rnn_states=None, values_only: bool = False, action_mask=None):
        """Inference-style forward on a dense batch (the reference's ActorCritic.forward surface)"""
        obs, B, stride = self._dense_obs(normalized_obs_dict)
        rnn = dict(states=rnn_states) if self.rnn_kind is not None else None
        heads = self.forward_heads(obs, B, sample_stride=stride, rnn=rnn)[-1]
        res = dict(values=heads[:, 0])
        if not values_only:
            res["action_logits"] = heads[:, 1:1 + self.num_action_params]
        res["new_rnn_states"] = self.new_rnn_states if self.rnn_kind is not None else rnn_states
        return res
