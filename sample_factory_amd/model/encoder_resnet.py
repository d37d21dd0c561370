"""The resnet_impala image encoder on the native kernels (reference: ResnetEncoder, sample_factory/model/encoder.py:153-221):
three stages of Conv2d(3x3, padding 1) -> MaxPool2d(3, 2, 1) -> two residual blocks x + conv(act(conv(act(x)))), with
16 / 32 / 32 channels, then act, the flatten in the reference's C*H*W order and cfg.encoder_conv_mlp_layers.

`ResnetImpalaTower` is an encoder tower of model/actor_critic_multikey.py (the same surface as `ActorCritic(part="encoder")`):
its forward ends at the encoder output, its backward starts from d(loss) / d(pre-activation of that output), which is the
trunk's `g_input`.  The 3x3 convs, the pools and their gradients are csrc/sf_resnet.hip; the fully connected layers are
the library's implicit-GEMM kernels as 1x1 layers, the first one with the `linear_after_conv` weight permutation (NHWC
flatten here, NCHW in the reference).  Every launch of the forward is a C-ABI call, so rollout steps replay as launch
programs."""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch

from sample_factory_amd import lib
from sample_factory_amd.model import actor_critic as _ac
from sample_factory_amd.model.actor_critic import ACT_KIND, NativeTower, _Layer, _linear_desc, _pad

RESNET_STAGES = ((16, 2), (32, 2), (32, 2))  # encoder.py:180-182 (configuration from the IMPALA paper)


def uses_resnet(cfg, obs_space) -> bool:
    """does this model have an image key whose encoder is resnet_impala?"""
    if cfg.encoder_conv_architecture != "resnet_impala":
        return False
    leaves = obs_space.spaces if hasattr(obs_space, "spaces") else {"obs": obs_space}
    return any(len(sp.shape) == 3 for k, sp in leaves.items() if k != "action_mask")


class _Conv3:
    """one Conv2d(Cin, Cout, 3, stride=1, padding=1): weights K-major [9*Cin, Cout], k = (kh*3 + kw)*Cin + c"""

    def __init__(self, name: str, cin: int, cout: int, h: int, w: int, act_in: int, u8: bool = False,
                 sub_mean: float = 0.0, inv_scale: float = 1.0):
        self.wname, self.bname = name + ".weight", name + ".bias"
        self.Cin, self.N, self.H, self.W = cin, cout, h, w
        self.K = 9 * cin
        self.ref_w_shape = (cout, cin, 3, 3)
        self.desc = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=int(u8), act_in=act_in, traj_T=0,
                                    sub_mean=sub_mean, inv_scale=inv_scale)

    def w_from_ref(self, w_ref: torch.Tensor) -> torch.Tensor:
        return w_ref.permute(2, 3, 1, 0).reshape(self.K, self.N).contiguous()

    def w_to_ref(self, w: torch.Tensor) -> torch.Tensor:
        return w.reshape(3, 3, self.Cin, self.N).permute(3, 2, 0, 1).contiguous()


class ResnetImpalaTower(NativeTower):
    """encoder tower of observation key `obs_key` (an image, u8 CHW) for cfg.encoder_conv_architecture = resnet_impala"""

    def __init__(self, cfg, obs_space, action_space, device="cuda", all_reduce=None, obs_key: str = "obs"):
        self.cfg, self.obs_key = cfg, obs_key
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("the native resnet_impala encoder runs on the GPU only")
        if cfg.nonlinearity not in ACT_KIND:
            raise NotImplementedError(f"Unknown nonlinearity {cfg.nonlinearity}")
        space = obs_space[obs_key]
        self.obs_shape = tuple(space.shape)
        self.obs_u8 = np.dtype(space.dtype) == np.uint8
        if len(self.obs_shape) != 3 or not self.obs_u8:
            raise NotImplementedError("resnet_impala tower: uint8 CHW image observations only")
        C, H, W = self.obs_shape
        if C > 32:
            raise NotImplementedError(f"resnet_impala tower: at most 32 input channels, got {C}")
        self.obs_elems = int(np.prod(self.obs_shape))
        self.training = True
        act = self.act_kind = ACT_KIND[cfg.nonlinearity]
        keys_ = getattr(cfg, "normalize_input_keys", None)
        norm_input = bool(cfg.normalize_input) and (not keys_ or obs_key in keys_)
        sub_mean = float(cfg.obs_subtract_mean)
        inv_scale = float(np.float32(1.0 / cfg.obs_scale)) if abs(cfg.obs_scale - 1.0) > 1e-5 else 1.0
        if abs(sub_mean) <= 1e-5:
            sub_mean = 0.0
        if obs_key != "obs":  # normalize.py:38-47: mean shift / scale belong to the key named "obs" only
            sub_mean, inv_scale = 0.0, 1.0
        # ---- layers in the reference's registration order: conv_head.<i> (conv, pool, blocks per stage), mlp_layers.<j>
        pfx = f"encoder.encoders.{obs_key}."
        self.stages = []  # (stage conv, [(conv1, conv2) per block], (H, W) before the pool, (OH, OW) after)
        self.convs: List[_Conv3] = []
        # normalize_input: the first conv stays the raw-frame layer and normalises in its loader (sf_res_conv_fwd_norm /
        # sf_res_conv_wgrad_norm); only with SF_CONV1_NORM=0 it reads on.apply's f32 NHWC batch
        self._fused_norm = norm_input and _ac._CONV1_NORM
        cin, h, w, i = C, H, W, 0
        for cout, blocks in RESNET_STAGES:
            first = i == 0 and (not norm_input or self._fused_norm)
            conv = _Conv3(f"{pfx}conv_head.{i}", cin, cout, h, w, 0, u8=first, sub_mean=sub_mean if first else 0.0,
                          inv_scale=inv_scale if first else 1.0)
            oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            i += 2
            blk = []
            for _ in range(blocks):
                c1 = _Conv3(f"{pfx}conv_head.{i}.res_block_core.1", cout, cout, oh, ow, act)
                c2 = _Conv3(f"{pfx}conv_head.{i}.res_block_core.3", cout, cout, oh, ow, act)
                blk.append((c1, c2))
                i += 1
            self.stages.append((conv, blk, (h, w), (oh, ow)))
            self.convs += [conv] + [c for b in blk for c in b]
            cin, h, w = cout, oh, ow
        self.conv_out_chw = (cin, h, w)
        feat = cin * h * w
        self.fcs: List[_Layer] = []
        for j, size in enumerate(cfg.encoder_conv_mlp_layers):
            self.fcs.append(_Layer(f"{pfx}mlp_layers.{2 * j}", _linear_desc(feat, size, act), (size, feat),
                                   "linear_after_conv" if j == 0 else "linear", first_fc_chw=self.conv_out_chw))
            feat = size
        self.feat = feat
        # no fully connected layer: the output is act(last stage) NHWC, the composite re-orders it into C*H*W columns
        self.out_chw = None if self.fcs else self.conv_out_chw
        self.params = self.convs + self.fcs
        off = 0
        self._segs = []
        for L in self.params:
            self._segs.append((off, off + _pad(L.K * L.N)))
            off = self._segs[-1][1] + _pad(L.N)
        self.num_flat = off
        self.obs_normalizer = None
        if norm_input:
            from sample_factory_amd.utils.normalize import ObservationNormalizer
            self.obs_normalizer = ObservationNormalizer(cfg, self.obs_shape, self.obs_u8, self.device,
                                                        all_reduce=all_reduce, world=getattr(cfg, "dp_world", 1))
            if obs_key != "obs":
                self.obs_normalizer.sub_mean, self.obs_normalizer.inv_scale = 0.0, 1.0
        self._init_scratch()
        self._ctx: Dict = {}
        self.seat_flat(torch.zeros(off, dtype=torch.float32, device=self.device),
                       torch.zeros(off, dtype=torch.float32, device=self.device),
                       torch.zeros(off, dtype=torch.float32, device=self.device))
        self.initialize_weights()

    # ------------------------------------------------------------------------------------------ parameters
    def seat_flat(self, flat_params: torch.Tensor, flat_grads: torch.Tensor, flat_params_t: torch.Tensor) -> None:
        """(re)build every layer's views on the given flat buffers [num_flat]; current values are carried over"""
        old = getattr(self, "flat_params", None)
        if old is not None:
            flat_params.copy_(old)
        self.flat_params, self.flat_grads, self.flat_params_t = flat_params, flat_grads, flat_params_t
        self._layout_gen += 1
        for L, (o, ob) in zip(self.params, self._segs):
            L.w = flat_params[o:o + L.K * L.N].view(L.K, L.N)
            L.b = flat_params[ob:ob + L.N]
            L.gw = flat_grads[o:o + L.K * L.N].view(L.K, L.N)
            L.gb = flat_grads[ob:ob + L.N]

    def num_params(self) -> int:
        return sum(L.K * L.N + L.N for L in self.params)

    def ref_param_shapes(self):
        out = []
        for L in self.params:
            out += [(L.wname, tuple(L.ref_w_shape)), (L.bname, (L.N,))]
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = self.normalizer_state()
        for L in self.params:
            sd[L.wname] = L.w_to_ref(L.w.detach()).cpu()
            sd[L.bname] = L.b.detach().cpu().clone()
        return sd

    def load_state_dict(self, sd, strict=True):
        with torch.no_grad():
            for L in self.params:
                L.w.copy_(L.w_from_ref(torch.as_tensor(sd[L.wname], dtype=torch.float32)))
                L.b.copy_(torch.as_tensor(sd[L.bname], dtype=torch.float32))
        self.params_changed()
        self.load_normalizer_state(sd)

    def flat_to_ref(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for L, (o, ob) in zip(self.params, self._segs):
            out[L.wname] = L.w_to_ref(flat[o:o + L.K * L.N].view(L.K, L.N)).cpu()
            out[L.bname] = flat[ob:ob + L.N].cpu().clone()
        return out

    def tensor_segment_ids(self):
        seg = torch.full((self.num_flat,), 255, dtype=torch.uint8)
        for i, (L, (o, ob)) in enumerate(zip(self.params, self._segs)):
            seg[o:o + L.K * L.N] = 2 * i
            seg[ob:ob + L.N] = 2 * i + 1
        return seg.to(self.device), 2 * len(self.params)

    def params_changed(self) -> None:
        """nothing derived from the parameters is cached (no transposed weight copies)"""

    def train(self, mode=True):
        self.training = mode
        return self

    # ------------------------------------------------------------------------------------------ weight snapshots
    def enable_weight_snapshots(self) -> None:
        self._snap = [self.flat_params.clone(), self.flat_params.clone()]
        self.snap_read = 0
        self._layout_gen += 1
        on = self.obs_normalizer
        self._snap_tabs = [(on.mu_tab.clone(), on.rstd_tab.clone()) for _ in range(2)] if on is not None else None

    def publish_weights(self, slot: int) -> None:
        self._snap[slot].copy_(self.flat_params)
        if self._snap_tabs is not None:
            self._snap_tabs[slot][0].copy_(self.obs_normalizer.mu_tab)
            self._snap_tabs[slot][1].copy_(self.obs_normalizer.rstd_tab)

    def _wb(self, li: int, tag: str):
        """weights / bias of parameter layer li: the published snapshot for an async rollout, else the live buffer"""
        L = self.params[li]
        if tag.startswith("inf") and self._snap is not None:
            o, ob = self._segs[li]
            buf = self._snap[self.snap_read]
            return buf[o:o + L.K * L.N].view(L.K, L.N), buf[ob:ob + L.N]
        return L.w, L.b

    # ------------------------------------------------------------------------------------------ forward / backward
    def forward_heads(self, obs: torch.Tensor, n: int, *, sample_stride: int, index=None, offset: int = 0,
                      traj_T: int = 0, tag="inf", rnn=None) -> List[torch.Tensor]:
        """encoder forward on n samples (addressing as ActorCritic.forward_heads); the last entry is the output [n, feat]
        (an fc layer's activated output, or act(last stage) NHWC when there is none)"""
        self._tls.role = "rollout" + tag[3:] if tag.startswith("inf") else "learner"
        act = self.act_kind
        x, stride, idx, off, tT = obs, sample_stride, index, offset, traj_T
        norm_tabs = None
        if self.obs_normalizer is not None:  # normalize_input=True
            on = self.obs_normalizer
            tabs = self._snap_tabs[self.snap_read] if (tag.startswith("inf") and self._snap is not None) else None
            if self._fused_norm:  # in the first conv's loader: the frames stay u8 in the slab, no f32 copy is written
                norm_tabs = tabs if tabs is not None else (on.mu_tab, on.rstd_tab)
            else:  # SF_CONV1_NORM=0: the normalised f32 NHWC batch (utils/normalize.py)
                xn = self._buf((tag, "obsn"), (n, self.obs_elems))
                on.apply(obs, sample_stride, n, xn, index=index, offset=offset, traj_T=traj_T, tabs=tabs)
                x, stride, idx, off, tT = xn, self.obs_elems, None, 0, 0
        first_in = (x, stride, idx, off, tT)
        saved = []  # per stage: (stage input, conv output, pooled, pool argmax, [(block input, t, y)])
        li = 0
        last_stage = len(self.stages) - 1
        y_act = None
        for s, (conv, blk, (h, w), (oh, ow)) in enumerate(self.stages):
            d = conv.desc
            if tT:
                d = lib.sf_res_desc.from_buffer_copy(conv.desc)
                d.traj_T = int(tT)
            wt, bs = self._wb(li, tag)
            full = self._buf((tag, "s", s, "conv"), (n, h, w, conv.N))
            if s == 0 and norm_tabs is not None:
                lib.res_conv_fwd_norm(x, stride, idx, off, norm_tabs[0], norm_tabs[1], wt, bs, full, n, d)
            else:
                lib.res_conv_fwd(x, stride, idx, off, wt, bs, full, n, d)
            li += 1
            pooled = self._buf((tag, "s", s, "pool"), (n, oh, ow, conv.N))
            arg = self._buf((tag, "s", s, "arg"), (n, oh, ow, conv.N), dtype=torch.uint8)
            lib.res_pool_fwd(full, pooled, arg, n, h, w, conv.N)
            stage_in = (x, stride, idx, off, tT)
            xb = pooled
            bl = []
            for b, (c1, c2) in enumerate(blk):
                t = self._buf((tag, "s", s, "b", b, "t"), (n, oh, ow, c1.N))
                w1, b1 = self._wb(li, tag)
                lib.res_conv_fwd(xb, oh * ow * c1.Cin, None, 0, w1, b1, t, n, c1.desc)
                y = self._buf((tag, "s", s, "b", b, "y"), (n, oh, ow, c2.N))
                w2, b2 = self._wb(li + 1, tag)
                if s == last_stage and b == len(blk) - 1:  # encoder.py:205: act after the last stage, from this epilogue
                    y_act = self._buf((tag, "y_act"), (n, oh, ow, c2.N))
                    lib.res_conv_fwd(t, oh * ow * c2.Cin, None, 0, w2, b2, y, n, c2.desc, residual=xb, out_act=y_act,
                                     act_out=act)
                else:
                    lib.res_conv_fwd(t, oh * ow * c2.Cin, None, 0, w2, b2, y, n, c2.desc, residual=xb)
                li += 2
                bl.append((xb, t, y))
                xb = y
            saved.append((stage_in, full, pooled, arg, bl))
            x, stride, idx, off, tT = xb, oh * ow * conv.N, None, 0, 0
        acts = [y_act]
        xin = y_act
        for j, L in enumerate(self.fcs):
            out = self._buf((tag, "fc", j), (n, L.N))
            wt, bs = self._wb(li + j, tag)
            wsb = lib.conv_fwd_workspace(n, L.desc)
            lib.conv_fwd_raw(xin, L.K, None, 0, wt, bs, out, n, L.desc, self._workspace(wsb) if wsb else None)
            acts.append(out)
            xin = out
        self._ctx[tag] = dict(first_in=first_in, saved=saved, acts=acts, norm_tabs=norm_tabs)
        return acts

    def backward(self, acts, g_out: torch.Tensor, obs, n: int, *, sample_stride: int = 0, index=None, offset: int = 0,
                 traj_T: int = 0) -> None:
        """d(loss) / d(pre-activation of the output) [n, feat] of the last "train" forward -> this tower's flat_grads"""
        ctx = self._ctx["train"]
        self._tls.role = "learner"
        act, acts = self.act_kind, ctx["acts"]
        g = g_out
        for j in range(len(self.fcs) - 1, -1, -1):
            L, xin = self.fcs[j], acts[j]  # xin: the activated input of fc layer j (act(last stage) for j = 0)
            lib.conv_wgrad_raw(xin, L.K, None, 0, g, L.gw, L.gb, n, L.desc,
                               self._workspace(lib.conv_wgrad_workspace(n, L.desc)))
            gin = self._buf(("g", "fc", j), (n, L.K))
            dd = lib.sf_conv_desc.from_buffer_copy(L.desc)
            dd.relu = act  # derivative of the activation that produced xin, through the stored output
            lib.conv_dgrad(g, L.w, xin, gin, n, dd)
            g = gin
        # g: d(loss) / d(output of the last residual block), NHWC
        for s in range(len(self.stages) - 1, -1, -1):
            conv, blk, (h, w), (oh, ow) = self.stages[s]
            stage_in, full, pooled, arg, bl = ctx["saved"][s]
            for b in range(len(blk) - 1, -1, -1):
                c1, c2 = blk[b]
                xb, t, _ = bl[b]
                ws = self._workspace(lib.res_conv_wgrad_workspace(n, c2.desc))
                lib.res_conv_wgrad(t, oh * ow * c2.Cin, None, 0, g, c2.gw, c2.gb, n, c2.desc, ws)
                g_t = self._buf(("g", "s", s, "b", b, "t"), (n, oh, ow, c1.N))
                lib.res_conv_dgrad(g, c2.w, t, g_t, n, c2.desc)  # * act'(t)
                lib.res_conv_wgrad(xb, oh * ow * c1.Cin, None, 0, g_t, c1.gw, c1.gb, n, c1.desc, ws)
                g_x = self._buf(("g", "s", s, "b", b, "x"), (n, oh, ow, c1.Cin))
                lib.res_conv_dgrad(g_t, c1.w, xb, g_x, n, c1.desc, g_add=g)  # g_y + dgrad * act'(x): the skip
                g = g_x
            g_full = self._buf(("g", "s", s, "full"), (n, h, w, conv.N))
            lib.res_pool_bwd(g, arg, g_full, n, h, w, conv.N)
            x, stride, idx, off, tT = stage_in
            d = conv.desc
            if tT:
                d = lib.sf_res_desc.from_buffer_copy(conv.desc)
                d.traj_T = int(tT)
            ws = self._workspace(lib.res_conv_wgrad_workspace(n, d))
            if s == 0 and ctx.get("norm_tabs") is not None:  # the forward normalised in the loader: so does the gradient
                mu_, rstd_ = ctx["norm_tabs"]
                lib.res_conv_wgrad_norm(x, stride, idx, off, mu_, rstd_, g_full, conv.gw, conv.gb, n, d, ws)
            else:
                lib.res_conv_wgrad(x, stride, idx, off, g_full, conv.gw, conv.gb, n, d, ws)
            if s > 0:
                g_in = self._buf(("g", "s", s, "in"), (n, h, w, conv.Cin))
                lib.res_conv_dgrad(g_full, conv.w, None, g_in, n, conv.desc)
                g = g_in
