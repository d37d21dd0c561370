"""--encoder_resnet_bf16: the 3x3 conv family on bf16 MFMA (csrc/sf_resnet_bf16.hip) against float64 torch on operands rounded
like the kernel's, its batch independence, a width-2 tower against a torch twin with the same rounding, and one training
iteration of the engine."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_resnet import ACTS, _cfg, _nchw, _nhwc, _space, _w_native  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG, _run  # noqa: E402

BF16 = (lib.res_conv_fwd_bf16, lib.res_conv_dgrad_bf16, lib.res_conv_wgrad_bf16, lib.res_conv_wgrad_bf16_workspace)


def _bf(t):
    return t.float().bfloat16().double()


class _Bf16Conv(torch.autograd.Function):
    """3x3 same conv in float64 whose matrix operands are rounded to bf16 in every pass, as the kernels round them.  ex / eg
    (optional): the rounding errors bf16(v) - v of the numbers the device rounded as input / output gradient, added to this
    side's own values instead of rounding them again"""

    @staticmethod
    def forward(ctx, x, w, b, ex=None, eg=None):
        xr, wr = _bf(x) if ex is None else x + ex, _bf(w)
        ctx.save_for_backward(xr, wr)
        ctx.eg = eg
        return F.conv2d(xr, wr, b, padding=1)

    @staticmethod
    def backward(ctx, gy):
        xr, wr = ctx.saved_tensors
        g = _bf(gy) if ctx.eg is None else gy + ctx.eg
        return (torch.nn.grad.conv2d_input(xr.shape, wr, g, padding=1), torch.nn.grad.conv2d_weight(xr, wr.shape, g, padding=1),
                g.sum((0, 2, 3)), None, None)


def _layer(cin, cout, h, w, n, act):
    """inputs as test_gpu_resnet_wide._layer (N(0,1) data, N(0, 1/(9 Cin)) weights), drawn in float32 so that the device
    and the reference round the same numbers; the epilogue terms (bias, residual, g_add, act') stay unrounded"""
    g = torch.Generator().manual_seed(cin * 100 + h * 10 + act)
    rnd = lambda *s: torch.randn(*s, generator=g).double()  # noqa: E731
    x, wt, b = rnd(n, cin, h, w), rnd(cout, cin, 3, 3).div((9 * cin) ** 0.5).float().double(), rnd(cout)
    res, gy, gadd = rnd(n, cout, h, w), rnd(n, cout, h, w), rnd(n, cin, h, w)
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = _Bf16Conv.apply(ACTS[act](xr), wr, br)
    y.backward(gy)
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=act, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    dev = dict(x=_nhwc(x).float().cuda(), w=_w_native(wt).float().cuda(), b=b.float().cuda(), res=_nhwc(res).float().cuda(),
               gy=_nhwc(gy).float().cuda(), gadd=_nhwc(gadd).float().cuda())
    ref = dict(y=y.detach(), res=res, gx=xr.grad, gadd=gadd, gw=_w_native(wr.grad), gb=br.grad)
    return d, dev, ref


# all four activations on the two smallest inputs (tanh / ELU are evaluated in fp32 on the device and in float64 here, and
# an element whose two values straddle a bf16 rounding boundary would differ by a bf16 ulp: about 1e-5 per element)
CASES = [(64, 128, 1, 1, 5, a) for a in range(4)] + [(128, 128, 5, 4, 2, a) for a in range(4)] + [
    (32, 32, 16, 16, 1, 1), (32, 64, 7, 9, 3, 0), (64, 64, 8, 6, 2, 1), (128, 64, 3, 37, 2, 1)]


@pytest.mark.parametrize("cin,cout,h,w,n,act", CASES)
def test_bf16_conv_fwd_dgrad_wgrad(cin, cout, h, w, n, act):
    d, t, ref = _layer(cin, cout, h, w, n, act)
    o = _run(d, t, n, act, *BF16)
    np.testing.assert_allclose(_nchw(o["y"]).cpu().double(), ref["y"], **FWD)
    np.testing.assert_allclose(_nchw(o["yres"]).cpu().double(), ref["res"] + ref["y"], **FWD)
    np.testing.assert_allclose(_nchw(o["yact"]).cpu().double(), ACTS[act](ref["res"] + ref["y"]), **FWD)
    np.testing.assert_allclose(_nchw(o["gx"]).cpu().double(), ref["gx"], **FWD)
    np.testing.assert_allclose(_nchw(o["gxadd"]).cpu().double(), ref["gadd"] + ref["gx"], **FWD)
    np.testing.assert_allclose(o["gw"].cpu().double(), ref["gw"], **WG)
    np.testing.assert_allclose(o["gb"].cpu().double(), ref["gb"], **WG)


@pytest.mark.parametrize("c,h,w", [(64, 8, 6), (128, 5, 4)])
def test_bf16_forward_does_not_depend_on_the_batch(c, h, w):
    d, t, _ = _layer(c, c, h, w, 5, 3)
    full, one = torch.empty(5, h, w, c, device="cuda"), torch.empty(1, h, w, c, device="cuda")
    lib.res_conv_fwd_bf16(t["x"], h * w * c, None, 0, t["w"], t["b"], full, 5, d)
    for i in range(5):
        lib.res_conv_fwd_bf16(t["x"][i:i + 1].contiguous(), h * w * c, None, 0, t["w"], t["b"], one, 1, d)
        assert torch.equal(one[0], full[i]), i


def _device_roundings(tower, n, tag="train"):
    """conv weight name -> (ex, eg): bf16(v) - v, NCHW float64, of the input and the output gradient each bf16 layer of the
    tower rounded in its last training forward and backward, read from the tower's own activation and gradient buffers"""
    B, act, out, last = tower._bufs, ACTS[tower.act_kind], {}, len(tower.stages) - 1
    err = lambda t: _nchw((t.bfloat16().float() - t).cpu().double())  # noqa: E731
    for s, (conv, blk, _, (oh, ow)) in enumerate(tower.stages):
        if s:
            out[conv.wname] = err(B[(tag, "s", s - 1, "b", len(tower.stages[s - 1][1]) - 1, "y")]), err(B[("g", "s", s, "full")])
        for b, (c1, c2) in enumerate(blk):
            xb = B[(tag, "s", s, "pool")] if b == 0 else B[(tag, "s", s, "b", b - 1, "y")]
            g2 = (B[("g", "s", s, "b", b + 1, "x")] if b + 1 < len(blk) else
                  B[("g", "s", s + 1, "in")] if s < last else B[("g", "fc", 0)].view(n, oh, ow, c2.N))
            out[c1.wname] = err(act(xb)), err(B[("g", "s", s, "b", b, "t")])
            out[c2.wname] = err(act(B[(tag, "s", s, "b", b, "t")])), err(g2)
    return out


def test_bf16_width_2_tower_matches_its_rounding_torch_twin():
    """forward and every parameter gradient; bounds of test_wide_tower_matches_its_torch_twin; 3 x 13 x 17 reaches all stages.

    "Rounded the same way" has to mean the same rounding decisions.  A twin that rounds its own float64 values again moves
    by 5.8e-3 (heads) and 8.7e-2 (gradients) when its input is perturbed by 1e-7 relative, the size of fp32 rounding: a value
    that differs in its last bits lands on the other bf16 neighbour with probability diff / ulp, and 14 stacked layers
    amplify that towards one bf16 ulp, so such a reference's own error is above these bounds (the tower measured 3.5e-3 and
    3.9e-2 against it).  So every bf16 layer of the twin keeps its OWN float64 input and output gradient, which a wiring
    mistake in the tower would still leave different, and adds the rounding error the device made on the same element."""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic, global_model_factory
    from sample_factory_amd.model.torch_policy import build_torch_actor_critic
    cfg = _cfg("elu", encoder_conv_mlp_layers=[64], encoder_resnet_width=2, encoder_resnet_bf16=True)
    shape, A, n = (3, 13, 17), 5, 9
    ac = create_actor_critic(cfg, _space(shape), spaces.Discrete(A), torch.device("cuda"))
    assert [c.bf16 for c in ac.encoders["obs"].convs] == [False] + [True] * 14
    tm = build_torch_actor_critic(cfg, _space(shape), spaces.Discrete(A), global_model_factory()).double()
    g = torch.Generator().manual_seed(7)
    sd = {name: (torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1)).float() for name, p in tm.named_parameters()}
    ac.load_state_dict(sd, strict=True)
    tm.load_state_dict({name: v.double() for name, v in ac.state_dict().items()}, strict=False)
    obs = torch.randint(0, 256, (n,) + shape, generator=g, dtype=torch.uint8)
    rollout = ac.forward_heads({"obs": obs.cuda()}, n, tag="inf")[-1].clone()
    heads = ac.forward_heads({"obs": obs.cuda()}, n, tag="train")[-1]
    assert torch.equal(rollout, heads)  # the behaviour policy and the learner evaluate the same function
    gh = torch.randn(heads.shape, generator=g).cuda()
    gh[:, 1 + A:] = 0
    ac.backward(None, gh, {"obs": obs.cuda()}, n)
    grads = ac.flat_to_ref(ac.flat_grads)
    rnd = _device_roundings(ac.encoders["obs"], n)
    assert len(rnd) == 14
    for name, m in tm.named_modules():
        if name + ".weight" in rnd:
            m.forward = lambda x, m=m, e=rnd[name + ".weight"]: _Bf16Conv.apply(x, m.weight, m.bias, *e)
    core, _ = tm.forward_core(tm.forward_head({"obs": obs.double() / 255.0}), torch.zeros(n, 1, dtype=torch.float64))
    out = tm.forward_tail(core)
    np.testing.assert_allclose(heads[:, 0].cpu().double(), out["values"].detach(), atol=2e-4, rtol=1e-3)
    np.testing.assert_allclose(heads[:, 1:1 + A].cpu().double(), out["action_logits"].detach(), atol=2e-4, rtol=1e-3)
    ghd = gh.cpu().double()
    ((out["values"] * ghd[:, 0]).sum() + (out["action_logits"] * ghd[:, 1:1 + A]).sum()).backward()
    for name, p in tm.named_parameters():
        err = float((grads[name].double() - p.grad).abs().max()) / (float(p.grad.abs().max()) + 1e-6)
        assert err < 2e-3, f"{name}: relative error {err:.2e}"


def test_bf16_width_2_trains_under_random_shift(tmp_path):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_atari", make_synthetic_env)
    cfg, runner = make_runner(default_cfg(
        env="synthetic_atari", use_rnn=False, nonlinearity="elu", normalize_input=False, obs_scale=255.0,
        encoder_conv_architecture="resnet_impala", rollout=8, batch_size=256, num_batches_per_epoch=2, num_epochs=1,
        num_workers=1, num_envs_per_worker=1, async_rl=False, seed=0, serial_mode=True, synthetic_num_agents=64,
        exploration_loss_coeff=0.01, train_dir=str(tmp_path), experiment="bf16", encoder_resnet_width=2,
        encoder_resnet_bf16=True, augment_random_shift=2))
    runner.init()
    ac = runner.learner.actor_critic
    assert any(c.bf16 for c in ac.encoders["obs"].convs)
    p0 = ac.flat_params.clone()
    stats = runner.iteration()
    torch.cuda.synchronize()
    assert np.isfinite(stats["train"]["loss"]) and runner.learner._shift_pad == 2
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    runner.learner.save()
    with open(os.path.join(tmp_path, "bf16", "config.json")) as f:
        assert json.load(f)["encoder_resnet_bf16"] is True
