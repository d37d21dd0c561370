"""--encoder_resnet_bf16 on the 16-channel layers of the width-1 tower (csrc/sf_resnet_bf16_c16.hip): 16 -> 16 and 16 -> 32
in every pass against float64 torch on operands rounded like the kernel's, batch independence and determinism to the bit,
and the width-1 tower against a torch twin that makes the device's rounding decisions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_resnet import ACTS, _cfg, _nchw, _space  # noqa: E402
from tests.test_gpu_resnet_bf16 import BF16, _Bf16Conv, _device_roundings, _layer  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG, _run  # noqa: E402

# 1 x 1: the halo is all zeros, five samples share a tile and the odd tap is the only live one.  3 x 37: two column tiles, a
# fragment that wraps rows, a row that is no multiple of 8.  36 x 48 at n = 257: a launch has at most 1024 work-groups and
# this image is four forward / data-gradient tiles and four (16 -> 16) or six (16 -> 32) weight-gradient bands, so 257 is the
# smallest n at which a work-group walks a second tile with its resident weights and a part holds a second band, which is
# also where the deal of K steps to the waves runs on across bands.  The tanh case stays at n = 2 and a ReLU one walks at 257:
# tanh is evaluated in fp32 on the device and in float64 here, an element whose two values straddle a bf16 rounding boundary
# moves 288 outputs by up to a bf16 ulp of the input times a weight (above atol), and among 257 x 16 x 36 x 48 inputs some
# do (measured: 1458 of 14.2 M outputs off by up to 1.2e-3); max(x, 0) is exact in both.
CASES = [(16, 16, 1, 1, 5, a) for a in range(4)] + [(16, 32, 5, 4, 2, a) for a in range(4)] + [
    (16, 16, 3, 37, 2, 1), (16, 32, 7, 9, 3, 0), (16, 16, 36, 48, 257, 1), (16, 32, 36, 48, 2, 2), (16, 32, 36, 48, 257, 1)]


@pytest.mark.parametrize("cin,cout,h,w,n,act", CASES)
def test_bf16_c16_conv_fwd_dgrad_wgrad(cin, cout, h, w, n, act):
    d, t, ref = _layer(cin, cout, h, w, n, act)
    o = _run(d, t, n, act, *BF16)
    np.testing.assert_allclose(_nchw(o["y"]).cpu().double(), ref["y"], **FWD)
    np.testing.assert_allclose(_nchw(o["yres"]).cpu().double(), ref["res"] + ref["y"], **FWD)
    np.testing.assert_allclose(_nchw(o["yact"]).cpu().double(), ACTS[act](ref["res"] + ref["y"]), **FWD)
    np.testing.assert_allclose(_nchw(o["gx"]).cpu().double(), ref["gx"], **FWD)
    np.testing.assert_allclose(_nchw(o["gxadd"]).cpu().double(), ref["gadd"] + ref["gx"], **FWD)
    np.testing.assert_allclose(o["gw"].cpu().double(), ref["gw"], **WG)
    np.testing.assert_allclose(o["gb"].cpu().double(), ref["gb"], **WG)


def test_bf16_still_refuses_other_pairs_with_a_16():
    d = lib.sf_res_desc(Cin=16, H=4, W=4, Cout=64, in_u8=0, act_in=1, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    x, w, b = torch.ones(1, 4, 4, 16, device="cuda"), torch.ones(144, 64, device="cuda"), torch.ones(64, device="cuda")
    out = torch.full((1, 4, 4, 64), 7.0, device="cuda")
    with pytest.raises(lib.SfHipError, match="16 -> 16 and 16 -> 32"):
        lib.res_conv_fwd_bf16(x, 256, None, 0, w, b, out, 1, d)
    assert lib.res_conv_wgrad_bf16_workspace(1, d) == 0 and bool((out == 7.0).all())


@pytest.mark.parametrize("cout,h,w", [(16, 8, 6), (32, 5, 4)])
def test_bf16_c16_forward_does_not_depend_on_the_batch(cout, h, w):
    d, t, _ = _layer(16, cout, h, w, 5, 3)
    full, one = torch.empty(5, h, w, cout, device="cuda"), torch.empty(1, h, w, cout, device="cuda")
    lib.res_conv_fwd_bf16(t["x"], h * w * 16, None, 0, t["w"], t["b"], full, 5, d)
    for i in range(5):
        lib.res_conv_fwd_bf16(t["x"][i:i + 1].contiguous(), h * w * 16, None, 0, t["w"], t["b"], one, 1, d)
        assert torch.equal(one[0], full[i]), i


def test_bf16_c16_weight_gradient_is_deterministic():
    h, w, n = 36, 48, 3
    d, t, _ = _layer(16, 32, h, w, n, 1)
    ws = torch.empty(lib.res_conv_wgrad_bf16_workspace(n, d), dtype=torch.uint8, device="cuda")
    gw, gb = torch.empty(2, 144, 32, device="cuda"), torch.empty(2, 32, device="cuda")
    for i in range(2):
        lib.res_conv_wgrad_bf16(t["x"], h * w * 16, None, 0, t["gy"], gw[i], gb[i], n, d, ws)
    assert torch.equal(gw[0], gw[1]) and torch.equal(gb[0], gb[1])


def test_bf16_width_1_tower_matches_its_rounding_torch_twin():
    """every layer but the raw-frame one on the bf16 family; the method and the bounds of
    test_bf16_width_2_tower_matches_its_rounding_torch_twin; 3 x 5 x 6 pools to 3 x 3, 2 x 2 and 1 x 1"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic, global_model_factory
    from sample_factory_amd.model.torch_policy import build_torch_actor_critic
    cfg = _cfg("elu", encoder_conv_mlp_layers=[64], encoder_resnet_width=1, encoder_resnet_bf16=True)
    shape, A, n = (3, 5, 6), 5, 4
    ac = create_actor_critic(cfg, _space(shape), spaces.Discrete(A), torch.device("cuda"))
    assert [c.bf16 for c in ac.encoders["obs"].convs] == [False] + [True] * 14
    tm = build_torch_actor_critic(cfg, _space(shape), spaces.Discrete(A), global_model_factory()).double()
    g = torch.Generator().manual_seed(11)
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
