"""--encoder_conv1_bf16 through the model: layer 0 of a convnet_impala / convnet_atari / f32-frame tower against float64 on the
tensors the tower itself fed it, rollout == training to the bit, the flag off, and one iteration of the engine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_conv1_bf16 import _bf, _w_frame, x_prime  # noqa: E402
from tests.test_gpu_resnet import ACTS, _cfg, _nchw  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG  # noqa: E402

N, A = 6, 5
# (architecture, frame shape, frame dtype, normalize_input, activation)
TOWERS = [("convnet_impala", (4, 84, 84), np.uint8, True, "elu"), ("convnet_atari", (4, 36, 36), np.uint8, False, "relu"),
          ("convnet_simple", (3, 72, 128), np.float32, True, "tanh")]


def _tower(arch, shape, dtype, norm, act, bf16=True):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    cfg = _cfg(act, encoder_conv_architecture=arch, encoder_conv_mlp_layers=[64], normalize_input=norm, encoder_conv1_bf16=bf16)
    u8 = dtype == np.uint8
    space = spaces.Dict({"obs": spaces.Box(0, 255 if u8 else 1, tuple(shape), dtype)})
    torch.manual_seed(3)
    ac = create_actor_critic(cfg, space, spaces.Discrete(A), torch.device("cuda"))
    g = torch.Generator().manual_seed(11)
    obs = (torch.randint(0, 256, (N,) + shape, generator=g, dtype=torch.uint8) if u8 else torch.rand((N,) + shape, generator=g)).cuda()
    if norm:  # tables of a normaliser that has seen data: part of every frame is clamped
        on = ac.obs_normalizer
        on.mu_tab.copy_((torch.rand(on.mu_tab.shape, generator=g) * 0.4).cuda())
        on.rstd_tab.copy_((torch.rand(on.rstd_tab.shape, generator=g) * 12.0 + 0.1).cuda())
    gh = torch.randn(N, ac.heads_ld, generator=g).cuda()
    gh[:, 1 + A:] = 0
    return ac, obs, gh


@pytest.mark.parametrize("arch,shape,dtype,norm,act", TOWERS)
def test_layer0_matches_float64_on_its_own_operands(arch, shape, dtype, norm, act):
    ac, obs, gh = _tower(arch, shape, dtype, norm, act)
    assert [L.bf16 for L in ac.layers] == [True] + [False] * (len(ac.layers) - 1)
    rollout = [a.clone() for a in ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="inf")]
    acts = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="train")
    assert torch.equal(rollout[0], acts[0]) and torch.equal(rollout[-1], acts[-1])  # one function in rollout and training
    ac.backward(acts, gh, obs, N, sample_stride=ac.obs_elems)
    torch.cuda.synchronize()
    ctx, L, kind = ac._ctx["train"], ac.layers[0], ac.act_kind
    assert ctx["relu_mask0"] is None and (ctx["norm_tabs"] is not None) == norm
    d = L.desc
    mu, rstd = ctx["norm_tabs"] if norm else (None, None)
    xb = _bf(x_prime(ctx["first_in"][0].view((N,) + shape), d.sub_mean, d.inv_scale, mu, rstd))
    w = L.w.cpu().double().t().reshape(d.Cout, d.Cin, 8, 8)
    y = _nchw(ctx["acts"][0].view(N, d.OH, d.OW, d.Cout)).cpu().double()
    g = _nchw(ac._bufs[("g", 0)].view(N, d.OH, d.OW, d.Cout)).cpu().double()
    np.testing.assert_allclose(y, ACTS[kind](F.conv2d(xb, _bf(w), L.b.cpu().double(), stride=4)), **FWD)
    np.testing.assert_allclose(L.gw.cpu().double(), _w_frame(torch.nn.grad.conv2d_weight(xb, w.shape, _bf(g), stride=4)), **WG)
    np.testing.assert_allclose(L.gb.cpu().double(), _bf(g).sum((0, 2, 3)), **WG)


def test_flag_off_runs_the_f32_path_to_the_bit(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a conv1 bf16 wrapper was called with encoder_conv1_bf16 off")
    for name in ("conv1_fwd_bf16", "conv1_wgrad_bf16", "conv1_wgrad_bf16_workspace", "conv1_bf16_supported"):
        monkeypatch.setattr(lib, name, boom)
    ac, obs, gh = _tower(*TOWERS[0], bf16=False)
    assert not any(L.bf16 for L in ac.layers)
    acts = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="train")
    ac.backward(acts, gh, obs, N, sample_stride=ac.obs_elems)
    L, (mu, rstd) = ac.layers[0], ac._ctx["train"]["norm_tabs"]
    out = torch.empty_like(acts[0])
    lib.conv_fwd_norm(obs, ac.obs_elems, None, 0, mu, rstd, L.w, L.b, out, N, L.desc)  # what the parent launches
    assert torch.equal(out, acts[0])


@pytest.mark.parametrize("flags", [dict(encoder_conv1_bf16=True),
                                   dict(encoder_conv1_bf16=True, encoder_conv_bf16=True, mlp_bf16=True)])
def test_one_iteration_with_the_flag(tmp_path, flags):
    from sample_factory_amd.train import make_runner
    from tests.test_gpu_rollout_reuse import _cfg as run_cfg
    cfg, runner = make_runner(run_cfg(train_dir=str(tmp_path), experiment="conv1_bf16", **flags))
    assert runner.init() == 0
    ac = runner.learner.actor_critic
    assert ac.layers[0].bf16 and ac.layers[1].bf16 == ("encoder_conv_bf16" in flags)
    p0 = ac.flat_params.clone()
    stats = runner.iteration()
    torch.cuda.synchronize()
    assert ac._keep is None  # reuse_rollout_activations=auto resolved to off: configure_keep returned 0
    assert np.isfinite(stats["train"]["loss"]) and torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    runner.close_envs()
