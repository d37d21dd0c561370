"""--encoder_conv_bf16 through the model: every served layer of a convnet_atari / convnet_simple tower against float64 on the
tensors the tower itself fed it, rollout == training to the bit, the flag off, and one iteration of the engine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_conv_bf16 import ACT_BWD, _bf  # noqa: E402
from tests.test_gpu_resnet import ACTS, _cfg, _nchw, _space, _w_native  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG  # noqa: E402

N, A = 6, 5
TOWERS = [("convnet_atari", (4, 36, 36), "relu"), ("convnet_atari", (3, 72, 128), "relu"), ("convnet_simple", (3, 72, 128), "elu"),
          ("convnet_simple", (4, 36, 36), "tanh")]


def _tower(arch, shape, act, bf16=True):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    cfg = _cfg(act, encoder_conv_architecture=arch, encoder_conv_mlp_layers=[64], encoder_conv_bf16=bf16)
    torch.manual_seed(3)
    ac = create_actor_critic(cfg, _space(shape), spaces.Discrete(A), torch.device("cuda"))
    g = torch.Generator().manual_seed(11)
    obs = torch.randint(0, 256, (N,) + shape, generator=g, dtype=torch.uint8).cuda()
    gh = torch.randn(N, ac.heads_ld, generator=g).cuda()
    gh[:, 1 + A:] = 0
    return ac, obs, gh


@pytest.mark.parametrize("arch,shape,act", TOWERS)
def test_tower_layers_match_float64_on_their_own_operands(arch, shape, act):
    ac, obs, gh = _tower(arch, shape, act)
    assert [L.bf16 for L in ac.layers] == [False, True, True] + [False] * (len(ac.layers) - 3)
    rollout = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="inf")[-1].clone()
    acts = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="train")
    assert torch.equal(rollout, acts[-1])  # the behaviour policy and the learner evaluate the same function
    ac.backward(acts, gh, obs, N, sample_stride=ac.obs_elems)
    torch.cuda.synchronize()
    ctx, kind = ac._ctx["train"], ac.act_kind
    for li in (1, 2):
        L, d = ac.layers[li], ac.layers[li].desc
        nchw = lambda t, c, h, w: _nchw(t.view(N, h, w, c)).cpu().double()  # noqa: E731
        x, y = nchw(ctx["inputs"][li], d.Cin, d.H, d.W), nchw(ctx["acts"][li], d.Cout, d.OH, d.OW)
        g, gin = nchw(ac._bufs[("g", li)], d.Cout, d.OH, d.OW), nchw(ac._bufs[("g", li - 1)], d.Cin, d.H, d.W)
        w = L.w_to_ref(L.w).cpu().double()
        np.testing.assert_allclose(y, ACTS[kind](F.conv2d(_bf(x), _bf(w), L.b.cpu().double(), stride=d.stride)), **FWD)
        np.testing.assert_allclose(L.gw.cpu().double(), _w_native(torch.nn.grad.conv2d_weight(_bf(x), w.shape, _bf(g), stride=d.stride)), **WG)
        np.testing.assert_allclose(L.gb.cpu().double(), _bf(g).sum((0, 2, 3)), **WG)
        ref = torch.nn.grad.conv2d_input(x.shape, _bf(w), _bf(g), stride=d.stride)
        if not (li == 1 and ctx["relu_mask0"] is not None):  # conv1's sign bits: its weight gradient masks, conv2 passes g on
            ref = ref * ACT_BWD[kind](x)
        np.testing.assert_allclose(gin, ref, **FWD)


def test_flag_off_never_reaches_the_bf16_family(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a bf16 wrapper was called with encoder_conv_bf16 off")
    for name in ("conv_fwd_bf16", "conv_dgrad_bf16", "conv_wgrad_bf16", "conv_wgrad_bf16_workspace", "conv_bf16_supported"):
        monkeypatch.setattr(lib, name, boom)
    heads = []
    for _ in range(2):
        ac, obs, gh = _tower("convnet_atari", (4, 36, 36), "relu", bf16=False)
        assert not any(L.bf16 for L in ac.layers)
        acts = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="train")
        ac.backward(acts, gh, obs, N, sample_stride=ac.obs_elems)
        heads.append((acts[-1].clone(), ac.flat_grads.clone()))
    assert torch.equal(heads[0][0], heads[1][0]) and torch.equal(heads[0][1], heads[1][1])


def test_one_iteration_with_the_flag(tmp_path):
    from sample_factory_amd.train import make_runner
    from tests.test_gpu_rollout_reuse import _cfg as run_cfg
    cfg, runner = make_runner(run_cfg(encoder_conv_bf16=True, train_dir=str(tmp_path), experiment="conv_bf16"))
    assert runner.init() == 0
    ac = runner.learner.actor_critic
    assert [L.bf16 for L in ac.layers[:3]] == [False, True, True]
    p0 = ac.flat_params.clone()
    stats = runner.iteration()
    torch.cuda.synchronize()
    assert ac._keep is None  # reuse_rollout_activations=auto resolved to off: configure_keep returned 0
    assert all(np.isfinite(v) for v in stats["train"].values() if isinstance(v, float))
    assert np.isfinite(stats["train"]["loss"]) and torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    runner.close_envs()
