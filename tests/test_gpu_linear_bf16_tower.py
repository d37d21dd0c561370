"""--mlp_bf16 through the model: every flagged fully connected layer of an image tower and a vector tower against float64 on the
tensors the tower itself fed it, rollout == training to the bit, the flag off, and one iteration of the engine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_conv_bf16 import ACT_BWD, _bf  # noqa: E402
from tests.test_gpu_resnet import ACTS, _cfg  # noqa: E402
from tests.test_gpu_resnet_wide import FWD, WG  # noqa: E402

N, A = 6, 5
# (cfg overrides, observation shape and dtype, [L.bf16 for L in ac.layers] under the flag)
TOWERS = {"image": (dict(encoder_conv_architecture="convnet_atari", encoder_conv_mlp_layers=[64], decoder_mlp_layers=[32]),
                    (4, 36, 36), np.uint8, [False, False, False, True, True, False]),
          "vector": (dict(encoder_mlp_layers=[64, 64], obs_scale=1.0), (24,), np.float32, [False, True, False])}


def _tower(name, bf16=True):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    over, shape, dtype, flags = TOWERS[name]
    cfg = _cfg("relu", mlp_bf16=bf16, **over)
    torch.manual_seed(3)
    space = spaces.Dict({"obs": spaces.Box(0, 255, shape, dtype)})
    ac = create_actor_critic(cfg, space, spaces.Discrete(A), torch.device("cuda"))
    g = torch.Generator().manual_seed(11)
    obs = torch.randint(0, 256, (N,) + shape, generator=g, dtype=torch.uint8) if dtype == np.uint8 else \
        torch.randn((N,) + shape, generator=g)
    gh = torch.randn(N, ac.heads_ld, generator=g).cuda()
    gh[:, 1 + A:] = 0
    return ac, obs.cuda(), gh, flags


@pytest.mark.parametrize("name", list(TOWERS))
def test_tower_layers_match_float64_on_their_own_operands(name):
    ac, obs, gh, flags = _tower(name)
    assert [L.bf16 for L in ac.layers] == flags
    rollout = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="inf")[-1].clone()
    acts = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="train")
    assert torch.equal(rollout, acts[-1])  # the behaviour policy and the learner evaluate the same function
    ac.backward(acts, gh, obs, N, sample_stride=ac.obs_elems)
    torch.cuda.synchronize()
    ctx, kind = ac._ctx["train"], ac.act_kind
    for li in (i for i, f in enumerate(flags) if f):
        L = ac.layers[li]
        rows = lambda t: t.reshape(N, -1).cpu().double()  # noqa: E731
        x, y, g, gin = rows(ctx["inputs"][li]), rows(ctx["acts"][li]), rows(ac._bufs[("g", li)]), rows(ac._bufs[("g", li - 1)])
        w = L.w.cpu().double()
        np.testing.assert_allclose(y, ACTS[kind](_bf(x) @ _bf(w) + L.b.cpu().double()), **FWD)
        np.testing.assert_allclose(L.gw.cpu().double(), _bf(x).t() @ _bf(g), **WG)
        np.testing.assert_allclose(L.gb.cpu().double(), _bf(g).sum(0), **WG)
        np.testing.assert_allclose(gin, (_bf(g) @ _bf(w).t()) * ACT_BWD[L.in_act_kind](x), **FWD)


@pytest.mark.parametrize("name", list(TOWERS))
def test_flag_off_never_reaches_the_bf16_family(monkeypatch, name):
    def boom(*a, **k):
        raise AssertionError("a bf16 wrapper was called with mlp_bf16 off")
    for fn in ("linear_fwd_bf16", "linear_dgrad_bf16", "linear_wgrad_bf16", "linear_wgrad_bf16_workspace", "linear_bf16_supported"):
        monkeypatch.setattr(lib, fn, boom)
    heads = []
    for _ in range(2):
        ac, obs, gh, _ = _tower(name, bf16=False)
        assert not any(L.bf16 for L in ac.layers)
        acts = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="train")
        ac.backward(acts, gh, obs, N, sample_stride=ac.obs_elems)
        heads.append((acts[-1].clone(), ac.flat_grads.clone()))
    assert torch.equal(heads[0][0], heads[1][0]) and torch.equal(heads[0][1], heads[1][1])


def test_one_iteration_with_the_flag(tmp_path):
    from sample_factory_amd.train import make_runner
    from tests.test_gpu_rollout_reuse import _cfg as run_cfg
    cfg, runner = make_runner(run_cfg(mlp_bf16=True, train_dir=str(tmp_path), experiment="mlp_bf16"))
    assert runner.init() == 0
    ac = runner.learner.actor_critic
    assert [L.bf16 for L in ac.layers] == [False, False, False, True, False]
    p0 = ac.flat_params.clone()
    stats = runner.iteration()
    torch.cuda.synchronize()
    assert ac._keep is None  # reuse_rollout_activations=auto resolved to off: configure_keep returned 0
    assert all(np.isfinite(v) for v in stats["train"].values() if isinstance(v, float))
    assert np.isfinite(stats["train"]["loss"]) and torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    runner.close_envs()
