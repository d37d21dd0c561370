"""resnet_impala on the native kernels (csrc/sf_resnet.hip, model/encoder_resnet.py): every kernel against float64 torch,
the model against the reference's forward (tests/golden/model_fwd_resnet.npz) and against torch autograd for its
gradients, checkpoints, and a training iteration of the whole engine."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "model_fwd_resnet.npz"), allow_pickle=True)
ACTS = {0: lambda x: x, 1: F.relu, 2: torch.tanh, 3: F.elu}


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _w_native(w):  # OIHW -> [(kh*3 + kw)*Cin + c, Cout]
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("cin,cout,h,w,n", [(16, 16, 7, 9, 5), (32, 32, 8, 6, 3), (16, 32, 1, 1, 7), (32, 16, 11, 4, 2)])
def test_res_conv_fwd_dgrad_wgrad_f32(act, cin, cout, h, w, n):
    g = torch.Generator().manual_seed(cin * 100 + h * 10 + act)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.2
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    res = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    gy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    gadd = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    wr, br = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(ACTS[act](xr), wr, br, padding=1)
    y.backward(gy)
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=act, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    xc, wc, bc = _nhwc(x).float().cuda(), _w_native(wt).float().cuda(), b.float().cuda()
    out = torch.empty(n, h, w, cout, device="cuda")
    out_act = torch.empty_like(out)
    lib.res_conv_fwd(xc, h * w * cin, None, 0, wc, bc, out, n, d)
    np.testing.assert_allclose(_nchw(out).cpu().double(), y.detach(), atol=2e-4, rtol=1e-4)
    rc = _nhwc(res).float().cuda()
    lib.res_conv_fwd(xc, h * w * cin, None, 0, wc, bc, out, n, d, residual=rc, out_act=out_act, act_out=act)
    np.testing.assert_allclose(_nchw(out).cpu().double(), res + y.detach(), atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(_nchw(out_act).cpu().double(), ACTS[act](res + y.detach()), atol=2e-4, rtol=1e-4)
    # data gradient: (conv_transpose(gy) * act'(x)) [+ g_add]
    gyc = _nhwc(gy).float().cuda()
    gx = torch.empty(n, h, w, cin, device="cuda")
    lib.res_conv_dgrad(gyc, wc, xc if act else None, gx, n, d)
    np.testing.assert_allclose(_nchw(gx).cpu().double(), xr.grad, atol=2e-4, rtol=1e-4)
    lib.res_conv_dgrad(gyc, wc, xc if act else None, gx, n, d, g_add=_nhwc(gadd).float().cuda())
    np.testing.assert_allclose(_nchw(gx).cpu().double(), gadd + xr.grad, atol=2e-4, rtol=1e-4)
    # weight / bias gradient, bit-identical across runs
    gw, gb = torch.empty(9 * cin, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(lib.res_conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.res_conv_wgrad(xc, h * w * cin, None, 0, gyc, gw, gb, n, d, ws)
    gw1, gb1 = gw.clone(), gb.clone()
    np.testing.assert_allclose(gw.cpu().double(), _w_native(wr.grad), atol=5e-4, rtol=1e-4)
    np.testing.assert_allclose(gb.cpu().double(), br.grad, atol=5e-4, rtol=1e-4)
    lib.res_conv_wgrad(xc, h * w * cin, None, 0, gyc, gw, gb, n, d, ws)
    assert torch.equal(gw, gw1) and torch.equal(gb, gb1)


@pytest.mark.parametrize("cin,h,w", [(4, 84, 84), (3, 13, 17), (1, 1, 2), (5, 6, 5)])
@pytest.mark.parametrize("mode", ["dense", "index", "traj"])
def test_res_conv_first_layer_u8(cin, h, w, mode):
    """raw u8 NCHW frames, (x - mean) / scale on load, zero padding in the normalised domain; index / offset / traj_T"""
    g = torch.Generator().manual_seed(cin + h + w)
    E, T, cout = 3, 4, 16
    slab = torch.randint(0, 256, (E, T + 1, cin, h, w), generator=g, dtype=torch.uint8)
    flat = slab[:, :T].reshape(E * T, cin, h, w)  # dataset row d = e*T + t
    mean, scale = 17.0, 255.0
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.2
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=1, act_in=0, traj_T=0, sub_mean=mean,
                        inv_scale=float(np.float32(1.0 / scale)))
    elems = cin * h * w
    if mode == "dense":
        rows, src, index, offset = torch.arange(2, 9), slab.reshape(-1, elems)[2:].cuda(), None, 0
        ref_in = slab.reshape(-1, cin, h, w)[2:9]
    elif mode == "index":
        rows = torch.tensor([5, 0, 9, 3, 3, 11], dtype=torch.int32)
        src, index, offset = flat.reshape(-1).cuda(), rows.cuda(), 0
        ref_in = flat[rows.long()]
    else:
        d.traj_T = T
        rows = torch.arange(3, 10)
        src, index, offset = slab.reshape(-1).cuda(), None, 3
        ref_in = flat[3:10]
    n = ref_in.shape[0]
    xn = (ref_in.double() - mean) / scale
    xr = xn.clone().requires_grad_(True)
    wr, br = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br, padding=1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    wc, bc = _w_native(wt).float().cuda(), b.float().cuda()
    out = torch.empty(n, h, w, cout, device="cuda")
    lib.res_conv_fwd(src, elems, index, offset, wc, bc, out, n, d)
    np.testing.assert_allclose(_nchw(out).cpu().double(), y.detach(), atol=2e-4, rtol=1e-4)
    gw, gb = torch.empty(9 * cin, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(lib.res_conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.res_conv_wgrad(src, elems, index, offset, _nhwc(gy).float().cuda(), gw, gb, n, d, ws)
    np.testing.assert_allclose(gw.cpu().double(), _w_native(wr.grad), atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(gb.cpu().double(), br.grad, atol=2e-3, rtol=1e-4)
    gw1 = gw.clone()
    lib.res_conv_wgrad(src, elems, index, offset, _nhwc(gy).float().cuda(), gw, gb, n, d, ws)
    assert torch.equal(gw, gw1)


@pytest.mark.parametrize("n,c,h,w", [(3, 16, 7, 9), (2, 32, 8, 8), (5, 16, 1, 1), (1, 32, 2, 5)])
def test_res_pool_ties_and_backward(n, c, h, w):
    """integer-valued inputs: ties everywhere, torch's first-maximum rule decides which input gets the gradient"""
    g = torch.Generator().manual_seed(n * h * w)
    x = torch.randint(-3, 3, (n, c, h, w), generator=g).double()
    xr = x.clone().requires_grad_(True)
    y, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    oh, ow = y.shape[2], y.shape[3]
    xc = _nhwc(x).float().cuda()
    out = torch.empty(n, oh, ow, c, device="cuda")
    arg = torch.empty(n, oh, ow, c, dtype=torch.uint8, device="cuda")
    lib.res_pool_fwd(xc, out, arg, n, h, w, c)
    assert torch.equal(_nchw(out).cpu().double(), y.detach())
    # window position -> flat input index, as torch reports it
    a = _nchw(arg).cpu().long()
    ohs = torch.arange(oh).view(1, 1, oh, 1)
    ows = torch.arange(ow).view(1, 1, 1, ow)
    flat_idx = (2 * ohs - 1 + a // 3) * w + (2 * ows - 1 + a % 3)
    assert torch.equal(flat_idx, idx)
    gx = torch.empty(n, h, w, c, device="cuda")
    lib.res_pool_bwd(_nhwc(gy).float().cuda(), arg, gx, n, h, w, c)
    np.testing.assert_allclose(_nchw(gx).cpu().double(), xr.grad, atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ model
def _cfg(act, **kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    base = dict(encoder_conv_architecture="resnet_impala", nonlinearity=act, obs_scale=255.0, obs_subtract_mean=0.0,
                normalize_input=False, use_rnn=False, normalize_returns=False)
    base.update(kw)
    cfg = default_cfg(**base)
    cfg.dp_world = 1
    return cfg


def _space(shape):
    from sample_factory_amd.envs import spaces
    return spaces.Dict({"obs": spaces.Box(0, 255, tuple(shape), np.uint8)})


def _seeded(tag):
    from oracle.weights import seeded_state
    shapes = [(str(n), ast.literal_eval(str(s))) for n, s in zip(G[f"{tag}_param_names"], G[f"{tag}_param_shapes"])]
    return {k: torch.from_numpy(v) for k, v in seeded_state(shapes, int(G[f"{tag}_param_seed"])).items()}


@pytest.mark.parametrize("tag", ["elu84", "relu84", "odd"])
def test_resnet_native_forward_matches_reference(tag):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.actor_critic_multikey import MultiKeyActorCritic
    from sample_factory_amd.model.encoder_resnet import ResnetImpalaTower
    from sample_factory_amd.model.model_factory import create_actor_critic
    obs = G[f"{tag}_obs"]
    ac = create_actor_critic(_cfg(str(G[f"{tag}_nonlinearity"])), _space(obs.shape[1:]), spaces.Discrete(6),
                             torch.device("cuda"))
    assert isinstance(ac, MultiKeyActorCritic) and isinstance(ac.encoders["obs"], ResnetImpalaTower)
    assert ac.num_params() == int(G[f"{tag}_num_params"])
    assert [n for n, _ in ac.ref_param_shapes()] == [str(n) for n in G[f"{tag}_param_names"]]
    sd = _seeded(tag)
    ac.load_state_dict(sd, strict=True)
    back = ac.state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    ac.eval()
    res = ac.forward({"obs": torch.from_numpy(obs).cuda()})
    torch.cuda.synchronize()
    np.testing.assert_allclose(res["action_logits"].cpu().numpy(), G[f"{tag}_action_logits"], atol=1e-4, rtol=1e-3)
    np.testing.assert_allclose(res["values"].cpu().numpy(), G[f"{tag}_values"], atol=1e-4, rtol=1e-3)


@pytest.mark.parametrize("act", ["elu", "relu", "tanh"])
@pytest.mark.parametrize("shape,mlp,norm", [((4, 36, 36), [64], False), ((3, 13, 17), [], False),
                                            ((4, 20, 12), [32, 16], True)])
def test_resnet_native_gradients_match_torch(act, shape, mlp, norm):
    """first-step gradients of every parameter: native forward + backward against the repository's torch construction
    (model/encoder.py ResnetEncoder + trunk) under float64 autograd, same weights and frames"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic, global_model_factory
    from sample_factory_amd.model.torch_policy import build_torch_actor_critic
    cfg = _cfg(act, encoder_conv_mlp_layers=mlp, normalize_input=norm)
    space, A, n = _space(shape), 5, 9
    ac = create_actor_critic(cfg, space, spaces.Discrete(A), torch.device("cuda"))
    tm = build_torch_actor_critic(cfg, space, spaces.Discrete(A), global_model_factory()).double()
    g = torch.Generator().manual_seed(len(mlp) * 7 + shape[1])
    sd = {}
    for name, p in tm.named_parameters():
        sd[name] = (torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1)).float()
    ac.load_state_dict(sd, strict=True)
    tm.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
    obs = torch.randint(0, 256, (n,) + shape, generator=g, dtype=torch.uint8)
    if norm:  # normalize_input: the same running statistics on both sides
        ac.obs_normalizer.update({"obs": obs.cuda()}, ac.obs_elems, n)
        sdn = {k: v for k, v in ac.state_dict().items() if k.startswith("obs_normalizer.")}
        mu = sdn["obs_normalizer.running_mean_std.running_mean_std.obs.running_mean"].double()
        var = sdn["obs_normalizer.running_mean_std.running_mean_std.obs.running_var"].double()
        xn = ((obs.double() / 255.0 - mu) / torch.sqrt(var + 1e-5)).clamp(-5, 5)
    else:
        xn = obs.double() / 255.0
    heads = ac.forward_heads({"obs": obs.cuda()}, n, tag="train")[-1]
    gh = torch.randn(heads.shape, generator=g).cuda()
    gh[:, 1 + A:] = 0
    ac.backward(None, gh, {"obs": obs.cuda()}, n)
    grads = ac.flat_to_ref(ac.flat_grads)
    head = tm.forward_head({"obs": xn})
    core, _ = tm.forward_core(head, torch.zeros(n, 1, dtype=torch.float64))
    out = tm.forward_tail(core)
    np.testing.assert_allclose(heads[:, 0].cpu().double(), out["values"].detach(), atol=2e-4, rtol=1e-3)
    np.testing.assert_allclose(heads[:, 1:1 + A].cpu().double(), out["action_logits"].detach(), atol=2e-4, rtol=1e-3)
    ghd = gh.cpu().double()
    loss = (out["values"] * ghd[:, 0]).sum() + (out["action_logits"] * ghd[:, 1:1 + A]).sum()
    loss.backward()
    for name, p in tm.named_parameters():
        ref = p.grad
        scale = float(ref.abs().max()) + 1e-6
        err = float((grads[name].double() - ref).abs().max()) / scale
        assert err < 2e-3, f"{name}: relative error {err:.2e}"


def test_resnet_training_iteration_and_checkpoint(tmp_path):
    """a sync training iteration of the whole engine on the synthetic 84x84x4 env; rollout steps replayed as launch
    programs; a state_dict round trip and a checkpoint file reload"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.model.actor_critic_multikey import MultiKeyActorCritic
    from sample_factory_amd.train import make_runner
    register_env("synthetic_atari", make_synthetic_env)
    cfg = default_cfg(env="synthetic_atari", use_rnn=False, nonlinearity="elu", normalize_input=False, obs_scale=255.0,
                      encoder_conv_architecture="resnet_impala", rollout=8, batch_size=256, num_batches_per_epoch=2,
                      num_epochs=1, num_workers=1, num_envs_per_worker=1, async_rl=False, seed=0, serial_mode=True,
                      synthetic_num_agents=64, exploration_loss_coeff=0.01)
    cfg, runner = make_runner(cfg)
    runner.init()
    ac = runner.learner.actor_critic
    assert isinstance(ac, MultiKeyActorCritic)
    p0 = ac.flat_params.clone()
    for _ in range(3):
        stats = runner.iteration()
    torch.cuda.synchronize()
    assert np.isfinite(stats["train"]["loss"])
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    sd = ac.state_dict()
    path = os.path.join(str(tmp_path), "ckpt.pth")
    torch.save(sd, path)
    flat = ac.flat_params.clone()
    ac.flat_params.zero_()
    ac.load_state_dict(torch.load(path), strict=True)
    assert torch.equal(ac.flat_params, flat)


# ------------------------------------------------------------------------------------------------ more kernel edges
def test_res_pool_nan_wins_and_strided_f32_input():
    """torch's max-pool lets a NaN replace the running maximum; a strided f32 input (in_sample_stride > elements)"""
    x = torch.arange(2 * 16 * 5 * 6, dtype=torch.float64).reshape(2, 16, 5, 6) % 7
    x[0, 3, 1, 1] = float("nan")
    x[1, 0, 4, 5] = float("nan")
    y, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    out = torch.empty(2, 3, 3, 16, device="cuda")
    arg = torch.empty(2, 3, 3, 16, dtype=torch.uint8, device="cuda")
    lib.res_pool_fwd(_nhwc(x).float().cuda(), out, arg, 2, 5, 6, 16)
    o = _nchw(out).cpu().double()
    assert torch.equal(torch.isnan(o), torch.isnan(y)) and torch.isnan(y).any()
    assert torch.equal(torch.nan_to_num(o, nan=-1.0), torch.nan_to_num(y, nan=-1.0))
    # strided f32 input: 3 extra floats between samples
    n, cin, h, w, cout = 4, 16, 5, 7, 32
    g = torch.Generator().manual_seed(5)
    xs = torch.randn(n, h * w * cin + 12, generator=g, dtype=torch.float64)
    xv = xs[:, :h * w * cin].reshape(n, h, w, cin)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.2
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.elu(_nchw(xv)), wt, b, padding=1)
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=3, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    res = torch.empty(n, h, w, cout, device="cuda")
    lib.res_conv_fwd(xs.float().cuda(), h * w * cin + 12, None, 0, _w_native(wt).float().cuda(), b.float().cuda(), res, n, d)
    np.testing.assert_allclose(_nchw(res).cpu().double(), ref, atol=2e-4, rtol=1e-4)


def test_res_conv_wgrad_precision_at_a_training_size():
    """stage-2 geometry of an 84x84 minibatch of 512 samples: 42x42 pixels, 903 168 rows in 1024 partial sums"""
    n, cin, cout, h, w = 512, 16, 16, 42, 42
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, h, w, cin, generator=g)
    gy = torch.randn(n, h, w, cout, generator=g)
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=1, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    gw, gb = torch.empty(9 * cin, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(lib.res_conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 1024 * (9 * cin * cout + cout) * 4
    lib.res_conv_wgrad(x.cuda(), h * w * cin, None, 0, gy.cuda(), gw, gb, n, d, ws)
    xd = F.relu(_nchw(x).double().cuda())
    ref = torch.nn.grad.conv2d_weight(xd, (cout, cin, 3, 3), _nchw(gy).double().cuda(), padding=1)
    err = float((gw.double() - _w_native(ref)).abs().max() / ref.abs().max())
    berr = float((gb.double() - _nchw(gy).double().cuda().sum((0, 2, 3))).abs().max() / float(gy.double().abs().sum((0, 1, 2)).max()))
    assert err < 2e-5 and berr < 2e-6, (err, berr)


def test_resnet_reference_first_layer_samples_and_f32_frames():
    """the first conv's pre-activation and the first pool's output against the reference's; f32 frames go to the torch path"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    from sample_factory_amd.model.torch_policy import TorchPolicyAdapter
    for tag in ("elu84", "odd"):
        obs = G[f"{tag}_obs"]
        ac = create_actor_critic(_cfg(str(G[f"{tag}_nonlinearity"])), _space(obs.shape[1:]), spaces.Discrete(6),
                                 torch.device("cuda"))
        ac.load_state_dict(_seeded(tag), strict=True)
        ac.forward({"obs": torch.from_numpy(obs).cuda()})
        saved = ac.encoders["obs"]._ctx["inf"]["saved"][0]
        conv0, pool0 = _nchw(saved[1]).cpu().numpy(), _nchw(saved[2]).cpu().numpy()
        np.testing.assert_allclose(conv0[:, :, ::3, ::3], G[f"{tag}_conv0_preact_sample"], atol=2e-5, rtol=1e-4)
        np.testing.assert_allclose(pool0[:, :, ::2, ::2], G[f"{tag}_pool0_sample"], atol=2e-5, rtol=1e-4)
    from sample_factory_amd.envs import spaces as sp
    obs = G["f32_obs"]
    space = sp.Dict({"obs": sp.Box(0, 255, tuple(obs.shape[1:]), np.float32)})
    ac = create_actor_critic(_cfg("elu"), space, sp.Discrete(6), torch.device("cuda"))
    assert isinstance(ac, TorchPolicyAdapter)
    ac.load_state_dict(_seeded("f32"), strict=True)
    ac.eval()
    res = ac.forward({"obs": torch.from_numpy(obs).cuda()}, None)
    np.testing.assert_allclose(res["action_logits"].detach().cpu().numpy(), G["f32_action_logits"], atol=1e-4, rtol=1e-3)


def test_resnet_switches_send_it_to_torch(monkeypatch):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    from sample_factory_amd.model.torch_policy import TorchPolicyAdapter
    space = spaces.Dict({"obs": spaces.Box(0, 255, (3, 13, 17), np.uint8),
                         "measurements": spaces.Box(-1, 1, (5,), np.float32)})
    monkeypatch.setenv("SF_NATIVE_MULTIKEY", "0")
    assert isinstance(create_actor_critic(_cfg("elu"), space, spaces.Discrete(6), torch.device("cuda")), TorchPolicyAdapter)
    monkeypatch.setenv("SF_NATIVE_MULTIKEY", "1")
    monkeypatch.setenv("SF_NATIVE_RESNET", "0")
    assert isinstance(create_actor_critic(_cfg("elu"), _space((3, 13, 17)), spaces.Discrete(6), torch.device("cuda")),
                      TorchPolicyAdapter)


# ------------------------------------------------------------------------------------------------ Learner.train replays
@pytest.mark.parametrize("name", ["resnet", "resnet_norm", "resnet_gru"])
def test_learner_train_matches_reference_resnet(tmp_path, name):
    """the reference's Learner.train (tests/golden/train_resnet*.npz): 16 x 8 on 4x36x36 u8 frames, 2 minibatches read in
    place from the slab through the index / traj_T addressing, invalid rows; first SGD step against the reference's float64
    run, Adam moments / deltas / gradient norms against its fp32 run, deltas against its float64 run"""
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.actor_critic import get_rnn_size
    from sample_factory_amd.model.actor_critic_multikey import MultiKeyActorCritic
    from tests.parity_util import compare_post_train
    from tests.test_gpu_parity_c2_c5 import _deltas_vs_float64, _first_step_gradient, _load_batch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"train_{name}.npz"), allow_pickle=True)
    E, T, A, nb = int(g["E"]), int(g["T"]), int(g["A"]), int(g["num_batches"])
    rnn = dict(use_rnn=True, rnn_type="gru", rnn_size=32, recurrence=8) if name == "resnet_gru" else dict(use_rnn=False,
                                                                                                           recurrence=1)
    cfg = _cfg("elu", encoder_conv_mlp_layers=[64], normalize_input=name == "resnet_norm", rollout=T, batch_size=E * T // nb,
               num_batches_per_epoch=nb, num_epochs=int(g["num_epochs"]), seed=0, exploration_loss_coeff=0.01,
               serial_mode=True, train_dir=str(tmp_path), experiment="t", record_grad_norm=True,
               normalize_returns=True, **rnn)
    obs_space = _space((4, 36, 36))
    env_info = EnvInfo(obs_space, spaces.Discrete(A), E)
    from oracle.weights import seeded_state
    st = seeded_state([(str(n), ast.literal_eval(str(s))) for n, s in zip(g["param_names"], g["param_shapes"])],
                      int(g["param_seed"]))

    def make_learner():
        pv = torch.zeros(1, dtype=torch.int32)
        ln = Learner(cfg, env_info, pv, 0, ParameterServer(0, pv))
        ln.init()
        ln.actor_critic.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
        return ln

    batch = _load_batch(g, env_info, E, T, get_rnn_size(cfg))
    assert int((torch.from_numpy(g["in_policy_id"]) != 0).sum()) > 0  # the replay has invalid rows
    _first_step_gradient(make_learner, g, batch, name, bound=5e-4)
    learner = make_learner()
    ac = learner.actor_critic
    assert isinstance(ac, MultiKeyActorCritic)
    assert [n for n, _ in ac.ref_param_shapes()] == [str(n) for n in g["param_names"]]
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    stats = learner.train(batch)
    torch.cuda.synchronize()
    assert stats["learner_env_steps"] == int(g["env_steps"]) and learner.train_step == int(g["train_step"])
    np.testing.assert_allclose(ac.returns_normalizer.stats.cpu().numpy(), g["out_rms"], rtol=1e-5)
    if name == "resnet_norm":
        sub = int(g["subsample"])
        sd = ac.state_dict()
        pfx = "obs_normalizer.running_mean_std.running_mean_std.obs."
        np.testing.assert_allclose(sd[pfx + "running_mean"].reshape(-1)[::sub].numpy(), g["obsn_mean"], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(sd[pfx + "running_var"].reshape(-1)[::sub].numpy(), g["obsn_var"], rtol=1e-5, atol=1e-7)
    compare_post_train(learner, g, before, name, m_rtol=5e-4, v_rtol=1e-3, d_rtol=1e-3, gn_rtol=2e-4)
    # against float64: 5e-4 of the largest delta, or no further than 1.5x the reference's own fp32 run where that is
    # further (GRU replay: Adam's g / sqrt(v) on near-zero conv0 gradients puts the reference's fp32 deltas 4e-3 away)
    _deltas_vs_float64(ac, g, before, None, name, tight=5e-4, flipped=5e-4, vs_ref32=1.5)


# ------------------------------------------------------------------------------------------------ end to end
_RESNET = dict(encoder_conv_architecture="resnet_impala", nonlinearity="elu", encoder_conv_mlp_layers=[64])


def test_resnet_replayed_rollouts_equal_the_wrapper_path():
    """rollout steps of the resnet model replayed as launch programs: the same run bit for bit as the wrapper path"""
    from sample_factory_amd import lib as L
    from tests.test_gpu_launch_programs import _run, _same_run
    plain = _run("conv_discrete", False, 5, **_RESNET)
    prog = _run("conv_discrete", True, 5, **_RESNET)
    _same_run(plain, prog)
    for s in prog["samplers"]:
        progs = [p for p in s._progs.values() if isinstance(p, L.LaunchProgram)]
        assert progs and all(p.unsafe is None for p in progs)
        assert s.program_replays >= s.T, s.program_replays


def test_resnet_async_with_weight_snapshots():
    """async mode with normalize_input: inference reads the published weights and normaliser tables of the tower"""
    from sample_factory_amd.model.encoder_resnet import ResnetImpalaTower
    from tests.test_gpu_launch_programs import _run
    kw = dict(async_rl=True, serial_mode=False, num_batches_to_accumulate=2, **_RESNET)
    out = _run("conv_normalized", True, 6, **kw)
    tower = out["samplers"][0].ac.encoders["obs"]
    assert isinstance(tower, ResnetImpalaTower) and tower._snap is not None and tower._snap_tabs is not None
    assert sum(out["steps"]) > 0
    for k, v in out["slabs"][-1].items():
        assert torch.isfinite(v.float()).all(), k
    assert torch.isfinite(out["params"]).all()


def _dp_run(num_agents, iters):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_atari", make_synthetic_env)
    cfg = default_cfg(env="synthetic_atari", use_rnn=False, normalize_input=False, obs_scale=255.0, rollout=8,
                      batch_size=num_agents * 8, num_batches_per_epoch=1, num_epochs=1, num_workers=1, num_envs_per_worker=1,
                      async_rl=False, seed=5, serial_mode=True, synthetic_num_agents=num_agents,
                      exploration_loss_coeff=0.01, learning_rate=1e-3, **_RESNET)
    cfg, runner = make_runner(cfg)
    runner.init()
    for _ in range(iters):
        stats = runner.iteration()
    torch.cuda.synchronize()
    ac = runner.learner.actor_critic
    return dict(params=ac.flat_params.cpu().numpy(), actions=runner.traj["actions"].cpu().numpy(),
                env_steps=stats["learner_env_steps"], loss=stats["train"]["loss"])


def _dp_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", SF_DP_BACKEND="gloo")
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **_dp_run(16, 2))
    torch.distributed.destroy_process_group()


def test_resnet_two_replicas_equal_one(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for k in ("WORLD_SIZE", "RANK"):
        os.environ.pop(k, None)
    single = _dp_run(32, 2)
    r = [np.load(tmp_path / f"rank{i}.npz") for i in range(2)]
    assert int(r[0]["env_steps"]) == single["env_steps"] == 2 * 32 * 8
    np.testing.assert_array_equal(r[0]["params"], r[1]["params"])
    assert abs(float(r[0]["loss"]) - single["loss"]) < 2e-3 * max(1.0, abs(single["loss"]))
    acts = np.concatenate([r[0]["actions"], r[1]["actions"]])
    assert (acts == single["actions"]).mean() > 0.99
    diff = np.abs(r[0]["params"] - single["params"])
    assert diff.max() < 1e-3 and (diff > 2e-5).mean() < 5e-3, (diff.max(), (diff > 2e-5).mean())
