"""Wide resnet_impala towers (cfg.encoder_resnet_width = 2, 4): the 3x3 conv family on fp32 MFMA (csrc/sf_resnet_mfma.hip)
and the first layer at Cout = 64 against float64 torch on the CPU, the routing of the plain entry points, the towers
against their torch twin, and a training iteration under an augmentation."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_resnet import ACTS, _cfg, _nchw, _nhwc, _space, _w_native  # noqa: E402

FWD = dict(atol=2e-4, rtol=1e-4)   # forward and data gradient (test_gpu_resnet.py)
WG = dict(atol=5e-4, rtol=1e-4)    # weight / bias gradient


def _layer(cin, cout, h, w, n, act, seed=0):
    """N(0,1) inputs, N(0, 1/(9 Cin)) weights; float64 references of every pass; the device operands"""
    g = torch.Generator().manual_seed(cin * 100 + h * 10 + act + seed)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / (9 * cin) ** 0.5
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    res = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    gy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    gadd = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(ACTS[act](xr), wr, br, padding=1)
    y.backward(gy)
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=act, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    dev = dict(x=_nhwc(x).float().cuda(), w=_w_native(wt).float().cuda(), b=b.float().cuda(), res=_nhwc(res).float().cuda(),
               gy=_nhwc(gy).float().cuda(), gadd=_nhwc(gadd).float().cuda())
    ref = dict(y=y.detach(), res=res, gx=xr.grad, gadd=gadd, gw=_w_native(wr.grad), gb=br.grad)
    return d, dev, ref


def _run(d, t, n, act, fwd, dgrad, wgrad, wgrad_ws):
    """every pass of one layer through the given entry points -> dict of device results"""
    h, w, cin, cout = d.H, d.W, d.Cin, d.Cout
    o = {k: torch.empty(n, h, w, cout, device="cuda") for k in ("y", "yres", "yact")}
    fwd(t["x"], h * w * cin, None, 0, t["w"], t["b"], o["y"], n, d)
    fwd(t["x"], h * w * cin, None, 0, t["w"], t["b"], o["yres"], n, d, residual=t["res"], out_act=o["yact"], act_out=act)
    o["gx"], o["gxadd"] = torch.empty(n, h, w, cin, device="cuda"), torch.empty(n, h, w, cin, device="cuda")
    dgrad(t["gy"], t["w"], t["x"] if act else None, o["gx"], n, d)
    dgrad(t["gy"], t["w"], t["x"] if act else None, o["gxadd"], n, d, g_add=t["gadd"])
    o["gw"], o["gb"] = torch.empty(9 * cin, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(wgrad_ws(n, d), dtype=torch.uint8, device="cuda")
    wgrad(t["x"], h * w * cin, None, 0, t["gy"], o["gw"], o["gb"], n, d, ws)
    return o


MFMA = (lib.res_conv_fwd_mfma, lib.res_conv_dgrad_mfma, lib.res_conv_wgrad_mfma, lib.res_conv_wgrad_mfma_workspace)
PLAIN = (lib.res_conv_fwd, lib.res_conv_dgrad, lib.res_conv_wgrad, lib.res_conv_wgrad_workspace)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("cin,cout,h,w,n", [(32, 64, 7, 9, 3), (64, 64, 8, 6, 2), (64, 128, 1, 1, 5), (128, 128, 5, 4, 2),
                                            (16, 16, 3, 17, 2), (32, 32, 16, 16, 1)])
def test_mfma_conv_fwd_dgrad_wgrad(act, cin, cout, h, w, n):
    d, t, ref = _layer(cin, cout, h, w, n, act)
    o = _run(d, t, n, act, *MFMA)
    np.testing.assert_allclose(_nchw(o["y"]).cpu().double(), ref["y"], **FWD)
    np.testing.assert_allclose(_nchw(o["yres"]).cpu().double(), ref["res"] + ref["y"], **FWD)
    np.testing.assert_allclose(_nchw(o["yact"]).cpu().double(), ACTS[act](ref["res"] + ref["y"]), **FWD)
    np.testing.assert_allclose(_nchw(o["gx"]).cpu().double(), ref["gx"], **FWD)
    np.testing.assert_allclose(_nchw(o["gxadd"]).cpu().double(), ref["gadd"] + ref["gx"], **FWD)
    np.testing.assert_allclose(o["gw"].cpu().double(), ref["gw"], **WG)
    np.testing.assert_allclose(o["gb"].cpu().double(), ref["gb"], **WG)


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128)])
def test_plain_entry_points_route_wide_layers_to_the_mfma_family(cin, cout):
    """refused (SF_ERR_UNSUPPORTED) before the family existed; now the same kernels, so the same bits"""
    d, t, _ = _layer(cin, cout, 6, 5, 3, 3, seed=1)
    a, b = _run(d, t, 3, 3, *PLAIN), _run(d, t, 3, 3, *MFMA)
    assert lib.res_conv_wgrad_workspace(3, d) == lib.res_conv_wgrad_mfma_workspace(3, d) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("cin,h,w", [(3, 13, 17), (4, 36, 36)])
@pytest.mark.parametrize("mode", ["dense", "index", "traj"])
def test_first_layer_u8_at_cout_64(cin, h, w, mode):
    """width 4: raw u8 frames into 64 channels on the FMA kernels; forward, normalising forward, weight gradient"""
    g = torch.Generator().manual_seed(cin + h + w)
    E, T, cout, mean, scale = 3, 4, 64, 17.0, 255.0
    slab = torch.randint(0, 256, (E, T + 1, cin, h, w), generator=g, dtype=torch.uint8)
    flat = slab[:, :T].reshape(E * T, cin, h, w)
    elems = cin * h * w
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=1, act_in=0, traj_T=0, sub_mean=mean,
                        inv_scale=float(np.float32(1.0 / scale)))
    if mode == "dense":
        src, index, offset, ref_in = slab.reshape(-1, elems)[2:].cuda(), None, 0, slab.reshape(-1, cin, h, w)[2:9]
    elif mode == "index":
        rows = torch.tensor([5, 0, 9, 3, 3, 11], dtype=torch.int32)
        src, index, offset, ref_in = flat.reshape(-1).cuda(), rows.cuda(), 0, flat[rows.long()]
    else:
        d.traj_T = T
        src, index, offset, ref_in = slab.reshape(-1).cuda(), None, 3, flat[3:10]
    n = ref_in.shape[0]
    mu, rstd = torch.rand(elems, generator=g) * 0.5 + 0.2, torch.rand(elems, generator=g) * 2.0 + 1.0
    xn = (ref_in.double() - mean) / scale
    xnn = ((xn - mu.double().view(1, cin, h, w)) * rstd.double().view(1, cin, h, w)).clamp(-5, 5)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.2
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    wr, br = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xn, wr, br, padding=1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    wc, bc = _w_native(wt).float().cuda(), b.float().cuda()
    out = torch.empty(n, h, w, cout, device="cuda")
    lib.res_conv_fwd(src, elems, index, offset, wc, bc, out, n, d)
    np.testing.assert_allclose(_nchw(out).cpu().double(), y.detach(), atol=2e-4, rtol=1e-4)
    lib.res_conv_fwd_norm(src, elems, index, offset, mu.cuda(), rstd.cuda(), wc, bc, out, n, d)
    np.testing.assert_allclose(_nchw(out).cpu().double(), F.conv2d(xnn, wt, b, padding=1), atol=2e-4, rtol=1e-4)
    gw, gb = torch.empty(9 * cin, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(lib.res_conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.res_conv_wgrad(src, elems, index, offset, _nhwc(gy).float().cuda(), gw, gb, n, d, ws)
    np.testing.assert_allclose(gw.cpu().double(), _w_native(wr.grad), atol=2e-3, rtol=1e-4)
    np.testing.assert_allclose(gb.cpu().double(), br.grad, atol=2e-3, rtol=1e-4)


@pytest.mark.parametrize("c", [64, 128])
def test_pools_at_wide_channel_counts(c):
    n, h, w = 2, 5, 7
    g = torch.Generator().manual_seed(c)
    x = torch.randint(-3, 3, (n, c, h, w), generator=g).double().requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    out = torch.empty(n, 3, 4, c, device="cuda")
    arg = torch.empty(n, 3, 4, c, dtype=torch.uint8, device="cuda")
    lib.res_pool_fwd(_nhwc(x.detach()).float().cuda(), out, arg, n, h, w, c)
    assert torch.equal(_nchw(out).cpu().double(), y.detach())
    gx = torch.empty(n, h, w, c, device="cuda")
    lib.res_pool_bwd(_nhwc(gy).float().cuda(), arg, gx, n, h, w, c)
    np.testing.assert_allclose(_nchw(gx).cpu().double(), x.grad, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("shape", [(3, 13, 17), (4, 36, 36)])
@pytest.mark.parametrize("act", ["elu", "relu"])
def test_wide_tower_matches_its_torch_twin(k, shape, act):
    """forward and every parameter gradient against model/encoder.py's ResnetEncoder + trunk in float64, same state_dict;
    bounds of test_resnet_native_gradients_match_torch"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.encoder_resnet import ResnetImpalaTower
    from sample_factory_amd.model.model_factory import create_actor_critic, global_model_factory
    from sample_factory_amd.model.torch_policy import build_torch_actor_critic
    cfg = _cfg(act, encoder_conv_mlp_layers=[64], encoder_resnet_width=k)
    space, A, n = _space(shape), 5, 9
    ac = create_actor_critic(cfg, space, spaces.Discrete(A), torch.device("cuda"))
    assert isinstance(ac.encoders["obs"], ResnetImpalaTower)
    assert [c.N for c, *_ in ac.encoders["obs"].stages] == [16 * k, 32 * k, 32 * k]
    tm = build_torch_actor_critic(cfg, space, spaces.Discrete(A), global_model_factory()).double()
    g = torch.Generator().manual_seed(k + shape[1])
    sd = {name: (torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1)).float() for name, p in tm.named_parameters()}
    ac.load_state_dict(sd, strict=True)
    back = ac.state_dict()
    assert all(torch.equal(back[name], v) for name, v in sd.items())
    tm.load_state_dict({name: v.double() for name, v in back.items()}, strict=False)  # ... and the other way
    obs = torch.randint(0, 256, (n,) + shape, generator=g, dtype=torch.uint8)
    heads = ac.forward_heads({"obs": obs.cuda()}, n, tag="train")[-1]
    gh = torch.randn(heads.shape, generator=g).cuda()
    gh[:, 1 + A:] = 0
    ac.backward(None, gh, {"obs": obs.cuda()}, n)
    grads = ac.flat_to_ref(ac.flat_grads)
    core, _ = tm.forward_core(tm.forward_head({"obs": obs.double() / 255.0}), torch.zeros(n, 1, dtype=torch.float64))
    out = tm.forward_tail(core)
    np.testing.assert_allclose(heads[:, 0].cpu().double(), out["values"].detach(), atol=2e-4, rtol=1e-3)
    np.testing.assert_allclose(heads[:, 1:1 + A].cpu().double(), out["action_logits"].detach(), atol=2e-4, rtol=1e-3)
    ghd = gh.cpu().double()
    ((out["values"] * ghd[:, 0]).sum() + (out["action_logits"] * ghd[:, 1:1 + A]).sum()).backward()
    for name, p in tm.named_parameters():
        err = float((grads[name].double() - p.grad).abs().max()) / (float(p.grad.abs().max()) + 1e-6)
        assert err < 2e-3, f"{name}: relative error {err:.2e}"


def test_width_2_trains_under_random_shift_and_reloads_through_enjoy(tmp_path):
    """one training iteration of the engine with --augment_random_shift=2 (refused for a tower that runs in torch), then the
    checkpoint through enjoy's loader into a model rebuilt from config.json"""
    from sample_factory_amd import enjoy
    from sample_factory_amd.cfg.arguments import default_cfg, load_from_checkpoint
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.model.encoder_resnet import ResnetImpalaTower
    from sample_factory_amd.model.model_factory import create_actor_critic
    from sample_factory_amd.train import make_runner
    register_env("synthetic_atari", make_synthetic_env)
    kw = dict(env="synthetic_atari", use_rnn=False, nonlinearity="elu", normalize_input=False, obs_scale=255.0,
              encoder_conv_architecture="resnet_impala", rollout=8, batch_size=256, num_batches_per_epoch=2, num_epochs=1,
              num_workers=1, num_envs_per_worker=1, async_rl=False, seed=0, serial_mode=True, synthetic_num_agents=64,
              exploration_loss_coeff=0.01, train_dir=str(tmp_path), experiment="wide")
    cfg, runner = make_runner(default_cfg(encoder_resnet_width=2, augment_random_shift=2, **kw))
    runner.init()
    ac = runner.learner.actor_critic
    assert isinstance(ac.encoders["obs"], ResnetImpalaTower) and ac.encoders["obs"].stages[2][0].N == 64
    p0 = ac.flat_params.clone()
    stats = runner.iteration()
    torch.cuda.synchronize()
    assert np.isfinite(stats["train"]["loss"]) and runner.learner._shift_pad == 2
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    runner.learner.save()
    assert os.path.isfile(tmp_path / "wide" / "config.json")
    cfg2 = load_from_checkpoint(default_cfg(**kw))  # enjoy: the width comes from config.json
    assert cfg2.encoder_resnet_width == 2
    ac2 = create_actor_critic(cfg2, runner.env_info.obs_space, runner.env_info.action_space, torch.device("cuda"))
    enjoy.load_state_dict(cfg2, ac2, torch.device("cuda"))
    assert torch.equal(ac2.flat_params, ac.flat_params)
