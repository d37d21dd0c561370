"""cfg.normalize_input=True on u8 CHW frames of ANY geometry: the observation normaliser is applied inside the first conv's
loader (MODE_U8_NORM of csrc/sf_nn.hip, res_load of csrc/sf_resnet.hip), no normalised f32 copy of the frames is written.
Kernels against float64, models against the materialising path (SF_CONV1_NORM=0), a Learner.train replay against the
reference (tests/golden/train_u8norm.npz, tools/gen_golden_u8norm.py), async snapshots, odd addresses, launch programs."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402

ACTS = {0: lambda x: x, 1: F.relu, 2: torch.tanh, 3: F.elu}
# (Cin, H, W, Cout, vector loader?) with an 8 x 8 stride 4 first layer: VizDoom, DMLab, the Atari frame under convnet_impala,
# one grey channel, the frames of the small replays, an odd width (scalar loader)
GEOMS = [(3, 72, 128, 32, True), (3, 72, 96, 16, True), (4, 84, 84, 16, True), (1, 84, 84, 32, True), (4, 36, 36, 32, True),
         (3, 45, 53, 32, False)]
GEOM_IDS = ["x".join(map(str, g[:4])) for g in GEOMS]
SUB, INV = 3.0, float(np.float32(1.0 / 255.0))


def _desc(cin, h, w, cout, act=1, traj_T=0, fmt=1, k=8, s=4):
    return lib.sf_conv_desc(Cin=cin, H=h, W=w, Cout=cout, KH=k, KW=k, stride=s, OH=(h - k) // s + 1, OW=(w - k) // s + 1,
                            in_u8=fmt, relu=act, traj_T=traj_T, sub_mean=SUB if fmt else 0.0, inv_scale=INV if fmt else 1.0)


# ------------------------------------------------------------------------------------------------ 1. the predicate
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_every_u8_geometry_is_taken_and_named(geom):
    cin, h, w, cout, vec = geom
    d = _desc(cin, h, w, cout)
    for n in (1, 77, 256, 4096):
        assert lib.conv_norm_supported(n, d), (geom, n)
        fwd, wg = lib.conv_kernel_name(4, n, d), lib.conv_kernel_name(5, n, d)
        want = 5 if vec else 2
        assert fwd.startswith("k_conv_fwd<") and fwd.endswith(f", {want}>"), fwd
        assert wg.startswith("k_conv_wgrad<") and wg.endswith(f", {want}>"), wg
    # the Nature-CNN conv1 keeps its strip-image kernels; activations in NHWC are not frames
    atari = _desc(4, 84, 84, 32)
    assert lib.conv_kernel_name(4, 77, atari) == "k_conv_u8_img_norm<2, 4, 5, 16>"
    assert lib.conv_kernel_name(5, 77, atari) == "k_conv1_wgrad_img_norm<2, 4>"
    assert not lib.conv_norm_supported(77, _desc(cin, h, w, cout, fmt=0))


# ------------------------------------------------------------------------------------------------ 2. kernels against float64
def _slab_case(cin, h, w, n, traj_T, use_index, g):
    """frames [rows, C, H, W] u8 on the GPU + (index, offset) + the [n, C, H, W] frames the launch reads"""
    rows = n + (n // traj_T + 2 if traj_T else 0) + 7
    frames = torch.randint(0, 256, (rows, cin, h, w), dtype=torch.uint8, generator=g).cuda()
    index = torch.randperm(n, generator=g).int().cuda() if use_index else None
    offset = 0 if use_index else 2
    dsel = index.long() if use_index else torch.arange(offset, offset + n, device="cuda")
    if traj_T:
        dsel = dsel + dsel // traj_T
    return frames, index, offset, frames[dsel]


def _tables(elems, g):
    """mu / rstd (f32, on the GPU) for pixels scaled to about [0, 1]: part of every frame clamps at +-5"""
    mu = (torch.rand(elems, generator=g) * 0.6 + 0.2).cuda()
    rstd = (1.0 / torch.sqrt(torch.rand(elems, generator=g) * 0.2 + 1e-3)).cuda()
    return mu, rstd


def _normalised64(x_u8, mu, rstd, shape):
    c, h, w = shape
    xn = (((x_u8.double() - SUB) * INV - mu.double().view(1, c, h, w)) * rstd.double().view(1, c, h, w)).clamp(-5, 5)
    share = float((xn.abs() == 5).double().mean())
    assert share > 1e-3, share  # the clamp is exercised
    return xn


def _conv_case(geom, n, traj_T, use_index, act, seed):
    """(fused errors, materialising-pair errors) of forward / weight gradient / bias gradient against float64, each as
    max|a - ref| / max|ref|"""
    cin, h, w, cout, vec = geom
    g = torch.Generator().manual_seed(seed)
    d = _desc(cin, h, w, cout, act=act, traj_T=traj_T)
    K, elems, P = cin * 64, cin * h * w, d.OH * d.OW
    frames, index, offset, x = _slab_case(cin, h, w, n, traj_T, use_index, g)
    mu, rstd = _tables(elems, g)
    wk = (torch.randn(K, cout, generator=g) / 16).cuda()          # frame order: k = (c*KH + kh)*KW + kw
    b = (torch.randn(cout, generator=g) * 0.1).cuda()
    dy = torch.randn((n * P, cout), generator=g).cuda()
    xn = _normalised64(x, mu, rstd, (cin, h, w))
    w4 = wk.double().t().reshape(cout, cin, 8, 8).clone().requires_grad_(True)
    b64 = b.double().clone().requires_grad_(True)
    pre = F.conv2d(xn, w4, b64, stride=4)
    ref = ACTS[act](pre).detach().permute(0, 2, 3, 1).reshape(n * P, cout)
    pre.backward(dy.double().reshape(n, d.OH, d.OW, cout).permute(0, 3, 1, 2))  # the LINEAR layer's gradient against dy
    gw_ref, gb_ref = w4.grad.reshape(cout, -1).t(), b64.grad

    def err(a, r):
        return float((a.double() - r).abs().max() / r.abs().max())

    assert lib.conv_norm_supported(n, d)
    out = torch.empty((n * P, cout), device="cuda")
    dw, db = torch.empty_like(wk), torch.empty_like(b)
    ws = torch.empty(lib.conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.conv_fwd_norm(frames, elems, index, offset, mu, rstd, wk, b, out, n, d)
    lib.conv_wgrad_norm(frames, elems, index, offset, mu, rstd, dy, dw, db, n, d, ws)
    fused = (err(out, ref), err(dw, gw_ref), err(db, gb_ref))
    dw1 = dw.clone()
    lib.conv_wgrad_norm(frames, elems, index, offset, mu, rstd, dy, dw, db, n, d, ws)
    assert torch.equal(dw, dw1)  # deterministic
    # the materialising pair on the same inputs: sf_obsnorm_apply, then sf_conv_fwd / sf_conv_wgrad on the f32 NHWC batch
    dm = _desc(cin, h, w, cout, act=act, fmt=0)
    xm = torch.empty((n, elems), device="cuda")
    lib.obsnorm_apply(frames, True, elems, index, offset, traj_T, n, elems, cin, h * w, SUB, INV, mu, rstd, xm)
    wm = wk.view(cin, 8, 8, cout).permute(1, 2, 0, 3).reshape(K, cout).contiguous()  # NHWC order: k = (kh*KW + kw)*Cin + c
    out_m, dw_m, db_m = torch.empty_like(out), torch.empty_like(wk), torch.empty_like(b)
    wsm = torch.empty(lib.conv_wgrad_workspace(n, dm), dtype=torch.uint8, device="cuda")
    lib.conv_fwd_raw(xm, elems, None, 0, wm, b, out_m, n, dm)
    lib.conv_wgrad_raw(xm, elems, None, 0, dy, dw_m, db_m, n, dm, wsm)
    gw_ref_m = gw_ref.reshape(cin, 8, 8, cout).permute(1, 2, 0, 3).reshape(K, cout)
    mat = (err(out_m, ref), err(dw_m, gw_ref_m), err(db_m, gb_ref))
    return fused, mat


def _check(fused, mat, what):
    """2e-6 (forward) / 5e-6 (gradients) of the largest reference entry; a longer reduction may take twice the error of the
    materialising pair on the same inputs (same f32 products, another summation order)"""
    print(f"{what}: fused fwd/dw/db {fused[0]:.3g} {fused[1]:.3g} {fused[2]:.3g}  materialised {mat[0]:.3g} {mat[1]:.3g} {mat[2]:.3g}")
    for e, m, fixed, nm in zip(fused, mat, (2e-6, 5e-6, 5e-6), ("forward", "weight gradient", "bias gradient")):
        assert e < max(fixed, 2.0 * m), (what, nm, e, m)


CASES = [(1, 0, False, 2), (77, 0, True, 3), (255, 5, False, 1), (130, 8, True, 2)]  # (n, traj_T, index?, activation)


@pytest.mark.parametrize("n,traj_T,use_index,act", CASES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_conv_fwd_wgrad_norm_on_u8_frames_vs_float64(geom, n, traj_T, use_index, act):
    """sf_conv_fwd_norm / sf_conv_wgrad_norm against F.conv2d on clamp(((x - s) * c - mu) * rstd, +-5) in float64: one
    sample, odd n, offset, index gather, slab rows (traj_T), obs_subtract_mean / obs_scale, tanh / elu / relu"""
    fused, mat = _conv_case(geom, n, traj_T, use_index, act, seed=geom[1] * 1000 + geom[2] + n)
    _check(fused, mat, f"{geom} n={n}")


def test_conv_wgrad_norm_at_a_training_size():
    """the first layer's weight gradient over a 2048-sample minibatch of 3x72x128 u8 frames (1 042 432 reduction rows)"""
    fused, mat = _conv_case(GEOMS[0], 2048, 0, False, 1, seed=11)
    _check(fused, mat, "3x72x128 n=2048")


# ------------------------------------------------------------------------------------------------ 3. resnet first layer
def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _close(got, ref, mat, atol, rtol, what):
    """|got - ref| <= atol + rtol |ref|; where that bound (set for inputs in [-0.07, 0.93]) does not hold for normalised
    pixels up to +-5: twice the largest error of the materialising pair on the same inputs"""
    e, em = (got - ref).abs(), float((mat - ref).abs().max())
    print(f"{what}: fused {float(e.max()):.3g} materialised {em:.3g}")
    tol = torch.clamp(atol + rtol * ref.abs(), min=2.0 * em)
    assert bool((e <= tol).all()), (what, float(e.max()), em)


@pytest.mark.parametrize("cin,h,w", [(4, 21, 19), (3, 13, 17), (1, 1, 2), (5, 6, 5)])
@pytest.mark.parametrize("mode", ["dense", "index", "traj"])
def test_res_conv_first_layer_u8_norm(cin, h, w, mode):
    """sf_res_conv_fwd_norm / sf_res_conv_wgrad_norm against float64 conv2d(padding=1) on the normalised frames; |mu * rstd|
    is a few units, so a padding tap that was normalised instead of left at zero is far outside the bound"""
    g = torch.Generator().manual_seed(cin + h + w)
    E, T, cout = 3, 4, 16
    slab = torch.randint(0, 256, (E, T + 1, cin, h, w), generator=g, dtype=torch.uint8)
    flat = slab[:, :T].reshape(E * T, cin, h, w)
    elems = cin * h * w
    d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=1, act_in=0, traj_T=0, sub_mean=SUB, inv_scale=INV)
    if mode == "dense":
        src, index, offset, ref_in = slab.reshape(-1, elems)[2:].cuda(), None, 0, slab.reshape(-1, cin, h, w)[2:9]
    elif mode == "index":
        rows = torch.tensor([5, 0, 9, 3, 3, 11], dtype=torch.int32)
        src, index, offset, ref_in = flat.reshape(-1).cuda(), rows.cuda(), 0, flat[rows.long()]
    else:
        d.traj_T = T
        src, index, offset, ref_in = slab.reshape(-1).cuda(), None, 3, flat[3:10]
    n = ref_in.shape[0]
    mu = (torch.rand(elems, generator=g) * 0.2 + 0.4)
    rstd = (torch.rand(elems, generator=g) * 8.0 + 4.0)
    assert float((mu * rstd).abs().min()) > 1.5
    xn = (((ref_in.double() - SUB) * INV - mu.double().view(1, cin, h, w)) * rstd.double().view(1, cin, h, w)).clamp(-5, 5)
    assert elems < 100 or ((xn.abs() == 5).any() and (xn.abs() < 5).any())  # (a frame of two pixels may not clamp)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.2
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    wr, br = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xn, wr, br, padding=1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    wc = wt.permute(2, 3, 1, 0).reshape(-1, cout).contiguous().float().cuda()
    bc, gyc, mt, rt = b.float().cuda(), _nhwc(gy).float().cuda(), mu.cuda(), rstd.cuda()
    out = torch.empty(n, h, w, cout, device="cuda")
    gw, gb = torch.empty(9 * cin, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(lib.res_conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.res_conv_fwd_norm(src, elems, index, offset, mt, rt, wc, bc, out, n, d)
    lib.res_conv_wgrad_norm(src, elems, index, offset, mt, rt, gyc, gw, gb, n, d, ws)
    gw1, gb1 = gw.clone(), gb.clone()
    lib.res_conv_wgrad_norm(src, elems, index, offset, mt, rt, gyc, gw, gb, n, d, ws)
    assert torch.equal(gw, gw1) and torch.equal(gb, gb1)
    # the materialising pair: sf_obsnorm_apply, then the f32 NHWC layer
    dm = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=0, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    xm = torch.empty((n, elems), device="cuda")
    lib.obsnorm_apply(src, True, elems, index, offset, d.traj_T, n, elems, cin, h * w, SUB, INV, mt, rt, xm)
    out_m, gw_m, gb_m = torch.empty_like(out), torch.empty_like(gw), torch.empty_like(gb)
    lib.res_conv_fwd(xm, elems, None, 0, wc, bc, out_m, n, dm)
    lib.res_conv_wgrad(xm, elems, None, 0, gyc, gw_m, gb_m, n, dm, ws)
    gw_ref = wr.grad.permute(2, 3, 1, 0).reshape(-1, cout)
    _close(_nchw(out).cpu().double(), y.detach(), _nchw(out_m).cpu().double(), 2e-4, 1e-4, "forward")
    _close(gw.cpu().double(), gw_ref, gw_m.cpu().double(), 2e-3, 1e-4, "weight gradient")
    _close(gb.cpu().double(), br.grad, gb_m.cpu().double(), 2e-3, 1e-4, "bias gradient")
    # the plain entry points refuse nothing new and the normalising ones need the raw-frame layer
    with pytest.raises(lib.SfHipError):
        lib.res_conv_fwd_norm(xm, elems, None, 0, mt, rt, wc, bc, out, n, dm)


# ------------------------------------------------------------------------------------------------ 4. models
MODELS = {  # name: (cfg overrides, image shape, extra vector key?)
    "convnet_simple": (dict(encoder_conv_architecture="convnet_simple"), (3, 36, 52), False),
    "convnet_impala": (dict(encoder_conv_architecture="convnet_impala"), (4, 84, 84), False),
    "resnet_impala": (dict(encoder_conv_architecture="resnet_impala"), (3, 36, 36), False),
    "two_keys": (dict(encoder_conv_architecture="convnet_simple", normalize_input_keys=["obs"], encoder_mlp_layers=[32]),
                 (3, 36, 52), True),
    "separate": (dict(encoder_conv_architecture="convnet_simple", actor_critic_share_weights=False), (3, 36, 52), False),
}


def _cfg(**over):
    from sample_factory_amd.cfg.arguments import default_cfg
    kw = dict(nonlinearity="elu", obs_scale=255.0, obs_subtract_mean=3.0, normalize_input=True, use_rnn=False,
              normalize_returns=False, encoder_conv_mlp_layers=[64])
    kw.update(over)
    cfg = default_cfg(**kw)
    cfg.dp_world = 1
    return cfg


def _space(shape, extra):
    from sample_factory_amd.envs import spaces
    d = {"obs": spaces.Box(0, 255, tuple(shape), np.uint8)}
    if extra:
        d["measurements"] = spaces.Box(-1, 1, (5,), np.float32)
    return spaces.Dict(d)


def _image_towers(ac):
    if hasattr(ac, "actor"):
        return _image_towers(ac.actor) + _image_towers(ac.critic)
    return [ac.encoders["obs"]] if hasattr(ac, "encoders") else [ac]


def _obs(shape, extra, lead, seed):
    g = torch.Generator().manual_seed(seed)
    o = {"obs": torch.randint(0, 256, tuple(lead) + tuple(shape), generator=g, dtype=torch.int32).to(torch.uint8).cuda()}
    if extra:
        o["measurements"] = (torch.rand(tuple(lead) + (5,), generator=g) * 2 - 1).cuda()
    return o


def _arg(ac, obs):
    return obs if getattr(ac, "multi_key", False) else obs["obs"]


def _no_apply(*a, **k):
    raise AssertionError("sf_obsnorm_apply ran: a normalised f32 copy of the frames was materialised")


@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_never_materialise_the_normalised_frames(name, tmp_path, monkeypatch):
    """a rollout forward and one Learner.train (statistics update, bootstrap forward, minibatches) with sf_obsnorm_apply
    replaced by a function that raises"""
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.algo.utils.shared_buffers import alloc_trajectory_tensors
    from sample_factory_amd.envs import spaces
    over, shape, extra = MODELS[name]
    E, T, A = 16, 4, 6
    cfg = _cfg(rollout=T, batch_size=E * T // 2, num_batches_per_epoch=2, num_epochs=1, seed=0, serial_mode=True,
               train_dir=str(tmp_path), experiment="t", **over)
    env_info = EnvInfo(_space(shape, extra), spaces.Discrete(A), E)
    monkeypatch.setattr(lib, "obsnorm_apply", _no_apply)
    pv = torch.zeros(1, dtype=torch.int32)
    learner = Learner(cfg, env_info, pv, 0, ParameterServer(0, pv))
    learner.init()
    ac = learner.actor_critic
    assert type(ac).__name__ in ("ActorCritic", "MultiKeyActorCritic", "SeparateActorCritic")
    towers = _image_towers(ac)
    assert towers and all(t._fused_norm and t.obs_normalizer is not None for t in towers)
    for t in towers:
        first = t.layers[0].desc if hasattr(t, "layers") else t.convs[0].desc
        assert first.in_u8 == 1  # the first layer keeps its raw-frame form
    g = torch.Generator().manual_seed(9)
    batch = alloc_trajectory_tensors(env_info, E, T, 1, "cuda")
    for k, v in _obs(shape, extra, (E, T + 1), 10).items():
        batch["obs"][k].copy_(v)
    logits = torch.randn((E, T, A), generator=g)
    actions = torch.randint(0, A, (E, T), generator=g)
    batch["action_logits"].copy_(logits)
    batch["actions"].copy_(actions.view(E, T, 1).float())
    batch["log_prob_actions"].copy_(torch.log_softmax(logits, -1).gather(-1, actions.view(E, T, 1)).view(E, T))
    batch["values"].copy_(torch.randn((E, T + 1), generator=g) * 0.1)
    batch["rewards"].copy_(torch.randn((E, T), generator=g))
    batch["dones"].copy_(torch.rand((E, T), generator=g) < 0.1)
    for k in ("policy_id", "policy_version", "time_outs", "rnn_states"):
        batch[k].zero_()
    batch["valids"].fill_(1)
    p0 = ac.flat_params.clone()
    ac.eval()
    res = ac.forward(_obs(shape, extra, (E,), 11))  # the rollout's forward
    assert torch.isfinite(res["values"]).all() and torch.isfinite(res["action_logits"]).all()
    stats = learner.train(batch)
    torch.cuda.synchronize()
    assert stats["learner_env_steps"] == E * T and learner.train_step == 2
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    assert float(ac.state_dict()["obs_normalizer.running_mean_std.running_mean_std.obs.count"]) > 1.0


@pytest.mark.parametrize("name", sorted(MODELS))
def test_fused_and_materialising_models_agree(name, monkeypatch):
    """the same model built with SF_CONV1_NORM off: heads of an inference pass and every parameter gradient of one training
    pass (dataset rows of an [E, T + 1, ...] slab) agree with the fused model"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    import sample_factory_amd.model.actor_critic as acm
    over, shape, extra = MODELS[name]
    cfg, space = _cfg(**over), _space(shape, extra)
    fused = create_actor_critic(cfg, space, spaces.Discrete(6), torch.device("cuda"))
    monkeypatch.setattr(acm, "_CONV1_NORM", False)
    mat = create_actor_critic(cfg, space, spaces.Discrete(6), torch.device("cuda"))
    monkeypatch.setattr(acm, "_CONV1_NORM", True)
    assert type(mat) is type(fused)
    assert all(t._fused_norm for t in _image_towers(fused)) and not any(t._fused_norm for t in _image_towers(mat))
    mat.load_state_dict(fused.state_dict(), strict=False)
    E, T = 12, 4
    obs = _obs(shape, extra, (E, T + 1), 21)
    n = E * T
    g = torch.Generator().manual_seed(22)
    g_heads = torch.zeros((n, fused.heads_ld), device="cuda")
    g_heads[:, :1 + fused.num_action_params] = torch.randn((n, 1 + fused.num_action_params), generator=g).cuda() / n
    outs = []
    for m in (fused, mat):
        m.obs_normalizer.update(_arg(m, obs), m.obs_elems, E * (T + 1))  # identical statistics on both
        m.train()
        m.flat_grads.zero_()
        acts = m.forward_heads(_arg(m, obs), n, sample_stride=m.obs_elems, index=None, offset=0, traj_T=T, tag="train")
        m.backward(acts, g_heads.clone(), _arg(m, obs), n, sample_stride=m.obs_elems, index=None, offset=0, traj_T=T)
        torch.cuda.synchronize()
        grads = m.flat_to_ref(m.flat_grads)
        m.eval()
        res = m.forward({k: v[:, 2].contiguous() for k, v in obs.items()})
        outs.append((grads, res["action_logits"].clone(), res["values"].clone()))
    np.testing.assert_allclose(outs[0][1].cpu().numpy(), outs[1][1].cpu().numpy(), atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(outs[0][2].cpu().numpy(), outs[1][2].cpu().numpy(), atol=2e-5, rtol=1e-4)
    for pname, _ in fused.ref_param_shapes():
        a, b = outs[0][0][pname].numpy(), outs[1][0][pname].numpy()
        scale = float(np.abs(b).max())
        assert scale > 0, f"{pname}: the materialising path's gradient is zero — the check would be vacuous"
        assert np.abs(a - b).max() <= 2e-4 * scale + 1e-7, (pname, float(np.abs(a - b).max()), scale)


# ------------------------------------------------------------------------------------------------ 5. replay of the reference
def test_learner_train_matches_reference_u8norm(tmp_path, monkeypatch):
    """the reference's Learner.train (tests/golden/train_u8norm.npz): 16 x 8 on 3x36x52 u8 frames, convnet_simple,
    normalize_input=True, 2 minibatches read in place from the slab, invalid rows; first SGD step against the reference's
    float64 run, the post-training state against its fp32 run; sf_obsnorm_apply must not run"""
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.actor_critic import ActorCritic
    from oracle.weights import seeded_state
    from tests.parity_util import compare_post_train
    from tests.test_gpu_nn import TIGHT
    from tests.test_gpu_parity_c2_c5 import _first_step_gradient, _load_batch
    name = "u8norm"
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"train_{name}.npz"), allow_pickle=True)
    E, T, A, nb = int(g["E"]), int(g["T"]), int(g["A"]), int(g["num_batches"])
    cfg = _cfg(encoder_conv_architecture="convnet_simple", obs_subtract_mean=0.0, rollout=T, batch_size=E * T // nb,
               num_batches_per_epoch=nb, num_epochs=int(g["num_epochs"]), seed=0, exploration_loss_coeff=0.01,
               serial_mode=True, train_dir=str(tmp_path), experiment="t", record_grad_norm=True, normalize_returns=True,
               recurrence=1)
    env_info = EnvInfo(_space((3, 36, 52), False), spaces.Discrete(A), E)
    st = seeded_state([(str(n), ast.literal_eval(str(s))) for n, s in zip(g["param_names"], g["param_shapes"])],
                      int(g["param_seed"]))

    def make_learner():
        pv = torch.zeros(1, dtype=torch.int32)
        ln = Learner(cfg, env_info, pv, 0, ParameterServer(0, pv))
        ln.init()
        ln.actor_critic.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
        return ln

    monkeypatch.setattr(lib, "obsnorm_apply", _no_apply)
    batch = _load_batch(g, env_info, E, T, 1)
    assert batch["obs"]["obs"].dtype == torch.uint8
    assert int((torch.from_numpy(g["in_policy_id"]) != 0).sum()) > 0  # the replay has invalid rows
    _first_step_gradient(make_learner, g, batch, name, bound=5e-4)
    learner = make_learner()
    ac = learner.actor_critic
    assert isinstance(ac, ActorCritic) and ac._fused_norm and ac.layers[0].desc.in_u8 == 1
    assert [n for n, _ in ac.ref_param_shapes()] == [str(n) for n in g["param_names"]]
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    stats = learner.train(batch)
    torch.cuda.synchronize()
    assert stats["learner_env_steps"] == int(g["env_steps"]) and learner.train_step == int(g["train_step"])
    np.testing.assert_allclose(ac.returns_normalizer.stats.cpu().numpy(), g["out_rms"], rtol=1e-5)
    compare_post_train(learner, g, before, name, **TIGHT)
    sub = int(g["subsample"])
    sd = ac.state_dict()
    pfx = "obs_normalizer.running_mean_std.running_mean_std.obs."
    assert sd[pfx + "running_mean"].shape == (3, 36, 52) and sd[pfx + "running_mean"].dtype == torch.float64
    np.testing.assert_allclose(sd[pfx + "running_mean"].reshape(-1)[::sub].numpy(), g["obsn_mean"], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(sd[pfx + "running_var"].reshape(-1)[::sub].numpy(), g["obsn_var"], rtol=1e-5, atol=1e-7)
    assert float(sd[pfx + "count"]) == float(g["obsn_count"])
    ac.eval()
    res = ac.forward({"obs": batch["obs"]["obs"][:, 0].contiguous()}, None)
    np.testing.assert_allclose(res["action_logits"].cpu().numpy(), g["eval_logits"], atol=2e-4, rtol=2e-3)
    np.testing.assert_allclose(res["values"].cpu().numpy(), g["eval_values"], atol=2e-4, rtol=2e-3)


# ------------------------------------------------------------------------------------------------ 6. async, odd addresses, programs
@pytest.mark.parametrize("name", ["convnet_simple", "resnet_impala"])
def test_inference_reads_the_published_tables_until_the_next_publish(name):
    """async mode: the learner updates the normaliser's tables in place; a rollout forward keeps the published pair"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    over, shape, extra = MODELS[name]
    ac = create_actor_critic(_cfg(**over), _space(shape, extra), spaces.Discrete(6), torch.device("cuda"))
    tower = _image_towers(ac)[0]
    E = 16
    first, second, probe = _obs(shape, extra, (E, 3), 31), _obs(shape, extra, (E, 3), 32), _obs(shape, extra, (E,), 33)
    second["obs"] //= 3  # other statistics
    ac.obs_normalizer.update(_arg(ac, first), ac.obs_elems, E * 3)
    ac.enable_weight_snapshots()
    ac.publish_weights(0)
    ac.snap_read = 0
    ac.eval()

    def heads(tag):
        return ac.forward_heads(_arg(ac, probe), E, sample_stride=0 if getattr(ac, "multi_key", False) else ac.obs_elems,
                                tag=tag)[-1].clone()

    h_pub = heads("inf")
    assert torch.equal(h_pub, heads("boot"))  # published == live so far
    key0, ptr0 = ac.launch_key("inf"), tower.obs_normalizer.mu_tab.data_ptr()  # (every buffer of both passes exists now)
    mu_before = tower.obs_normalizer.mu_tab.clone()
    ac.obs_normalizer.update(_arg(ac, second), ac.obs_elems, E * 3)  # the learner moves on
    assert not torch.equal(mu_before, tower.obs_normalizer.mu_tab)
    assert torch.equal(tower._snap_tabs[0][0], mu_before)
    assert tower.obs_normalizer.mu_tab.data_ptr() == ptr0 and ac.launch_key("inf") == key0  # in place: programs stay valid
    assert torch.equal(heads("inf"), h_pub)
    h_live = heads("boot")
    assert not torch.equal(h_live, h_pub)
    ac.publish_weights(1)
    ac.snap_read = 1
    assert ac.launch_key("inf") != key0  # another slot: a recorded program is not replayed, it is recorded again
    assert torch.equal(heads("inf"), h_live)


@pytest.mark.parametrize("name,shape", [("convnet_simple", (3, 36, 52)), ("convnet_simple", (3, 45, 53)),
                                        ("resnet_impala", (3, 36, 36))])
def test_frames_at_an_odd_address_give_the_same_heads(name, shape):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    ac = create_actor_critic(_cfg(**MODELS[name][0]), _space(shape, False), spaces.Discrete(6), torch.device("cuda"))
    n, elems = 24, int(np.prod(shape))
    obs = _obs(shape, False, (n,), 41)["obs"]
    ac.obs_normalizer.update(_arg(ac, {"obs": obs}), ac.obs_elems, n)
    ac.eval()
    a = ac.forward({"obs": obs})["action_logits"].clone()
    buf = torch.empty(n * elems + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view((n,) + tuple(shape))
    view.copy_(obs)
    assert view.data_ptr() % 4 == 1
    b = ac.forward({"obs": view})["action_logits"].clone()
    assert torch.isfinite(a).all()
    np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("arch", ["convnet_impala", "resnet_impala"])
def test_fused_norm_rollouts_replayed_as_programs_equal_the_wrapper_path(arch):
    """5 iterations (rollout + train, the normaliser's tables updated in place by every train) of a fused-norm model on the
    synthetic 4x84x84 u8 env: the replayed run is the wrapper-path run bit for bit"""
    from tests.test_gpu_launch_programs import _run, _same_run
    kw = dict(encoder_conv_architecture=arch, encoder_conv_mlp_layers=[64])
    plain = _run("conv_normalized", False, 5, **kw)
    prog = _run("conv_normalized", True, 5, **kw)
    _same_run(plain, prog)
    ac = prog["samplers"][0].ac
    assert all(t._fused_norm for t in _image_towers(ac))
    for s in prog["samplers"]:
        progs = [p for p in s._progs.values() if isinstance(p, lib.LaunchProgram)]
        assert progs and all(p.unsafe is None for p in progs)
        assert s.program_replays >= s.T, s.program_replays
        names = [c[2] for k, p in s._progs.items() if k[0] == "policy" for c in p.calls]
        assert "sf_obsnorm_apply" not in names
        assert ("sf_res_conv_fwd_norm" if arch == "resnet_impala" else "sf_conv_fwd_norm") in names
