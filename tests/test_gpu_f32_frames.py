"""float32 CHW image observations on the native kernels (sf_conv_desc.in_u8 = 2): the first conv layer reads the f32 frames
in place from the trajectory slab, (x - sub_mean) * inv_scale and the observation normaliser formed in its loader.  Every
kernel mode against float64 torch, the model against the reference's forward (tests/golden/model_fwd_f32frames.npz) and
Learner.train (tests/golden/train_f32frames*.npz), and the runtime: launch programs, async snapshots, data parallelism and
checkpoints."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "model_fwd_f32frames.npz"), allow_pickle=True)
CASES = [str(c) for c in G["cases"]]
ACTS = {0: lambda x: x, 1: F.relu, 2: torch.tanh, 3: F.elu}


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _w_frame(w):  # OIHW -> [(c*KH + kh)*KW + kw, Cout]
    return w.reshape(w.shape[0], -1).t().contiguous()


def _desc(cin, h, w, cout, k, s, act=1, mean=0.0, inv_scale=1.0, traj_T=0):
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    return lib.sf_conv_desc(Cin=cin, H=h, W=w, Cout=cout, KH=k, KW=k, stride=s, OH=oh, OW=ow, in_u8=lib.IN_F32_FRAME,
                            relu=act, traj_T=traj_T, sub_mean=mean, inv_scale=inv_scale)


def _frames_case(cin, h, w, mode, g):
    """(device source, index, offset, in_sample_stride, traj_T, float64 reference batch [n, C, H, W])"""
    E, T, elems = 3, 5, cin * h * w
    slab = torch.rand((E, T + 1, cin, h, w), generator=g) * 3.0 - 1.0
    flat = slab[:, :T].reshape(E * T, cin, h, w)  # dataset row d = e*T + t
    if mode == "dense":
        return slab.reshape(-1, elems)[2:].cuda(), None, 0, elems, 0, slab.reshape(-1, cin, h, w)[2:12].double()
    if mode == "index":
        rows = torch.tensor([5, 0, 14, 3, 3, 11, 7], dtype=torch.int32)
        return flat.reshape(-1).cuda(), rows.cuda(), 0, elems, 0, flat[rows.long()].double()
    if mode == "traj":
        return slab.reshape(-1).cuda(), None, 3, elems, T, flat[3:12].double()
    # strided: 4 extra floats between samples (the vector loader still applies), offset into the buffer
    pad = torch.rand((E * T, elems + 4), generator=g)
    pad[:, :elems] = flat.reshape(E * T, elems)
    return pad.reshape(-1).cuda(), None, 2, elems + 4, 0, flat[2:11].double()


GEOMS = [  # (Cin, H, W, Cout, K, S, vector loader)
    (4, 84, 84, 32, 8, 4, True),
    (3, 36, 36, 16, 8, 4, True),
    (1, 45, 53, 32, 8, 4, False),   # W % 4 != 0: scalar loader
    (3, 13, 17, 16, 4, 2, False),   # stride 2: scalar loader
]


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("mode", ["dense", "index", "traj", "strided"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g[:3])))
def test_conv_fwd_wgrad_on_f32_frames(geom, mode, norm):
    cin, h, w, cout, k, s, vec = geom
    g = torch.Generator().manual_seed(cin * 1000 + h + w + (7 if norm else 0))
    src, index, offset, stride, traj_T, x = _frames_case(cin, h, w, mode, g)
    n, elems = x.shape[0], cin * h * w
    mean, scale = 0.25, 0.5
    inv = float(np.float32(1.0 / scale))
    d = _desc(cin, h, w, cout, k, s, act=1, mean=mean, inv_scale=inv, traj_T=traj_T)
    xn = (x - mean) * inv
    if norm:  # tables that push part of the frame beyond +-5 (the clamp)
        mu = (torch.rand(elems, generator=g, dtype=torch.float64) - 0.5)
        rstd = torch.rand(elems, generator=g, dtype=torch.float64) * 12.0 + 0.1
        mu32, rstd32 = mu.float(), rstd.float()
        xn = ((xn - mu32.double().view(1, cin, h, w)) * rstd32.double().view(1, cin, h, w)).clamp(-5, 5)
        assert (xn.abs() == 5).any() and (xn.abs() < 5).any()
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    xr = xn.clone()
    wr, br = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br, stride=s)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    wc, bc = _w_frame(wt).float().cuda(), b.float().cuda()
    out = torch.empty(n * d.OH * d.OW, cout, device="cuda")
    gw, gb = torch.empty(cin * k * k, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(lib.conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    gyc = gy.permute(0, 2, 3, 1).reshape(-1, cout).float().cuda()
    if norm:
        assert lib.conv_norm_supported(n, d)
        mt, rt = mu32.cuda(), rstd32.cuda()
        lib.conv_fwd_norm(src, stride, index, offset, mt, rt, wc, bc, out, n, d)
        lib.conv_wgrad_norm(src, stride, index, offset, mt, rt, gyc, gw, gb, n, d, ws)
        names = lib.conv_kernel_name(4, n, d), lib.conv_kernel_name(5, n, d)
    else:
        lib.conv_fwd_raw(src, stride, index, offset, wc, bc, out, n, d)
        lib.conv_wgrad_raw(src, stride, index, offset, gyc, gw, gb, n, d, ws)
        names = lib.conv_kernel_name(0, n, d), lib.conv_kernel_name(1, n, d)
    want_mode = (4 if norm else 3) if vec else 2
    assert all(nm.startswith(("k_conv_fwd<", "k_conv_wgrad<")) and nm.endswith(f", {want_mode}>") for nm in names), names
    ref = F.relu(y.detach())
    np.testing.assert_allclose(_nchw(out.view(n, d.OH, d.OW, cout)).cpu().double(), ref, atol=2e-4, rtol=1e-4)
    scale_w = float(wr.grad.abs().max())
    np.testing.assert_allclose(gw.cpu().double(), _w_frame(wr.grad), atol=2e-5 * scale_w + 1e-5, rtol=1e-4)
    np.testing.assert_allclose(gb.cpu().double(), br.grad, atol=1e-4, rtol=1e-4)
    gw1 = gw.clone()
    if norm:
        lib.conv_wgrad_norm(src, stride, index, offset, mt, rt, gyc, gw, gb, n, d, ws)
    else:
        lib.conv_wgrad_raw(src, stride, index, offset, gyc, gw, gb, n, d, ws)
    assert torch.equal(gw, gw1)  # deterministic


def test_f32_frames_refused_by_every_other_family():
    """format 2 is taken by the register-staged fp32 kernels only: every fast family's query answers 0, the data gradient
    refuses it, the misaligned-table and out-of-range cases are reported"""
    for n in (1, 256, 4096):
        d = _desc(4, 84, 84, 32, 8, 4)
        assert not lib.conv_relu_mask_supported(n, d)
        assert not lib.conv_fwd_t_supported(n, d)
        assert lib.conv_fwd_t_workspace(n, d) == 0
        assert lib.conv_norm_supported(n, d)
        assert lib.conv_kernel_name(0, n, d).endswith(", 3>")
        assert lib.conv_kernel_name(1, n, d).endswith(", 3>")
        assert lib.conv_kernel_name(4, n, d).endswith(", 4>")
    d = _desc(4, 84, 84, 32, 8, 4)
    with pytest.raises(lib.SfHipError):
        lib.conv_dgrad(torch.zeros(20 * 20 * 32, device="cuda"), torch.zeros(256, 32, device="cuda"), None,
                       torch.zeros(4 * 84 * 84, device="cuda"), 1, d)
    bad = _desc(4, 84, 84, 32, 8, 4)
    bad.in_u8 = 3
    assert not lib.conv_norm_supported(1, bad)
    with pytest.raises(lib.SfHipError):
        lib.conv_fwd_raw(torch.zeros(4 * 84 * 84, device="cuda"), 4 * 84 * 84, None, 0, torch.zeros(256, 32, device="cuda"),
                         None, torch.zeros(400, 32, device="cuda"), 1, bad)
    # the u8 families are unchanged
    u8 = _desc(4, 84, 84, 32, 8, 4)
    u8.in_u8 = lib.IN_U8_FRAME
    assert lib.conv_relu_mask_supported(4096, u8) and lib.conv_norm_supported(4096, u8)
    assert lib.conv_kernel_name(4, 4096, u8) == "k_conv_u8_img_norm<2, 4, 5, 16>"


def test_f32_frames_wgrad_precision_at_a_training_size():
    """conv1's weight gradient over a 2048-sample minibatch of 4x84x84 f32 frames (819 200 reduction rows)"""
    n, cin, h, w, cout = 2048, 4, 84, 84, 32
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand((n, cin, h, w), generator=g, device="cuda")
    d = _desc(cin, h, w, cout, 8, 4, mean=0.5, inv_scale=2.0)
    gy = torch.randn((n, d.OH, d.OW, cout), generator=g, device="cuda")
    gw, gb = torch.empty(cin * 64, cout, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(lib.conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.conv_wgrad_raw(x, cin * h * w, None, 0, gy, gw, gb, n, d, ws)
    xd = (x.double() - 0.5) * 2.0
    ref = torch.nn.grad.conv2d_weight(xd, (cout, cin, 8, 8), _nchw(gy).double(), stride=4)
    err = float((gw.double() - _w_frame(ref)).abs().max() / ref.abs().max())
    berr = float((gb.double() - gy.double().sum((0, 1, 2))).abs().max() / float(gy.double().abs().sum((0, 1, 2)).max()))
    assert err < 2e-5 and berr < 2e-6, (err, berr)


# ------------------------------------------------------------------------------------------------ model
def _cfg(tag=None, **over):
    from sample_factory_amd.cfg.arguments import default_cfg
    kw = dict(encoder_conv_architecture="convnet_simple", nonlinearity="elu", obs_scale=1.0, obs_subtract_mean=0.0,
              normalize_input=False, use_rnn=False, normalize_returns=False)
    if tag is not None:
        kw.update(encoder_conv_architecture=str(G[f"{tag}_arch"]), nonlinearity=str(G[f"{tag}_nonlinearity"]),
                  obs_scale=float(G[f"{tag}_scale"]), obs_subtract_mean=float(G[f"{tag}_sub_mean"]))
    kw.update(over)
    cfg = default_cfg(**kw)
    cfg.dp_world = 1
    return cfg


def _space(shape, dtype=np.float32, extra=False):
    from sample_factory_amd.envs import spaces
    d = {"obs": spaces.Box(0, 1, tuple(shape), dtype)}
    if extra:
        d["measurements"] = spaces.Box(-1, 1, (5,), np.float32)
    return spaces.Dict(d)


def _seeded(tag):
    from oracle.weights import seeded_state
    shapes = [(str(n), ast.literal_eval(str(s))) for n, s in zip(G[f"{tag}_param_names"], G[f"{tag}_param_shapes"])]
    return {k: torch.from_numpy(v) for k, v in seeded_state(shapes, int(G[f"{tag}_param_seed"])).items()}


@pytest.mark.parametrize("tag", CASES)
def test_native_forward_matches_reference(tag):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.actor_critic import ActorCritic
    from sample_factory_amd.model.model_factory import create_actor_critic
    obs = G[f"{tag}_obs"]
    ac = create_actor_critic(_cfg(tag), _space(obs.shape[1:]), spaces.Discrete(6), torch.device("cuda"))
    assert isinstance(ac, ActorCritic) and ac.layers[0].kind == "conv_f32frame"
    assert ac.layers[0].desc.in_u8 == lib.IN_F32_FRAME
    ac.load_state_dict(_seeded(tag), strict=True)
    assert [n for n, _ in ac.ref_param_shapes()] == [str(n) for n in G[f"{tag}_param_names"]]
    sd = ac.state_dict()  # the reference's layout comes back out
    for k, v in _seeded(tag).items():
        assert torch.equal(sd[k], v.float()), k
    ac.eval()
    res = ac.forward({"obs": torch.from_numpy(obs).cuda()})
    np.testing.assert_allclose(res["action_logits"].cpu().numpy(), G[f"{tag}_action_logits"], atol=5e-5, rtol=1e-4)
    np.testing.assert_allclose(res["values"].cpu().numpy(), G[f"{tag}_values"], atol=5e-5, rtol=1e-4)
    conv0 = ac._ctx["inf"]["acts"][0]
    d = ac.layers[0].desc
    pre = _nchw(conv0.view(obs.shape[0], d.OH, d.OW, d.Cout)).cpu().numpy()
    want = ACTS[d.relu](torch.from_numpy(G[f"{tag}_conv0_preact_sample"])).numpy()
    np.testing.assert_allclose(pre[:, :, ::2, ::2], want, atol=2e-5, rtol=1e-4)


def test_factory_returns_native_models_for_f32_images():
    """single key, several keys and separate actor / critic weights on f32 frames: native; float64 frames: the torch path"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.actor_critic import ActorCritic
    from sample_factory_amd.model.actor_critic_multikey import MultiKeyActorCritic
    from sample_factory_amd.model.actor_critic_separate import SeparateActorCritic
    from sample_factory_amd.model.model_factory import create_actor_critic
    from sample_factory_amd.model.torch_policy import TorchPolicyAdapter
    dev, A = torch.device("cuda"), spaces.Discrete(6)
    assert isinstance(create_actor_critic(_cfg(), _space((3, 36, 36)), A, dev), ActorCritic)
    mk = create_actor_critic(_cfg(encoder_conv_mlp_layers=[32], encoder_mlp_layers=[32]), _space((3, 36, 36), extra=True),
                             A, dev)
    assert isinstance(mk, MultiKeyActorCritic) and mk.encoders["obs"].layers[0].kind == "conv_f32frame"
    sep = create_actor_critic(_cfg(actor_critic_share_weights=False), _space((3, 36, 36)), A, dev)
    assert isinstance(sep, SeparateActorCritic) and sep.actor.layers[0].kind == "conv_f32frame"
    sep_mk = create_actor_critic(_cfg(actor_critic_share_weights=False, encoder_conv_mlp_layers=[32],
                                      encoder_mlp_layers=[32]), _space((3, 36, 36), extra=True), A, dev)
    assert isinstance(sep_mk, SeparateActorCritic)
    for ac in (mk, sep, sep_mk):
        x = {"obs": torch.rand(6, 3, 36, 36, device="cuda")}
        if ac is not sep:
            x["measurements"] = torch.rand(6, 5, device="cuda")
        ac.eval()
        res = ac.forward(x if getattr(ac, "multi_key", False) else x["obs"])
        assert torch.isfinite(res["values"]).all() and torch.isfinite(res["action_logits"]).all()
    # refused image dtypes fall back instead of raising
    for dt in (np.float64, np.float16):
        ac = create_actor_critic(_cfg(), _space((3, 36, 36), dtype=dt), A, dev)
        assert isinstance(ac, TorchPolicyAdapter)
        ac = create_actor_critic(_cfg(actor_critic_share_weights=False), _space((3, 36, 36), dtype=dt), A, dev)
        assert isinstance(ac, TorchPolicyAdapter)


def test_normalize_input_fused_and_materialised_agree(monkeypatch):
    """normalize_input=True: the fused loader (sf_conv_fwd_norm) and the materialising path give the same forward; a frame
    view off the 16-byte grid is gathered into an aligned copy"""
    from sample_factory_amd.envs import spaces
    import sample_factory_amd.model.actor_critic as acm
    cfg = _cfg(normalize_input=True, obs_subtract_mean=0.25, obs_scale=0.5)
    space = _space((4, 36, 36))
    fused = acm.ActorCritic(cfg, space, spaces.Discrete(6), "cuda")
    assert fused._fused_norm
    monkeypatch.setattr(acm, "_CONV1_NORM", False)
    mat = acm.ActorCritic(cfg, space, spaces.Discrete(6), "cuda")
    assert not mat._fused_norm
    mat.load_state_dict(fused.state_dict(), strict=False)
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.rand((64, 4, 36, 36), generator=g, device="cuda")
    for m in (fused, mat):  # identical statistics on both
        m.obs_normalizer.update(obs, 4 * 36 * 36, 64)
    a = fused.forward(obs)["action_logits"].clone()
    b = mat.forward(obs)["action_logits"].clone()
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=2e-5, rtol=1e-4)
    buf = torch.empty(64 * 4 * 36 * 36 + 1, device="cuda")
    view = buf[1:].view(64, 4, 36, 36)  # 4 bytes off the 16-byte grid
    view.copy_(obs)
    c = fused.forward(view)["action_logits"].clone()
    np.testing.assert_allclose(c.cpu().numpy(), a.cpu().numpy(), atol=1e-6, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ Learner.train replays
@pytest.mark.parametrize("name", ["f32frames", "f32frames_norm", "f32frames_gru"])
def test_learner_train_matches_reference_f32frames(tmp_path, name):
    """the reference's Learner.train (tests/golden/train_f32frames*.npz): 16 x 8 on 3x36x36 f32 frames, 2 minibatches read
    in place from the slab through the index / traj_T addressing, invalid rows; first SGD step against the reference's
    float64 run, Adam moments / deltas / gradient norms against its fp32 run, deltas against its float64 run"""
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.actor_critic import ActorCritic, get_rnn_size
    from tests.parity_util import compare_post_train
    from tests.test_gpu_parity_c2_c5 import _deltas_vs_float64, _first_step_gradient, _load_batch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"train_{name}.npz"), allow_pickle=True)
    E, T, A, nb = int(g["E"]), int(g["T"]), int(g["A"]), int(g["num_batches"])
    rnn = dict(use_rnn=True, rnn_type="gru", rnn_size=32, recurrence=8) if name == "f32frames_gru" else dict(use_rnn=False,
                                                                                                             recurrence=1)
    cfg = _cfg(encoder_conv_mlp_layers=[64], normalize_input=name == "f32frames_norm", rollout=T, batch_size=E * T // nb,
               num_batches_per_epoch=nb, num_epochs=int(g["num_epochs"]), seed=0, exploration_loss_coeff=0.01,
               serial_mode=True, train_dir=str(tmp_path), experiment="t", record_grad_norm=True,
               normalize_returns=True, **rnn)
    obs_space = _space((3, 36, 36))
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
    assert batch["obs"]["obs"].dtype == torch.float32
    assert int((torch.from_numpy(g["in_policy_id"]) != 0).sum()) > 0  # the replay has invalid rows
    _first_step_gradient(make_learner, g, batch, name, bound=5e-4)
    learner = make_learner()
    ac = learner.actor_critic
    assert isinstance(ac, ActorCritic) and ac.layers[0].kind == "conv_f32frame"
    assert ac._fused_norm == (name == "f32frames_norm")
    assert [n for n, _ in ac.ref_param_shapes()] == [str(n) for n in g["param_names"]]
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    stats = learner.train(batch)
    torch.cuda.synchronize()
    assert stats["learner_env_steps"] == int(g["env_steps"]) and learner.train_step == int(g["train_step"])
    np.testing.assert_allclose(ac.returns_normalizer.stats.cpu().numpy(), g["out_rms"], rtol=1e-5)
    if name == "f32frames_norm":
        sub = int(g["subsample"])
        sd = ac.state_dict()
        pfx = "obs_normalizer.running_mean_std.running_mean_std.obs."
        np.testing.assert_allclose(sd[pfx + "running_mean"].reshape(-1)[::sub].numpy(), g["obsn_mean"], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(sd[pfx + "running_var"].reshape(-1)[::sub].numpy(), g["obsn_var"], rtol=1e-5, atol=1e-7)
    compare_post_train(learner, g, before, name, m_rtol=5e-4, v_rtol=1e-3, d_rtol=1e-3, gn_rtol=2e-4)
    _deltas_vs_float64(ac, g, before, None, name, tight=5e-4, flipped=5e-4, vs_ref32=1.5)


# ------------------------------------------------------------------------------------------------ end to end
class F32FrameBanditEnv:
    """GPU vector env with float32 [C, H, W] frames in [0, 1] (the frames a user env emits after scaling its pixels); the
    rewarded action is drawn per step and painted into channel 0 as a bright row, so a policy can learn it"""

    def __init__(self, num_agents=64, num_actions=4, shape=(3, 36, 36), seed=0, extra=False):
        from sample_factory_amd.envs import spaces
        self.num_agents, self.A, self.shape, self.extra = int(num_agents), int(num_actions), tuple(shape), extra
        d = {"obs": spaces.Box(0, 1, self.shape, np.float32)}
        if extra:
            d["measurements"] = spaces.Box(0, 1, (self.A,), np.float32)
        self.observation_space = spaces.Dict(d)
        self.action_space = spaces.Discrete(self.A)
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(int(seed))
        self._draw()

    def _draw(self):
        self.target = torch.randint(0, self.A, (self.num_agents,), generator=self.gen, device="cuda")
        self.img = torch.rand((self.num_agents,) + self.shape, generator=self.gen, device="cuda") * 0.5
        self.img[torch.arange(self.num_agents, device="cuda"), 0, self.target] = 1.0

    def _out(self):
        o = {"obs": self.img}
        if self.extra:
            o["measurements"] = F.one_hot(self.target, self.A).float()
        return o

    def reset(self, **kwargs):
        self._draw()
        return self._out(), {}

    def step(self, actions):
        a = torch.as_tensor(actions, device="cuda").reshape(-1).long()
        rew = (a == self.target).float()
        term = torch.ones(self.num_agents, dtype=torch.bool, device="cuda")
        self._draw()
        return self._out(), rew, term, torch.zeros_like(term), {}

    def close(self):
        pass


def _register():
    from sample_factory_amd.envs.env_utils import register_env

    def make(full_env_name, cfg=None, env_config=None, render_mode=None):
        n = getattr(cfg, "synthetic_num_agents", 64) if cfg is not None else 64
        seed = (getattr(cfg, "seed", None) or 0) if cfg is not None else 0
        return F32FrameBanditEnv(num_agents=n, seed=seed, extra=full_env_name.endswith("_dict"))

    register_env("f32frame_bandit", make)
    register_env("f32frame_bandit_dict", make)


_F32 = dict(env="f32frame_bandit", encoder_conv_architecture="convnet_simple", nonlinearity="relu", obs_scale=1.0,
            encoder_conv_mlp_layers=[64], use_rnn=False, synthetic_num_agents=64, batch_size=256)


@pytest.mark.parametrize("over", [dict(normalize_input=False), dict(normalize_input=True),
                                  dict(env="f32frame_bandit_dict", normalize_input=True, encoder_mlp_layers=[32])],
                         ids=["plain", "norm", "multikey"])
def test_f32_frames_replayed_rollouts_equal_the_wrapper_path(over):
    """rollout steps of an f32-frame model replayed as launch programs: the same run bit for bit as the wrapper path"""
    from tests.test_gpu_launch_programs import _run, _same_run
    _register()
    kw = dict(_F32, **over)
    plain = _run("conv_discrete", False, 5, **kw)
    prog = _run("conv_discrete", True, 5, **kw)
    _same_run(plain, prog)
    ac = prog["samplers"][0].ac
    tower = ac.encoders["obs"] if hasattr(ac, "encoders") else ac
    assert tower.layers[0].kind == "conv_f32frame"
    for s in prog["samplers"]:
        progs = [p for p in s._progs.values() if isinstance(p, lib.LaunchProgram)]
        assert progs and all(p.unsafe is None for p in progs)
        assert s.program_replays >= s.T, s.program_replays


def test_f32_frames_async_with_weight_snapshots():
    """async mode with normalize_input: inference reads the published weights and normaliser tables"""
    from tests.test_gpu_launch_programs import _run
    _register()
    kw = dict(_F32, async_rl=True, serial_mode=False, num_batches_to_accumulate=2, normalize_input=True)
    out = _run("conv_discrete", True, 6, **kw)
    ac = out["samplers"][0].ac
    assert ac.layers[0].kind == "conv_f32frame" and ac._snap is not None and ac._snap_tabs is not None
    assert sum(out["steps"]) > 0
    for k, v in out["slabs"][-1].items():
        assert torch.isfinite(v.float()).all(), k
    assert torch.isfinite(out["params"]).all()


def test_f32_frames_training_and_checkpoint_in_reference_layout(tmp_path):
    """a few sync iterations learn; the checkpoint holds the reference's names / shapes and loads into the reference's
    architecture (the torch construction of the same cfg) and back into a fresh native model"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.model.actor_critic import ActorCritic
    from sample_factory_amd.model.model_factory import create_actor_critic
    from sample_factory_amd.model.torch_policy import TorchPolicyAdapter
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.train import make_runner
    _register()
    cfg = default_cfg(**dict(_F32, rollout=8, num_batches_per_epoch=2, num_epochs=1, num_workers=1, num_envs_per_worker=1,
                             async_rl=False, seed=0, serial_mode=True, normalize_input=True, learning_rate=1e-3))
    cfg, runner = make_runner(cfg)
    runner.init()
    ac = runner.learner.actor_critic
    assert isinstance(ac, ActorCritic) and ac.layers[0].kind == "conv_f32frame"
    p0 = ac.flat_params.clone()
    for _ in range(3):
        stats = runner.iteration()
    torch.cuda.synchronize()
    assert np.isfinite(stats["train"]["loss"])
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(ac.flat_params, p0)
    sd = ac.state_dict()
    path = os.path.join(str(tmp_path), "ckpt.pth")
    torch.save(sd, path)
    loaded = torch.load(path)
    # the reference's architecture in torch (the same cfg on the torch path) takes the checkpoint as it stands
    os.environ["SF_NATIVE_F32FRAMES"] = "0"
    try:
        ref = create_actor_critic(cfg, ac.obs_space, ac.action_space, torch.device("cuda"))
    finally:
        del os.environ["SF_NATIVE_F32FRAMES"]
    assert isinstance(ref, TorchPolicyAdapter)
    assert [(k, tuple(s)) for k, s in ref.ref_param_shapes()] == [(k, tuple(s)) for k, s in ac.ref_param_shapes()]
    ref.load_state_dict(loaded, strict=True)
    obs = torch.rand(8, 3, 36, 36, device="cuda")
    ac.eval()
    ref.eval()
    with torch.no_grad():
        want = ref.forward({"obs": obs}, None)["action_logits"]
    got = ac.forward(obs)["action_logits"]
    np.testing.assert_allclose(got.cpu().numpy(), want.detach().cpu().numpy(), atol=5e-5, rtol=1e-4)
    fresh = ActorCritic(cfg, spaces.Dict({"obs": spaces.Box(0, 1, (3, 36, 36), np.float32)}), ac.action_space, "cuda")
    fresh.load_state_dict(loaded, strict=True)
    assert torch.equal(fresh.flat_params, ac.flat_params)


def _dp_run(num_agents, iters):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.train import make_runner
    _register()
    cfg = default_cfg(**dict(_F32, normalize_input=False, rollout=8, batch_size=num_agents * 8, num_batches_per_epoch=1,
                             num_epochs=1, num_workers=1, num_envs_per_worker=1, async_rl=False, seed=5, serial_mode=True,
                             synthetic_num_agents=num_agents, exploration_loss_coeff=0.01, learning_rate=1e-3))
    cfg, runner = make_runner(cfg)
    runner.init()
    for _ in range(iters):
        stats = runner.iteration()
    torch.cuda.synchronize()
    ac = runner.learner.actor_critic
    return dict(params=ac.flat_params.cpu().numpy(), env_steps=stats["learner_env_steps"], loss=stats["train"]["loss"])


def _dp_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", SF_DP_BACKEND="gloo")
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **_dp_run(16, 2))
    torch.distributed.destroy_process_group()


def test_f32_frames_two_replicas_stay_in_sync(tmp_path):
    """two data-parallel ranks of 16 envs each: identical parameters on both ranks and the step count of one 32-env run"""
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
    assert np.isfinite(r[0]["params"]).all() and np.isfinite(float(r[0]["loss"]))
