"""--augment_random_shift through the learner and the runner.

Learner twin: a flag-on learner trains once on a batch while every sf_random_shift_gather launch is recorded.  Each recorded
output must equal the NumPy model of the slab rows it names, bit for bit; forward and backward must have been handed the same
dense buffers with the dense addressing; the draw ids advance by one per SGD step from train_step; every dataset row is
gathered exactly once per key.  Then the TWIN batch is built — the slab with every dataset row replaced by its NumPy-shifted
frame, by the recorded minibatch membership — and a flag-OFF learner trains on it from the same weights.  If dense row i were
paired with anything but dataset row index[i] (actions, advantages, masks, recurrent chunk states, V-trace), the two runs
would train on different (frame, target) pairs.  The two are two correct evaluations of one step: parameters, exp_avg and
exp_avg_sq are compared with parity_util.compare_post_train at TIGHT of tests/test_gpu_nn.py, and bit for bit where the
dense and the indexed launches of the model resolve to the same kernels.  A twin shifted with draw_id + 1 must FAIL the same
comparison (the check can see a wrong shift).  Feed-forward (shuffle off / on), recurrent with recurrence 4, and a dict
observation (image + vector key, the multi-key composite).

Normaliser: the running moments after one train() equal a flag-off run's bit for bit.  Runner: PixelCatch, sync and async."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd.envs import frame_ops  # noqa: E402
from sample_factory_amd.envs import pixel_catch as pc  # noqa: E402
from tests.parity_util import compare_post_train  # noqa: E402

pytestmark = pytest.mark.gpu

E, T, A, PAD = 16, 8, 5, 4
IMG = (4, 36, 36)


def _spaces(dict_obs):
    from sample_factory_amd.envs import spaces
    keys = {"obs": spaces.Box(0, 255, IMG, np.uint8)}
    if dict_obs:
        keys["measurements"] = spaces.Box(-1.0, 1.0, (7,), np.float32)
    return spaces.Dict(keys)


def _learner(tmp_path, name, obs_space, **over):
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    base = dict(use_rnn=False, recurrence=1, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_simple", encoder_conv_mlp_layers=[64], rollout=T, batch_size=E * T // 2,
                num_batches_per_epoch=2, num_epochs=1, seed=3, serial_mode=True, train_dir=str(tmp_path), experiment=name,
                record_grad_norm=True)
    base.update(over)
    cfg = default_cfg(**base)
    env_info = EnvInfo(obs_space, spaces.Discrete(A), E)
    pv = torch.zeros(1, dtype=torch.int32)
    learner = Learner(cfg, env_info, pv, 0, ParameterServer(0, pv))
    learner.init()
    return learner, env_info


def _batch(env_info, rnn_size, seed=11):
    """a plausible trajectory batch: random frames, actions drawn from the recorded logits, a few episode ends"""
    from sample_factory_amd.algo.utils.shared_buffers import alloc_trajectory_tensors
    g = torch.Generator().manual_seed(seed)
    b = alloc_trajectory_tensors(env_info, E, T, rnn_size, "cuda")
    b["obs"]["obs"].copy_(torch.randint(0, 256, (E, T + 1) + IMG, generator=g, dtype=torch.int32).to(torch.uint8))
    if "measurements" in b["obs"]:
        b["obs"]["measurements"].copy_(torch.rand((E, T + 1, 7), generator=g) * 2 - 1)
    logits = torch.randn((E, T, A), generator=g)
    actions = torch.distributions.Categorical(logits=logits).sample()
    b["action_logits"].copy_(logits)
    b["actions"].copy_(actions.view(E, T, -1).float())
    b["log_prob_actions"].copy_(torch.log_softmax(logits, -1).gather(-1, actions[..., None])[..., 0])
    b["values"].copy_(torch.randn((E, T + 1), generator=g) * 0.5)
    b["rewards"].copy_(torch.randn((E, T), generator=g))
    b["dones"].copy_(torch.rand((E, T), generator=g) < 0.1)
    b["time_outs"].zero_()
    b["policy_id"].zero_()
    b["policy_version"].zero_()
    b["valids"].fill_(True)
    b["rnn_states"].copy_(torch.randn((E, T + 1, rnn_size), generator=g) * 0.3)
    return b


def _clone(batch):
    out = type(batch)()
    for k, v in batch.items():
        out[k] = _clone(v) if isinstance(v, dict) else v.clone()
    return out


def _spy_gathers(monkeypatch, log):
    from sample_factory_amd import lib
    real = lib.random_shift_gather

    def spy(dst, src, n, shape, **kw):
        real(dst, src, n, shape, **kw)
        idx, off = kw.get("index"), int(kw.get("offset", 0))
        rows = idx[:n].cpu().numpy().astype(np.int64) if idx is not None else np.arange(off, off + n, dtype=np.int64)
        log.append(dict(draw_id=int(kw["draw_id"]), rows=rows, out=dst[:n].clone(), shape=tuple(shape), pad=int(kw["pad"]),
                        seed=int(kw["seed"]), recurrence=int(kw["recurrence"]), traj_T=int(kw["traj_T"]), src_ptr=src.data_ptr(),
                        dst_ptr=dst.data_ptr(), n=int(n)))
    monkeypatch.setattr(lib, "random_shift_gather", spy)


def _spy_model(ac, log):
    """record what forward_heads (tag "train") and backward were handed"""
    fwd, bwd = ac.forward_heads, ac.backward

    def ptrs(obs):
        return {k: v.data_ptr() for k, v in obs.items()} if isinstance(obs, dict) else {"obs": obs.data_ptr()}

    def forward_heads(obs, n, **kw):
        if kw.get("tag") == "train":
            log.append(("fwd", ptrs(obs), n, kw.get("index"), kw.get("offset", 0), kw.get("traj_T", 0), kw.get("sample_stride")))
        return fwd(obs, n, **kw)

    def backward(acts, g_heads, obs, n, **kw):
        log.append(("bwd", ptrs(obs), n, kw.get("index"), kw.get("offset", 0), kw.get("traj_T", 0), kw.get("sample_stride")))
        return bwd(acts, g_heads, obs, n, **kw)
    ac.forward_heads, ac.backward = forward_heads, backward


def _golden_of(learner, before):
    """the flag-off twin's result in the layout compare_post_train reads"""
    ac = learner.actor_critic
    after, m, v = ac.state_dict(), ac.flat_to_ref(learner.exp_avg), ac.flat_to_ref(learner.exp_avg_sq)
    names = [n for n, _ in ac.ref_param_shapes()]
    g = dict(subsample=1, param_names=names, grad_norms=np.array(learner._grad_norms))
    for n in names:
        g["m_" + n], g["v_" + n] = m[n].reshape(-1).double().numpy(), v[n].reshape(-1).double().numpy()
        g["delta_" + n] = (after[n].double() - before[n].double()).reshape(-1).numpy()
    return g


def _twin_batch(batch0, gathers, seed, draw_shift=0):
    """batch0 with every dataset row of the image key replaced by its NumPy-shifted frame, by recorded membership"""
    twin = _clone(batch0)
    slab = batch0["obs"]["obs"].cpu().numpy()
    flat = slab.reshape((E * (T + 1),) + IMG)
    out = flat.copy()
    for rec in gathers:
        if rec["pad"] == 0:
            continue
        d = rec["rows"]
        rows = d + d // T
        dy, dx = frame_ops.random_shift_draws(seed, rec["draw_id"] + draw_shift, d // rec["recurrence"], rec["pad"])
        out[rows] = frame_ops.random_shift_frames(flat[rows], dy, dx, rec["pad"])
    twin["obs"]["obs"].copy_(torch.from_numpy(out.reshape(slab.shape)))
    return twin


def _twin_case(tmp_path, monkeypatch, dict_obs=False, **over):
    from tests.test_gpu_nn import TIGHT
    from sample_factory_amd import lib
    from sample_factory_amd.model.actor_critic import get_rnn_size
    obs_space = _spaces(dict_obs)
    on, env_info = _learner(tmp_path, "on", obs_space, augment_random_shift=PAD, **over)
    ac = on.actor_critic
    assert type(ac).__name__ == ("MultiKeyActorCritic" if dict_obs else "ActorCritic") and on._shift_pad == PAD
    assert on._shift_seed == frame_ops.random_shift_seed(on.cfg.seed, 0, 0)
    rnn_size = get_rnn_size(on.cfg) if on.cfg.use_rnn else 1
    batch0 = _batch(env_info, rnn_size)
    w0 = ac.flat_params.clone()
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    step0 = on.train_step = 41          # a resumed run: the draws continue from the checkpoint's train_step
    gathers, calls = [], []
    _spy_gathers(monkeypatch, gathers)
    _spy_model(ac, calls)
    assert on.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    monkeypatch.undo()
    keys = ["measurements", "obs"] if dict_obs else ["obs"]
    steps, R = on.cfg.num_batches_per_epoch, on.cfg.recurrence
    assert on.train_step == step0 + steps and len(gathers) == steps * len(keys)
    # ---- every launch against the NumPy model of the slab rows it names
    for i, rec in enumerate(gathers):
        key = keys[i % len(keys)]
        leaf = batch0["obs"][key].cpu().numpy()
        flat = leaf.reshape((E * (T + 1),) + leaf.shape[2:])
        d = rec["rows"]
        assert rec["draw_id"] == step0 + i // len(keys) and rec["seed"] == on._shift_seed and rec["traj_T"] == T
        assert rec["recurrence"] == R and rec["n"] == on.cfg.batch_size
        got = rec["out"].cpu().numpy()
        if key == "obs":
            assert rec["pad"] == PAD and rec["shape"] == IMG
            dy, dx = frame_ops.random_shift_draws(rec["seed"], rec["draw_id"], d // R, PAD)
            want = frame_ops.random_shift_frames(flat[d + d // T], dy, dx, PAD)
            assert (dy != PAD).any() or (dx != PAD).any()
            if R > 1:  # one draw per chunk: the rows of a chunk are consecutive and share it
                assert (d.reshape(-1, R) == d[::R, None] + np.arange(R)).all() and (dy.reshape(-1, R) == dy[::R, None]).all()
        else:
            assert rec["pad"] == 0 and rec["shape"] == (1, 1, 7)
            want = flat[d + d // T]
        assert got.tobytes() == want.tobytes(), (i, key)
    for k in range(len(keys)):  # every dataset row exactly once per key
        seen = np.concatenate([rec["rows"] for rec in gathers[k::len(keys)]])
        assert np.array_equal(np.sort(seen), np.arange(E * T))
    # ---- forward and backward got the same dense buffers, with the dense addressing
    fwds, bwds = [c for c in calls if c[0] == "fwd"], [c for c in calls if c[0] == "bwd"]
    assert len(fwds) == len(bwds) == steps
    for s, (f, b) in enumerate(zip(fwds, bwds)):
        assert f[1:] == b[1:] and f[3] is None and f[4] == 0 and f[5] == 0 and f[2] == on.cfg.batch_size
        for k_i, key in enumerate(keys):
            assert f[1][key] == gathers[s * len(keys) + k_i]["dst_ptr"]
    # ---- the twins: flag off, same weights, pre-shifted slab
    def run_twin(name, draw_shift):
        off, _ = _learner(tmp_path, name, obs_space, **over)
        assert off._shift_pad == 0
        off.actor_critic.flat_params.copy_(w0)
        off.actor_critic.params_changed()
        off.train_step = step0
        seen = []
        _spy_gathers(monkeypatch, seen)
        mbs = []
        real = off._get_minibatches
        off._get_minibatches = lambda *a: mbs.append(real(*a)) or mbs[-1]
        assert off.train(_twin_batch(batch0, gathers, on._shift_seed, draw_shift)) is not None
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert not seen                                   # flag off: the gather is never launched
        member = [idx.cpu().numpy() if idx is not None else np.arange(o, o + n) for idx, o, n in mbs[0]]
        for s, rows in enumerate(member):                 # the twin trained on the same minibatches
            assert np.array_equal(rows, gathers[s * len(keys)]["rows"])
        return off
    good = run_twin("off", 0)
    g = _golden_of(good, before)
    compare_post_train(on, g, before, "augment_twin", **TIGHT)
    if not dict_obs and not on.cfg.use_rnn:
        L0, n = ac.layers[0], on.cfg.batch_size
        same_kernels = not (L0.wt is not None and lib.conv_fwd_t_supported(n, L0.desc)) and lib.conv_fwd_workspace(n, L0.desc) == 0
        equal = torch.equal(ac.flat_params, good.actor_critic.flat_params) and torch.equal(on.exp_avg, good.exp_avg) and \
            torch.equal(on.exp_avg_sq, good.exp_avg_sq)
        print(f"dense and indexed conv1 launches resolve to the same kernels: {same_kernels}; twins bit-equal: {equal}")
        assert equal or not same_kernels
    # ---- negative control: a twin shifted by the NEXT step's draws is a different training step
    wrong = run_twin("wrong", 1)
    with pytest.raises(AssertionError):
        compare_post_train(on, _golden_of(wrong, before), before, "augment_twin_wrong", **TIGHT)


@pytest.mark.parametrize("shuffle", [False, True], ids=["in_order", "shuffled"])
def test_learner_twin_feed_forward(tmp_path, monkeypatch, shuffle):
    _twin_case(tmp_path, monkeypatch, shuffle_minibatches=shuffle)


def test_learner_twin_recurrent_chunks(tmp_path, monkeypatch):
    _twin_case(tmp_path, monkeypatch, use_rnn=True, rnn_type="gru", rnn_size=32, recurrence=4, shuffle_minibatches=True)


def test_learner_twin_dict_observation(tmp_path, monkeypatch):
    _twin_case(tmp_path, monkeypatch, dict_obs=True, encoder_mlp_layers=[16, 16], shuffle_minibatches=True)


def test_normaliser_moments_come_from_the_envs_frames(tmp_path):
    obs_space = _spaces(False)
    states = []
    for name, pad in (("on", PAD), ("off", 0)):
        learner, env_info = _learner(tmp_path, "norm_" + name, obs_space, normalize_input=True, augment_random_shift=pad)
        assert learner.train(_batch(env_info, 1)) is not None
        torch.cuda.synchronize()
        states.append({k: v.cpu() for k, v in learner.actor_critic.normalizer_state().items()})
    assert states[0].keys() == states[1].keys() and len(states[0]) >= 3
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k


# ------------------------------------------------------------------------------------------------ the runner
def _runner_cfg(tmp_path, name, **kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    register_env("pixel_catch", pc.make_pixel_catch_env)
    agents = 64
    base = dict(env="pixel_catch", use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_simple", encoder_conv_mlp_layers=[64], rollout=8, batch_size=agents * 8,
                num_batches_per_epoch=1, num_epochs=1, num_workers=1, num_envs_per_worker=1, worker_num_splits=1,
                async_rl=False, serial_mode=True, seed=5, env_gpu_observations=False, env_gpu_actions=False,
                env_workers_mode="inline", pixel_catch_agents=agents, pixel_catch_size=36, pixel_catch_frames=4,
                pixel_catch_balls=4, train_dir=str(tmp_path), experiment=name)
    base.update(kw)
    return default_cfg(**base)


def _count_gathers(monkeypatch):
    from sample_factory_amd import lib
    real, count = lib.random_shift_gather, [0]

    def counted(*a, **kw):
        count[0] += 1
        return real(*a, **kw)
    monkeypatch.setattr(lib, "random_shift_gather", counted)
    return count


@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
def test_runner_trains_pixel_catch_under_the_flag(tmp_path, monkeypatch, async_rl):
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    from sample_factory_amd.train import make_runner
    extra = dict(async_rl=True, serial_mode=False) if async_rl else {}
    count = _count_gathers(monkeypatch)
    cfg, runner = make_runner(_runner_cfg(tmp_path, "aug", augment_random_shift=PAD, **extra))
    assert runner.init() == 0
    try:
        p0 = runner.learner.actor_critic.flat_params.clone()
        for _ in range(3):
            runner.iteration()
        torch.cuda.synchronize()
        learner = runner.learner
        stats = dict(learner.last_summary)
        assert stats and all(np.isfinite(float(v)) for v in stats.values()), stats
        assert torch.isfinite(learner.actor_critic.flat_params).all() and not torch.equal(p0, learner.actor_critic.flat_params)
        assert learner.reuse_stats["reused"] == 0 and "augment_random_shift" in learner.reuse_stats["last_reason"]
        assert getattr(learner.actor_critic, "_keep", None) is None
        assert count[0] == learner.train_step >= 1        # one gather per SGD step, none from rollouts or bootstrap values
        assert json.load(open(tmp_path / "aug" / "config.json"))["augment_random_shift"] == PAD
        learner.save()
    finally:
        runner.close_envs()
    del runner
    # ---- enjoy reads the flag back from config.json and never gathers
    count[0] = 0
    argv = ["--env=pixel_catch", f"--train_dir={tmp_path}", "--experiment=aug", "--max_num_episodes=8", "--pixel_catch_agents=8"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    pc.add_pixel_catch_args(parser)
    status, avg = enjoy(parse_full_cfg(parser, argv))
    assert status == 0 and np.isfinite(avg) and count[0] == 0


def test_runner_with_the_flag_off_never_gathers(tmp_path, monkeypatch):
    from sample_factory_amd.train import make_runner
    count = _count_gathers(monkeypatch)
    cfg, runner = make_runner(_runner_cfg(tmp_path, "plain"))
    assert runner.init() == 0
    try:
        for _ in range(2):
            runner.iteration()
        torch.cuda.synchronize()
        assert count[0] == 0 and runner.learner.train_step >= 1 and runner.learner._shift_pad == 0
        assert json.load(open(tmp_path / "plain" / "config.json"))["augment_random_shift"] == 0
    finally:
        runner.close_envs()
