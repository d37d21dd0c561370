"""--augment_consistency_coeff (DrAC) through the learner and the runner, on the twin set-up and the sizes
of tests/test_gpu_augment_shift_e2e.py.

One `_losses_native` (feed-forward with shuffle off / on, GRU with recurrence 4, a dict observation on the multi-key
composite): the dense buffers hold the slab rows the index names in rows [0, n) and frame_ops.random_shift_frames of them
in rows [n, 2n); g_heads[:n] is bit for bit what lib.ppo_loss writes for heads[:n]; g_heads[n:] meets the float64
yardstick (tests/consistency_refs.py) on the heads read back.  One `train`: forward and backward were handed the same
2n-row buffers, the draw ids advance by one per SGD step.

Pairing: on a slab of flat frames (one grey level per sample) a shift is the identity, so every student row equals its
target: consistency sums exactly 0, and the trained parameters and Adam moments lie within TIGHT (tests/test_gpu_nn.py) of
a flag-off learner's.  With the shifted half rotated by one row (a test-only permutation) the KL is not zero.

Linearity: the flat gradient of a DrAC step is the flag-off gradient on the minibatch plus the gradient of a backward
pass over the n shifted rows alone, fed with the yardstick's consistency gradients.

alpha = 0 launches no consistency loss; the runner on PixelCatch, sync and async; enjoy; the refusals at Learner.init."""
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
from tests import consistency_refs as R  # noqa: E402
from tests.parity_util import compare_post_train  # noqa: E402
from tests.test_gpu_augment_shift_e2e import (A, E, IMG, PAD, T, _batch, _clone, _golden_of, _learner, _runner_cfg,  # noqa: E402
                                               _spaces, _spy_gathers, _spy_model)

pytestmark = pytest.mark.gpu

ALPHA = 0.1
MODELS = {"in_order": dict(shuffle_minibatches=False),
          "shuffled": dict(shuffle_minibatches=True),
          "gru": dict(use_rnn=True, rnn_type="gru", rnn_size=32, recurrence=4, shuffle_minibatches=True),
          "dict_obs": dict(encoder_mlp_layers=[16, 16], shuffle_minibatches=True)}


def _drac(tmp_path, name, model, **kw):
    return _learner(tmp_path, name, _spaces(model == "dict_obs"), augment_random_shift=PAD, augment_consistency_coeff=ALPHA,
                    **MODELS[model], **kw)


def _rnn_size(cfg):
    from sample_factory_amd.model.actor_critic import get_rnn_size
    return get_rnn_size(cfg) if cfg.use_rnn else 1


def _count(monkeypatch, name):
    from sample_factory_amd import lib
    real, count = getattr(lib, name), [0]

    def counted(*a, **kw):
        count[0] += 1
        return real(*a, **kw)
    monkeypatch.setattr(lib, name, counted)
    return count


def _check_gathers(gathers, batch0, keys, n, R_, seed, step0):
    """two launches per key and SGD step: the plain gather into rows [0, n), the shifted one into rows [n, 2n)"""
    per_step = 2 * len(keys)
    for i, rec in enumerate(gathers):
        key, shifted = keys[(i % per_step) // 2], i % 2 == 1
        leaf = batch0["obs"][key].cpu().numpy()
        flat = leaf.reshape((E * (T + 1),) + leaf.shape[2:])
        d = rec["rows"]
        assert rec["draw_id"] == step0 + i // per_step and rec["seed"] == seed and rec["traj_T"] == T
        assert rec["recurrence"] == R_ and rec["n"] == n
        want = flat[d + d // T]
        if key == "obs":
            assert rec["shape"] == IMG and rec["pad"] == (PAD if shifted else 0)
            if shifted:
                dy, dx = frame_ops.random_shift_draws(seed, rec["draw_id"], d // R_, PAD)
                assert (dy != PAD).any() or (dx != PAD).any()
                want = frame_ops.random_shift_frames(want, dy, dx, PAD)
        else:
            assert rec["pad"] == 0 and rec["shape"] == (1, 1, 7)
        assert rec["out"].cpu().numpy().tobytes() == want.tobytes(), (i, key, shifted)
        if shifted:  # row n + i is the twin of row i: the second half starts n rows behind the first, same dataset rows
            first = gathers[i - 1]
            assert np.array_equal(first["rows"], d) and rec["src_ptr"] == first["src_ptr"]
            assert rec["dst_ptr"] == first["dst_ptr"] + n * want[0].size * want.dtype.itemsize


@pytest.mark.parametrize("model", list(MODELS))
def test_one_losses_native_and_one_train(tmp_path, monkeypatch, model):
    from sample_factory_amd import lib
    on, env_info = _drac(tmp_path, "on", model)
    ac, cfg = on.actor_critic, on.cfg
    assert on._cons_coeff == ALPHA and on._shift_pad == PAD
    keys = ["measurements", "obs"] if model == "dict_obs" else ["obs"]
    n, R_, ld = cfg.batch_size, cfg.recurrence, ac.heads_ld
    batch0 = _batch(env_info, _rnn_size(cfg))
    step0 = on.train_step = 41
    # ---- one _losses_native on the SECOND minibatch
    buff, N, num_invalids = on._prepare_batch(_clone(batch0))
    mb = on._get_minibatches(n, N)[1]
    gathers = []
    _spy_gathers(monkeypatch, gathers)
    acts, g_heads, sc = on._losses_native(buff, mb, num_invalids)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(gathers) == 2 * len(keys) and on._mb_rows == 2 * n
    _check_gathers(gathers, batch0, keys, n, R_, on._shift_seed, step0)
    heads = acts[-1]
    assert heads.shape == (2 * n, ld) and g_heads.shape == (2 * n, ld)
    index, offset, _ = mb
    rows = index.long() if index is not None else torch.arange(offset, offset + n, device="cuda")
    assert np.array_equal(rows.cpu().numpy(), gathers[0]["rows"])
    # g_heads[:n]: bit for bit the PPO loss the test runs itself on heads[:n]
    mine = torch.zeros((n, ld), device="cuda")
    sums, ratio = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(n, device="cuda")
    lib.ppo_loss(heads[:n, 1:], ld, heads[:n, 0], ld, buff.actions, buff.log_prob_actions, buff.action_logits, buff["values"],
                 buff.advantages, buff.returns, buff.valids, index, offset, n, A, on.loss_cfg, on._moments, sums,
                 mine[:, 1:], mine[:, 0], ratio_out=ratio, head_sizes=on._head_sizes)
    torch.cuda.synchronize()
    assert torch.equal(mine, g_heads[:n]) and torch.equal(sums, on._sums) and torch.equal(ratio, on._ratio)
    assert g_heads[:n, :1 + A].abs().max() > 0
    # g_heads[n:]: the yardstick on the heads read back
    valid = buff.valids[rows].cpu()
    ref = R.consistency_reference(heads[:n].cpu(), heads[n:].cpu(), valid, [A], ALPHA, ALPHA, n_valid=float(on._moments[2]))
    got, want = g_heads[n:, :1 + A].double().cpu().numpy(), ref["g"].numpy()
    np.testing.assert_allclose(got[:, 1:], want[:, 1:], rtol=5e-4, atol=1e-5 * np.abs(want[:, 1:]).max())
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=5e-4, atol=1e-5 * np.abs(want[:, 0]).max())
    assert (g_heads[:, 1 + A:] == 0).all() and ref["kl_sum"] > 0
    cs = on._cons_sums.cpu().numpy()
    assert abs(cs[0] - ref["kl_sum"]) <= 1e-6 + 2e-5 * ref["kl_sum"] and abs(cs[1] - ref["dv2_sum"]) <= 1e-6 + 2e-5 * ref["dv2_sum"]
    assert cs[3] == ref["n_valid"] and abs(cs[2] - ref["kl_max"]) <= 1e-4 * max(1.0, ref["kl_max"])
    nv = ref["n_valid"]
    for slot, want_s in ((11, ref["kl_sum"] / nv), (12, ref["kl_max"]), (13, ref["dv2_sum"] / nv)):
        assert abs(float(sc[slot]) - want_s) <= 1e-4 * max(1.0, abs(want_s)), (slot, float(sc[slot]), want_s)
    # _calculate_losses keeps its signature and reports the first n rows
    dist, pl, el, kl_old, kll, vl, summ = on._calculate_losses((buff, mb), num_invalids)
    assert kl_old.shape[0] == int(valid.sum()) and summ["values"].shape == (n,) and summ.ratio.shape == (n,)
    assert all(torch.isfinite(x).all() for x in (pl, el, kll, vl, kl_old))
    # ---- one train(): forward and backward see the same 2n-row buffers; the draw ids advance by one per SGD step
    gathers, calls = [], []
    _spy_gathers(monkeypatch, gathers)
    _spy_model(ac, calls)
    cons = _count(monkeypatch, "consistency_loss")
    assert on.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    monkeypatch.undo()
    steps = cfg.num_batches_per_epoch
    assert on.train_step == step0 + steps and len(gathers) == steps * 2 * len(keys) and cons[0] == steps
    _check_gathers(gathers, batch0, keys, n, R_, on._shift_seed, step0)
    for k in range(len(keys)):  # every dataset row exactly once per key and half
        for half in (0, 1):
            seen = np.concatenate([rec["rows"] for rec in gathers[2 * k + half::2 * len(keys)]])
            assert np.array_equal(np.sort(seen), np.arange(E * T))
    fwds, bwds = [c for c in calls if c[0] == "fwd"], [c for c in calls if c[0] == "bwd"]
    assert len(fwds) == len(bwds) == steps
    for s, (f, b) in enumerate(zip(fwds, bwds)):
        assert f[1:] == b[1:] and f[3] is None and f[4] == 0 and f[5] == 0 and f[2] == 2 * n
        for k_i, key in enumerate(keys):
            assert f[1][key] == gathers[(s * len(keys) + k_i) * 2]["dst_ptr"]
    stats = dict(on.last_summary)
    for k in ("consistency_kl", "consistency_kl_max", "consistency_value"):
        assert np.isfinite(stats[k]) and stats[k] > 0, (k, stats)
    assert stats["consistency_kl_max"] >= stats["consistency_kl"]


# ------------------------------------------------------------------------------------------------ pairing
def _flat_batch(env_info, rnn_size):
    """every frame flat, one distinct grey level per sample of the slab: any shift is the identity"""
    b = _batch(env_info, rnn_size)
    levels = (torch.randperm(E * (T + 1), generator=torch.Generator().manual_seed(2)) + 17).to(torch.uint8)
    assert E * (T + 1) + 17 <= 256 and len(set(levels.tolist())) == E * (T + 1)
    b["obs"]["obs"].copy_(levels.view(E, T + 1, 1, 1, 1).expand((E, T + 1) + IMG).cuda())
    return b


def _spy_consistency(monkeypatch, log):
    from sample_factory_amd import lib
    real = lib.consistency_loss

    def spy(*a, **kw):
        real(*a, **kw)
        log.append(a[15].clone())  # sums: {sum KL, sum dv^2, max KL, n_valid}
    monkeypatch.setattr(lib, "consistency_loss", spy)


@pytest.mark.parametrize("model", ["shuffled", "gru"])
def test_pairing_on_flat_frames(tmp_path, monkeypatch, model):
    from sample_factory_amd import lib
    from tests.test_gpu_nn import TIGHT
    on, env_info = _drac(tmp_path, "on", model)
    ac = on.actor_critic
    batch0 = _flat_batch(env_info, _rnn_size(on.cfg))
    w0 = ac.flat_params.clone()
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    sums = []
    _spy_consistency(monkeypatch, sums)
    assert on.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(sums) == on.cfg.num_batches_per_epoch
    for s in sums:  # every student row equals its target: exactly nothing, whatever the draws were
        s = s.cpu().numpy()
        print("consistency sums on flat frames:", s)
        assert s[0] == 0.0 and s[1] == 0.0 and s[2] == 0.0 and s[3] == on.cfg.batch_size
    assert on.last_summary["consistency_kl"] == 0.0 and on.last_summary["consistency_value"] == 0.0
    # ... so the step is the flag-off step
    off, _ = _learner(tmp_path, "off", _spaces(False), **MODELS[model])
    assert off._shift_pad == 0 and off._cons_coeff == 0.0
    off.actor_critic.flat_params.copy_(w0)
    off.actor_critic.params_changed()
    none = _count(monkeypatch, "consistency_loss")
    assert off.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert none[0] == 0
    compare_post_train(on, _golden_of(off, before), before, f"drac_pairing_{model}", **TIGHT)
    # ---- the halves paired off by one: the shifted half rotated by a row is another sample's frame
    wrong, _ = _drac(tmp_path, "wrong", model)
    wrong.actor_critic.flat_params.copy_(w0)
    wrong.actor_critic.params_changed()
    real = lib.random_shift_gather

    def rotated(dst, src, n, shape, **kw):
        real(dst, src, n, shape, **kw)
        if kw["pad"] > 0:
            dst[:n].copy_(dst[:n].roll(1, 0))
    monkeypatch.setattr(lib, "random_shift_gather", rotated)
    sums = []
    _spy_consistency(monkeypatch, sums)
    assert wrong.train(_clone(batch0)) is not None
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert all(float(s[0]) > 0.0 and float(s[1]) > 0.0 for s in sums), [s.tolist() for s in sums]
    assert wrong.last_summary["consistency_kl"] > 0.0


# ------------------------------------------------------------------------------------------------ linearity
def test_gradient_is_the_ppo_gradient_plus_the_consistency_gradient(tmp_path):
    """rtol: TIGHT's d_rtol.  atol per parameter tensor: TIGHT's floor (1e-4) of the tensor's largest reference gradient —
    an element whose gradient is ~0 is a sum over 2n rows of terms of the tensor's scale, and its f32 rounding error is
    relative to that scale, not to the element (parity_util.py uses 25 x this floor for weight deltas)"""
    from tests.test_gpu_nn import TIGHT
    model = "shuffled"
    on, env_info = _drac(tmp_path, "on", model)
    off, _ = _learner(tmp_path, "off", _spaces(False), **MODELS[model])
    off.actor_critic.flat_params.copy_(on.actor_critic.flat_params)
    off.actor_critic.params_changed()
    batch0 = _batch(env_info, 1)
    on.train_step = off.train_step = 7
    n = on.cfg.batch_size
    np.random.seed(123)
    buff, N, inv = on._prepare_batch(_clone(batch0))
    mb = on._get_minibatches(n, N)[1]
    acts, g_heads, _ = on._losses_native(buff, mb, inv)
    ac = on.actor_critic
    ac.backward(acts, g_heads, on._mb_frames[0], on._mb_rows, sample_stride=ac.obs_elems, **on._mb_frames[1])
    g_drac = ac.flat_to_ref(ac.flat_grads.clone())
    # (1) the flag-off learner's gradient on the same minibatch
    buff_o, _, inv_o = off._prepare_batch(_clone(batch0))
    oc = off.actor_critic
    acts_o, g_o, _ = off._losses_native(buff_o, mb, inv_o)
    assert off._mb_rows == n and g_o.shape[0] == n
    heads_t = acts_o[-1][:n].cpu()
    oc.backward(acts_o, g_o, off._mb_frames[0], n, sample_stride=oc.obs_elems, **off._mb_frames[1])
    g_ppo = oc.flat_to_ref(oc.flat_grads.clone())
    # (2) backward over the n shifted rows alone, fed with the yardstick's consistency gradients
    index, offset, _ = mb
    d = index.cpu().numpy().astype(np.int64)
    flat = batch0["obs"]["obs"].cpu().numpy().reshape((E * (T + 1),) + IMG)
    dy, dx = frame_ops.random_shift_draws(on._shift_seed, 7, d // on.cfg.recurrence, PAD)
    shifted = torch.from_numpy(frame_ops.random_shift_frames(flat[d + d // T], dy, dx, PAD)).cuda().view(n, -1)
    dense = dict(sample_stride=oc.obs_elems, index=None, offset=0, traj_T=0)
    acts_s = oc.forward_heads(shifted, n, tag="train", **dense)
    valid = buff_o.valids[index.long()].cpu()
    ref = R.consistency_reference(heads_t, acts_s[-1][:n].cpu(), valid, [A], ALPHA, ALPHA, n_valid=float(off._moments[2]))
    g_c = torch.zeros((n, oc.heads_ld), device="cuda")
    g_c[:, :1 + A] = ref["g"].float().cuda()
    oc.backward(acts_s, g_c, shifted, n, **dense)
    g_cons = oc.flat_to_ref(oc.flat_grads.clone())
    torch.cuda.synchronize()
    for name in g_drac:
        want = (g_ppo[name].double() + g_cons[name].double()).cpu().numpy()
        got = g_drac[name].double().cpu().numpy()
        assert np.abs(g_cons[name].cpu().numpy()).max() > 0, name
        np.testing.assert_allclose(got, want, rtol=TIGHT["d_rtol"], atol=TIGHT["floor"] * np.abs(want).max(), err_msg=name)


# ------------------------------------------------------------------------------------------------ alpha = 0
@pytest.mark.parametrize("pad", [PAD, 0], ids=["rad", "off"])
def test_alpha_zero_launches_no_consistency_loss(tmp_path, monkeypatch, pad):
    learner, env_info = _learner(tmp_path, "a0", _spaces(False), augment_random_shift=pad, shuffle_minibatches=True)
    cons, gath = _count(monkeypatch, "consistency_loss"), _count(monkeypatch, "random_shift_gather")
    assert learner.train(_batch(env_info, 1)) is not None
    torch.cuda.synchronize()
    steps, n = learner.cfg.num_batches_per_epoch, learner.cfg.batch_size
    assert cons[0] == 0 and gath[0] == (steps if pad else 0) and learner._mb_rows == n
    assert not hasattr(learner, "_cons_sums") and "consistency_kl" not in learner.last_summary
    bufs = learner.actor_critic._bufs
    if pad:
        assert bufs[("aug", "obs")].shape[0] == n               # the dense buffer keeps its size
    else:
        assert ("aug", "obs") not in bufs
    assert bufs[("g", "heads")].shape[0] == n and ("rnn", "keep_tm2") not in bufs


# ------------------------------------------------------------------------------------------------ the runner
@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
def test_runner_trains_pixel_catch_with_the_consistency_loss(tmp_path, monkeypatch, async_rl):
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    from sample_factory_amd.train import make_runner
    extra = dict(async_rl=True, serial_mode=False) if async_rl else {}
    gath, cons = _count(monkeypatch, "random_shift_gather"), _count(monkeypatch, "consistency_loss")
    cfg, runner = make_runner(_runner_cfg(tmp_path, "drac", augment_random_shift=PAD, augment_consistency_coeff=ALPHA, **extra))
    assert runner.init() == 0
    try:
        p0 = runner.learner.actor_critic.flat_params.clone()
        for _ in range(4):
            runner.iteration()
        torch.cuda.synchronize()
        learner = runner.learner
        stats = dict(learner.last_summary)
        assert stats and all(np.isfinite(float(v)) for v in stats.values()), stats
        for k in ("consistency_kl", "consistency_kl_max", "consistency_value"):
            assert k in stats and stats[k] >= 0.0, (k, stats)
        assert torch.isfinite(learner.actor_critic.flat_params).all() and not torch.equal(p0, learner.actor_critic.flat_params)
        assert learner.reuse_stats["reused"] == 0
        assert cons[0] == learner.train_step >= 1 and gath[0] == 2 * learner.train_step
        saved = json.load(open(tmp_path / "drac" / "config.json"))
        assert saved["augment_consistency_coeff"] == ALPHA and saved["augment_random_shift"] == PAD
        learner.save()
    finally:
        runner.close_envs()
    del runner
    # ---- enjoy reads the flag back from config.json and launches neither
    gath[0] = cons[0] = 0
    argv = ["--env=pixel_catch", f"--train_dir={tmp_path}", "--experiment=drac", "--max_num_episodes=8", "--pixel_catch_agents=8"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    pc.add_pixel_catch_args(parser)
    status, avg = enjoy(parse_full_cfg(parser, argv))
    assert status == 0 and np.isfinite(avg) and gath[0] == 0 and cons[0] == 0


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw,exc,names", [
    (dict(augment_random_shift=PAD, augment_consistency_coeff=-0.5), ValueError, ["augment_consistency_coeff"]),
    (dict(augment_random_shift=PAD, augment_consistency_coeff=float("nan")), ValueError, ["augment_consistency_coeff"]),
    (dict(augment_random_shift=PAD, augment_consistency_coeff=float("inf")), ValueError, ["augment_consistency_coeff"]),
    (dict(augment_consistency_coeff=ALPHA), ValueError, ["augment_consistency_coeff", "augment_random_shift"]),
    (dict(augment_random_shift=PAD, augment_consistency_coeff=ALPHA, mask_actions_in_loss=True), NotImplementedError,
     ["augment_consistency_coeff", "mask_actions_in_loss"])], ids=["negative", "nan", "inf", "no_shift", "masked_loss"])
def test_learner_init_refuses(tmp_path, monkeypatch, kw, exc, names):
    cons = _count(monkeypatch, "consistency_loss")
    with pytest.raises(exc) as e:
        _learner(tmp_path, "bad", _spaces(False), **kw)
    assert all(nm in str(e.value) for nm in names) and cons[0] == 0
