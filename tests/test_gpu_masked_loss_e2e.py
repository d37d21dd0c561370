"""cfg.mask_actions_in_loss through the whole engine: MaskedBanditEnv / MaskedTupleBanditEnv -> masked
sampler -> slab -> Learner._prepare_batch keeps the slab's mask view -> sf_vtrace_masked / sf_ppo_loss_masked.  With the
flag on the learner's first evaluation of a rollout, on unchanged weights, finds the distribution the sampler drew from
(ratios 1, KL 0, up to the f32 log-prob's rounding); with it off the ratios start away from 1, as the issue describes.
Set up as tests/test_gpu_masked_tuple_e2e.py and tests/test_gpu_nn.py::test_action_mask_end_to_end."""
import numpy as np
import pytest
import torch

from test_gpu_action_heads import logp_tol

pytestmark = pytest.mark.gpu

ENVS = {"bandit6": ("masked_bandit", None, 25, 3e-3, [32]), "4x3": ("masked_tuple_bandit", (4, 3), 30, 3e-3, [64]),
        "150x5": ("masked_tuple_bandit", (150, 5), 40, 1e-2, [64])}


def _runner(name, **over):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_masked_bandit_env, make_masked_tuple_bandit_env
    from sample_factory_amd.train import make_runner
    register_env("masked_bandit", make_masked_bandit_env)
    register_env("masked_tuple_bandit", make_masked_tuple_bandit_env)
    env, heads, iters, lr, mlp = ENVS[name]
    kw = dict(env=env, use_rnn=False, nonlinearity="tanh", normalize_input=False, encoder_mlp_layers=mlp, rollout=8,
              batch_size=256, num_batches_per_epoch=2, num_epochs=2, num_workers=1, num_envs_per_worker=1, async_rl=False,
              seed=4, serial_mode=True, synthetic_num_agents=64, learning_rate=lr, gamma=0.0, normalize_returns=False,
              mask_actions_in_loss=True)
    if heads is not None:
        kw["synthetic_head_sizes"] = heads
    kw.update(over)
    cfg, runner = make_runner(default_cfg(**kw))
    runner.init()
    return runner, iters


def _first_look(runner, ds, flag):
    """_calculate_losses on the whole prepared dataset of the rollout in runner.traj, before any update"""
    ln = runner.learner
    ln._loss_mask_on = flag
    buff, N, num_invalids = ln._prepare_batch(runner.traj[ds])
    assert ("action_mask" in buff) == flag
    dist, _, _, kl_old, _, _, summ = ln._calculate_losses(buff, num_invalids)
    torch.cuda.synchronize()
    return buff, dist, kl_old, summ


@pytest.mark.parametrize("name", list(ENVS), ids=list(ENVS))
def test_first_evaluation_of_a_rollout_finds_the_sampled_distribution(name):
    """after the first rollout, on unchanged weights.  Flag on: kl_old_mean and max |ratio - 1| within the sampler <->
    loss bound, 2 * logp_tol(logp, A) per row (exp(bound) - 1 for the ratio; the bound's mean for the KL mean); the returned
    distribution carries the mask rows and the float64 mean of its kl_divergence agrees with the kernel's scalar within
    check_loss's scalar bound (1e-6 + 2e-5 relative).  Flag off, same rollout: max |ratio - 1| is beyond the bound."""
    from sample_factory_amd.algo.utils.action_distributions import get_action_distribution
    runner, _ = _runner(name)
    ln = runner.learner
    assert ln._loss_mask_on is True
    p0 = ln.actor_critic.flat_params.clone()
    runner._rollout_all(float(ln.train_step))
    ds = runner._ready[0]
    A = ln.num_action_params
    lp = runner.traj["log_prob_actions"].double().cpu().numpy().reshape(-1)
    bound = 2 * logp_tol(lp, A)
    buff, dist, kl_old, summ = _first_look(runner, ds, True)
    assert torch.equal(p0, ln.actor_critic.flat_params)
    assert buff.action_mask.data_ptr() == runner.traj["obs"]["action_mask"].data_ptr() and buff.action_mask.shape[1] == 9
    ratio = summ.ratio.double().cpu().numpy()
    kl_mean = float(summ.kl_old_mean)
    print(f"{name} flag on: max |ratio - 1| {np.abs(ratio - 1).max():.3e} (bound {np.expm1(bound).min():.3e}..), "
          f"kl_old_mean {kl_mean:.3e}")
    assert np.all(np.abs(ratio - 1.0) <= np.expm1(bound)), (np.abs(ratio - 1).max(), bound.min())
    assert abs(kl_mean) <= bound.mean(), (kl_mean, bound.mean())
    members = getattr(dist, "distributions", [dist])
    mask_rows = runner.traj["obs"]["action_mask"][:, :8].reshape(512, A)
    assert all(d.action_mask is not None for d in members)
    assert torch.equal(torch.cat([d.action_mask for d in members], -1).to(torch.uint8), mask_rows)
    space = ln.env_info.action_space
    d64 = get_action_distribution(space, dist.raw_logits.double(), mask_rows.double())
    o64 = get_action_distribution(space, buff.action_logits.double(), mask_rows.double())
    kl64 = float(d64.kl_divergence(o64)[buff.valids].mean())
    assert abs(kl64 - kl_mean) <= 1e-6 + 2e-5 * abs(kl64), (kl64, kl_mean)
    assert kl_old.shape == (int(buff.valids.sum()),)
    # flag off, the same rollout: the learner re-evaluates the unmasked distribution
    buff, dist, kl_old, summ = _first_look(runner, ds, False)
    off = np.abs(summ.ratio.double().cpu().numpy() - 1.0)
    print(f"{name} flag off: max |ratio - 1| {off.max():.3e}, mean {off.mean():.3e}")
    assert off.max() > 100 * np.expm1(bound).max() and (off > np.expm1(bound)).mean() > 0.5
    assert all(getattr(d, "action_mask", None) is None for d in getattr(dist, "distributions", [dist]))


@pytest.mark.parametrize("name,vtrace", [("bandit6", False), ("4x3", False), ("150x5", False), ("4x3", True)],
                         ids=["bandit6", "4x3", "150x5", "4x3-vtrace"])
def test_training_under_the_mask_learns_the_bandit(name, vtrace):
    """a short run with the flag on reaches the reward bound the existing masked end-to-end tests assert for the env
    (MaskedBanditEnv: the last iteration's mean reward above the first's + 0.25 and above 0.7; the Tuple bandits: the mean
    of the last ten iterations above that of the first ten), every action of the last rollout is allowed, and the loss
    launches were the masked ones.  Once more with V-trace (recurrence = rollout, gamma 0.9: one-step episodes)"""
    from sample_factory_amd import lib
    over = dict(with_vtrace=True, recurrence=8, gamma=0.9) if vtrace else {}
    runner, iters = _runner(name, **over)
    ln = runner.learner
    calls = []
    real_loss, real_vt = lib.ppo_loss, lib.vtrace

    def spy(real, tag):
        def f(*a, **k):
            calls.append((tag, k.get("mask") is not None, k.get("mask_T")))
            return real(*a, **k)
        return f
    lib.ppo_loss, lib.vtrace = spy(real_loss, "loss"), spy(real_vt, "vtrace")
    try:
        rewards = []
        for _ in range(iters):
            stats = runner.iteration()
            rewards.append(float(runner.traj["rewards"].mean()))
    finally:
        lib.ppo_loss, lib.vtrace = real_loss, real_vt
    assert np.isfinite(stats["train"]["loss"]) and torch.isfinite(ln.actor_critic.flat_params).all()
    assert runner.samplers[0].env.last_allowed.all()
    assert calls and all(m and t == 8 for _, m, t in calls), calls[:4]
    assert vtrace == any(tag == "vtrace" for tag, _, _ in calls)
    print(f"{name} vtrace={vtrace}: reward first {rewards[0]:.3f} last {rewards[-1]:.3f}, first ten "
          f"{np.mean(rewards[:10]):.3f} last ten {np.mean(rewards[-10:]):.3f}")
    if name == "bandit6":
        assert rewards[-1] > rewards[0] + 0.25 and rewards[-1] > 0.7, (rewards[0], rewards[-1])
    else:
        assert np.mean(rewards[-10:]) > np.mean(rewards[:10]), (rewards[:10], rewards[-10:])
