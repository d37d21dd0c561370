"""Tuple action spaces under obs["action_mask"] through the whole engine: MaskedTupleBanditEnv -> policy forward ->
sf_sample_write_step_tuple_masked (the lane-per-row kernel for Tuple(Discrete(4), Discrete(3)), the wave-per-row kernel
for Tuple(Discrete(150), Discrete(5))) -> slab -> Learner.train, with the policy half of a step recorded and replayed as
a launch program.  The pattern of tests/test_gpu_nn.py::test_action_mask_end_to_end."""
import numpy as np
import pytest
import torch

from test_gpu_action_heads import logp_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


@pytest.mark.parametrize("head_sizes,iters,lr", [((4, 3), 30, 3e-3), ((150, 5), 40, 1e-2)], ids=["4x3", "150x5"])
def test_masked_tuple_bandit_end_to_end(lib, head_sizes, iters, lr):
    """the slab holds one mask column per distribution parameter; over every recorded step (step 0 of a rollout
    included) no member's action is masked out (the env's own per-member record agrees); the recorded log-prob is
    the float64 sum of the members' masked log-softmax of the recorded RAW logits at the recorded actions, within logp_tol; the learner trains on it (it
    re-evaluates the unmasked distribution, as the reference does) and the mean reward of the last ten iterations is
    above that of the first ten; the policy half of a step is a launch program whose one sampler call is
    sf_sample_write_step_tuple_masked, safe to replay, and is replayed (the checks above run on replayed steps too)"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import MaskedTupleBanditEnv, make_masked_tuple_bandit_env
    from sample_factory_amd.train import make_runner
    register_env("masked_tuple_bandit", make_masked_tuple_bandit_env)
    n, T, A = 64, 8, sum(head_sizes)
    cfg = default_cfg(env="masked_tuple_bandit", use_rnn=False, nonlinearity="tanh", normalize_input=False,
                      encoder_mlp_layers=[64], rollout=T, batch_size=256, num_batches_per_epoch=2, num_epochs=2,
                      num_workers=1, num_envs_per_worker=1, async_rl=False, seed=4, serial_mode=True,
                      synthetic_num_agents=n, synthetic_head_sizes=head_sizes, learning_rate=lr, gamma=0.0,
                      normalize_returns=False)
    cfg, runner = make_runner(cfg)
    runner.init()
    ac = runner.learner.actor_critic
    sampler = runner.samplers[0]
    assert isinstance(sampler.env, MaskedTupleBanditEnv) and sampler.masked and sampler.heads == list(head_sizes)
    assert ac.num_action_params == A and runner.traj["obs"]["action_mask"].shape == (n, T + 1, A)
    assert runner.traj["actions"].shape == (n, T, len(head_sizes))
    offs = torch.tensor([sum(head_sizes[:i]) for i in range(len(head_sizes))], device="cuda")
    p0 = ac.flat_params.clone()
    rewards = []
    if not sampler._started:
        sampler.reset()  # (the first rollout would do it: slab column 0 then holds the mask of its step 0 before it runs)
    for it in range(iters):
        # step 0 of a rollout is sampled under the mask the env returned with the LAST observation of the rollout before it
        # (slab column T, carried into column 0 when the next round starts); the first rollout's is the reset's, column 0.
        # Read before the iteration overwrites it.
        mask0 = (runner.traj["obs"]["action_mask"][:, T:] if it else runner.traj["obs"]["action_mask"][:, :1]).clone()
        runner.iteration()
        tr = runner.traj
        a = tr["actions"].long()
        mk = torch.cat([mask0, tr["obs"]["action_mask"][:, 1:-1]], 1)    # the masks of steps 0 .. T - 1
        assert ((a >= 0) & (a < torch.tensor(head_sizes, device="cuda"))).all()
        assert mk.gather(-1, a + offs).all(), f"iteration {it}: a masked-out action was recorded"
        assert sampler.env.last_allowed.all()
        lg = tr["action_logits"].double() + (mk == 0) * -1e9
        want = sum(torch.log_softmax(lg[..., o:o + h], -1).gather(-1, a[..., i:i + 1]).squeeze(-1)
                   for i, (o, h) in enumerate(zip(offs.tolist(), head_sizes))).cpu().numpy()
        got = tr["log_prob_actions"].cpu().numpy()
        np.testing.assert_array_less(np.abs(got - want), logp_tol(want, A), err_msg=f"iteration {it}")
        rewards.append(float(tr["rewards"].mean()))
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(p0, ac.flat_params)
    first, last = float(np.mean(rewards[:10])), float(np.mean(rewards[-10:]))
    print(f"masked tuple bandit {head_sizes}: mean reward of the first 10 iterations {first:.4f}, of the last 10 {last:.4f}")
    assert last > first, (first, last)
    pol = [p for k, p in sampler._progs.items() if k[0] == "policy" and isinstance(p, lib.LaunchProgram)]
    assert len(pol) >= T and sampler.program_replays >= T, (len(pol), sampler.program_replays)
    for p in pol:
        names = [c[2] for c in p.calls]
        assert [x for x in names if x.startswith("sf_sample_write_step")] == ["sf_sample_write_step_tuple_masked"], names
        assert names[-1] == "sf_sample_write_step_tuple_masked" and p.unsafe is None
