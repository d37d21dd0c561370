"""PixelCatch through the whole engine at 36 x 36 x 4 with convnet_simple and a rollout of 8.

  * replay: the slab's recorded actions, replayed through the NumPy model from the same seed, reproduce obs[:, 1:], rewards
    and dones of every rollout exactly (sync and async; the device env renders into the slab: zero_copy);
  * twins: the device env, the host env with frames=4 and the host env with frames=1 under --device_framestack=4 yield
    identical slabs and identical parameters after four iterations (the method of tests/test_gpu_hwc_frames_e2e.py);
  * learning: the conv rollout-and-train loop improves the catch rate from frames it rendered itself;
  * the run's checkpoint loads in enjoy.

Learning, as measured when this test was written (tools/pixel_catch_bench.py --learning, profiles/pixel_catch_learning.json;
the random player catches 0.175): catch rate over iterations 0-50 / 100-150 / 200-250 / 350-400 of seed 1: 0.15 / 0.24 /
0.90 / 0.99, seed 2: 0.16 / 0.17 / 0.36 / 0.58, seed 3: 0.14 / 0.25 / 0.67 / 0.99; 150 iterations (LEARN_ITERS, 0.6 s) is
the smallest count, in steps of 10, at which all three seeds meet both conditions of the learning test."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd.envs import pixel_catch as pc  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE, K, T, BALLS = 36, 4, 8, 4
FIELDS = ("actions", "action_logits", "log_prob_actions", "rewards", "dones", "time_outs")
# the smallest count of iterations at which seeds 1, 2 and 3 all met both learning conditions on the MI355X
LEARN_ITERS = 150


def _cfg(env="pixel_catch", agents=64, frames=K, **kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    register_env("pixel_catch", pc.make_pixel_catch_env)
    register_env("pixel_catch_host", pc.make_pixel_catch_host_env)
    base = dict(env=env, use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_simple", encoder_conv_mlp_layers=[64], rollout=T, batch_size=agents * T,
                num_batches_per_epoch=1, num_epochs=1, num_workers=1, num_envs_per_worker=1, worker_num_splits=1,
                async_rl=False, serial_mode=True, seed=5, env_gpu_observations=False, env_gpu_actions=False,
                env_workers_mode="inline", pixel_catch_agents=agents, pixel_catch_size=SIZE, pixel_catch_frames=frames,
                pixel_catch_balls=BALLS)
    base.update(kw)
    return default_cfg(**base)


def _snapshot(rows):
    snap = {f: rows[f].cpu().numpy().copy() for f in FIELDS}
    snap["values"] = rows["values"][:, :T].cpu().numpy().copy()
    snap["obs"] = rows["obs"]["obs"].cpu().numpy().copy()
    return snap


def run(iters, **kw):
    """(one snapshot of the slab rows per trained-on rollout, parameters at the start and at the end, runner)"""
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_cfg(**kw))
    assert runner.init() == 0
    try:
        p0 = runner.learner.actor_critic.flat_params.clone()
        snaps = []
        for _ in range(iters):
            runner.iteration()
            torch.cuda.synchronize()
            snaps.append(_snapshot(runner._prev_rows[0]))
        return snaps, p0, runner.learner.actor_critic.flat_params.clone(), runner
    finally:
        runner.close_envs()


# ------------------------------------------------------------------------------------------------ replay
@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
def test_recorded_actions_replayed_through_the_model_reproduce_the_slab(async_rl):
    N = 128
    extra = dict(async_rl=True, serial_mode=False, learning_rate=0.0) if async_rl else {}
    snaps, p0, p1, runner = run(4, agents=N, **extra)
    assert runner.sampler.zero_copy and not runner.sampler.host_env
    assert runner.env_info.obs_space["obs"].shape == (K, SIZE, SIZE)
    state = pc.model_reset(N, 0, 5, SIZE, SIZE, K, BALLS)
    assert np.array_equal(snaps[0]["obs"][:, 0], pc.render(state, SIZE, SIZE, K))
    landed = 0
    for r, s in enumerate(snaps):
        assert s["obs"].shape == (N, T + 1, K, SIZE, SIZE)
        assert np.array_equal(s["obs"][:, 0], pc.render(state, SIZE, SIZE, K)), f"rollout {r}: carried-over first column"
        for t in range(T):
            a = s["actions"][:, t].reshape(N, -1)[:, 0].astype(np.int64)
            assert ((a >= 0) & (a < 3)).all()
            state, rew, term = pc.model_step(state, a, 0, 5, SIZE, SIZE, K, BALLS)
            assert np.array_equal(s["obs"][:, t + 1], pc.render(state, SIZE, SIZE, K)), (r, t)
            assert s["rewards"][:, t].tobytes() == rew.tobytes(), (r, t)
            assert np.array_equal(s["dones"][:, t].astype(bool), term) and not s["time_outs"][:, t].any(), (r, t)
            landed += int((rew != 0).sum())
    assert landed > 0
    assert async_rl or not torch.equal(p0, p1)


def test_the_gymnasium_route_plays_the_same_game():
    env = pc.PixelCatchVecEnv(num_agents=7, size=(SIZE, SIZE), frames=K, balls_per_episode=2, seed=3, env0=11)
    host = pc.PixelCatchHostEnv(num_agents=7, size=(SIZE, SIZE), frames=K, balls_per_episode=2, seed=3, env0=11)
    assert env.observation_space["obs"].shape == host.observation_space["obs"].shape == (K, SIZE, SIZE)
    o, _ = env.reset()
    ho, _ = host.reset()
    assert o["obs"].is_cuda and np.array_equal(o["obs"].cpu().numpy(), ho["obs"])
    rng = np.random.default_rng(0)
    for _ in range(80):
        a = rng.integers(0, 3, 7)
        o, rew, term, trunc, _ = env.step(a)
        ho, hrew, hterm, htrunc, _ = host.step(a)
        assert np.array_equal(o["obs"].cpu().numpy(), ho["obs"]) and np.array_equal(rew.cpu().numpy(), hrew)
        assert np.array_equal(term.cpu().numpy(), hterm) and not trunc.any()
    assert np.array_equal(env.state.cpu().numpy(), host.state)


# ------------------------------------------------------------------------------------------------ twins
def test_device_env_and_host_twins_yield_identical_slabs_and_parameters(tmp_path):
    N = 64
    a, pa0, pa, ra = run(4, agents=N, train_dir=str(tmp_path / "device"))
    b, pb0, pb, rb = run(4, agents=N, env="pixel_catch_host", train_dir=str(tmp_path / "host4"))
    c, pc0, pc_, rc = run(4, agents=N, env="pixel_catch_host", frames=1, device_framestack=K, train_dir=str(tmp_path / "host1"))
    assert ra.sampler.zero_copy and rb.sampler.host_env and rc.sampler.host_env
    assert {k: r.key.frame_shape[0] for k, r in rc.sampler.routes.items() if r.key.k > 1} == {"obs": 1}
    assert rc.env.observation_space["obs"].shape == (1, SIZE, SIZE)
    assert ra.env_info.obs_space["obs"].shape == rb.env_info.obs_space["obs"].shape == rc.env_info.obs_space["obs"].shape
    for r in range(4):
        for other, what in ((b, "host env, frames=4"), (c, "host env, frames=1 under device_framestack=4")):
            for f in a[r]:
                x, y = a[r][f], other[r][f]
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"rollout {r}, {what}: {f}"
    assert torch.equal(pa0, pb0) and torch.equal(pa0, pc0)
    assert torch.equal(pa, pb) and torch.equal(pa, pc_) and not torch.equal(pa, pa0)


# ------------------------------------------------------------------------------------------------ learning
def random_player_rate(balls=20000, N=256, seed=123):
    """catch rate of uniform random actions on the NumPy model (36 x 36), over at least `balls` balls"""
    rng = np.random.default_rng(seed)
    st = pc.model_reset(N, 0, seed, SIZE, SIZE, 1, BALLS)
    caught = landed = 0
    while landed < balls:
        st, rew, _ = pc.model_step(st, rng.integers(0, 3, N), 0, seed, SIZE, SIZE, 1, BALLS)
        caught += int((rew > 0).sum())
        landed += int((rew != 0).sum())
    return caught / landed


LEARN = dict(agents=1024, batch_size=2048, num_batches_per_epoch=4, num_epochs=1, learning_rate=5e-4)


def learning_run(seed, iters, **kw):
    """per iteration (balls caught, balls landed) in the rollout it trained on; the runner"""
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_cfg(seed=seed, **dict(LEARN, **kw)))
    assert runner.init() == 0
    curve = []
    for _ in range(iters):
        runner.iteration()
        rew = runner._prev_rows[0]["rewards"]
        curve.append((int((rew > 0).sum()), int((rew != 0).sum())))
    return curve, runner


def rate(curve):
    return sum(c for c, _ in curve) / max(1, sum(n for _, n in curve))


def test_the_conv_path_learns_to_catch_and_its_checkpoint_loads_in_enjoy(tmp_path):
    """The mean catch rate of the last 10 iterations is above that of the first 10 and above the random player's by at
    least five binomial standard errors of the balls it was measured over.  Nothing absolute is asserted."""
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    curve, runner = learning_run(1, LEARN_ITERS, train_dir=str(tmp_path), experiment="pixel_catch_learn")
    first, last, balls = rate(curve[:10]), rate(curve[-10:]), sum(n for _, n in curve[-10:])
    rnd = random_player_rate()
    se = float(np.sqrt(rnd * (1.0 - rnd) / balls))
    print(f"PixelCatch 36 x 36 x 4, 1024 agents, {LEARN_ITERS} iterations: catch rate of the first 10 iterations {first:.4f}, "
          f"of the last 10 {last:.4f} over {balls} balls; random player {rnd:.4f}, standard error {se:.4f}")
    assert last > first, (first, last)
    assert last >= rnd + 5.0 * se, (last, rnd, se)
    # ---- the checkpoint in enjoy: 50 agents x 4 balls = 200 balls per round of episodes
    runner.learner.save()
    del runner
    argv = ["--env=pixel_catch", f"--train_dir={tmp_path}", "--experiment=pixel_catch_learn", "--max_num_episodes=50",
            "--eval_deterministic=True", "--pixel_catch_agents=50"]
    parser, _ = parse_sf_args(argv, evaluation=True)
    pc.add_pixel_catch_args(parser)
    status, avg = enjoy(parse_full_cfg(parser, argv))
    assert status == 0 and -BALLS <= avg <= BALLS
    print(f"enjoy, deterministic policy: average episode return {avg:.3f} = catch rate {(avg / BALLS + 1) / 2:.4f} over at "
          f"least 200 balls")
