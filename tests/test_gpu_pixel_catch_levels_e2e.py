"""PixelCatch with levels through the whole engine: 64 agents, 36 x 36 x 4, 3 decoys, a set of 4 levels, one ball per episode.

  * replay: the slab's recorded actions, replayed through the NumPy model, reproduce obs[:, 1:], rewards and dones exactly
    (sync and async; the device env renders the decoys into the slab: zero_copy);
  * twins: the device env, the host env with frames=4 and the host env with frames=1 under --device_framestack=4 yield
    identical slabs and parameters;
  * a short run's checkpoint loads in enjoy, with the saved flags and on held-out levels given on the command line; the
    frames enjoy plays come from the requested range (current_levels()).
Nothing is asserted about the generalisation gap: that number is reported, not tested."""
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

N, SIZE, K, T, BALLS, ND, L, S, SEED = 64, 36, 4, 8, 1, 3, 4, 0, 5
FIELDS = ("actions", "action_logits", "log_prob_actions", "rewards", "dones", "time_outs")
LEVELS = dict(pixel_catch_decoys=ND, pixel_catch_levels=L, pixel_catch_start_level=S)


def _cfg(env="pixel_catch", frames=K, **kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    register_env("pixel_catch", pc.make_pixel_catch_env)
    register_env("pixel_catch_host", pc.make_pixel_catch_host_env)
    base = dict(env=env, use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_simple", encoder_conv_mlp_layers=[64], rollout=T, batch_size=N * T,
                num_batches_per_epoch=1, num_epochs=1, num_workers=1, num_envs_per_worker=1, worker_num_splits=1,
                async_rl=False, serial_mode=True, seed=SEED, env_gpu_observations=False, env_gpu_actions=False,
                env_workers_mode="inline", pixel_catch_agents=N, pixel_catch_size=SIZE, pixel_catch_frames=frames,
                pixel_catch_balls=BALLS, **LEVELS)
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


def _frame(state):
    return pc.render(state, SIZE, SIZE, K, 0, SEED, BALLS, ND, L, S)


@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
def test_recorded_actions_replayed_through_the_model_reproduce_the_slab(async_rl):
    extra = dict(async_rl=True, serial_mode=False, learning_rate=0.0) if async_rl else {}
    snaps, p0, p1, runner = run(6, **extra)
    assert runner.sampler.zero_copy and not runner.sampler.host_env
    assert (runner.env.decoys, runner.env.levels, runner.env.start_level) == (ND, L, S)
    state = pc.model_reset(N, 0, SEED, SIZE, SIZE, K, BALLS, ND, L, S)
    plain = pc.render(state, SIZE, SIZE, K)
    assert np.array_equal(snaps[0]["obs"][:, 0], _frame(state)) and not np.array_equal(snaps[0]["obs"][:, 0], plain)
    ended, levels = 0, set()
    for r, s in enumerate(snaps):
        assert s["obs"].shape == (N, T + 1, K, SIZE, SIZE)
        assert np.array_equal(s["obs"][:, 0], _frame(state)), f"rollout {r}: carried-over first column"
        for t in range(T):
            a = s["actions"][:, t].reshape(N, -1)[:, 0].astype(np.int64)
            state, rew, term = pc.model_step(state, a, 0, SEED, SIZE, SIZE, K, BALLS, ND, L, S)
            assert np.array_equal(s["obs"][:, t + 1], _frame(state)), (r, t)
            assert s["rewards"][:, t].tobytes() == rew.tobytes(), (r, t)
            assert np.array_equal(s["dones"][:, t].astype(bool), term) and not s["time_outs"][:, t].any(), (r, t)
            ended += int(term.sum())
            levels |= set(pc.episode_level(state, np.arange(N), SEED, BALLS, L, S).tolist())
    assert ended >= N and levels == set(range(S, S + L))  # (an episode is one ball: at most D = 34 of the 48 steps)
    assert async_rl or not torch.equal(p0, p1)


def test_device_env_and_host_twins_yield_identical_slabs_and_parameters(tmp_path):
    """With frames=1 the host env renders ONE plane per step and the device stacks them.  A plane rendered before an
    episode's end would keep the old level's decoys, but the stack of a finished episode is refilled with the new first
    frame (as the game's own planes are), and inside an episode the level does not change: the three runs agree."""
    a, pa0, pa, ra = run(4, train_dir=str(tmp_path / "device"))
    b, pb0, pb, rb = run(4, env="pixel_catch_host", train_dir=str(tmp_path / "host4"))
    c, pc0, pc_, rc = run(4, env="pixel_catch_host", frames=1, device_framestack=K, train_dir=str(tmp_path / "host1"))
    assert ra.sampler.zero_copy and rb.sampler.host_env and rc.sampler.host_env
    assert {k: r.key.frame_shape[0] for k, r in rc.sampler.routes.items() if r.key.k > 1} == {"obs": 1}
    assert rc.env.observation_space["obs"].shape == (1, SIZE, SIZE)
    assert (rb.env.decoys, rb.env.levels, rc.env.decoys, rc.env.levels) == (ND, L, ND, L)
    for r in range(4):
        for other, what in ((b, "host env, frames=4"), (c, "host env, frames=1 under device_framestack=4")):
            for f in a[r]:
                x, y = a[r][f], other[r][f]
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"rollout {r}, {what}: {f}"
    assert a[3]["dones"].any() or a[2]["dones"].any()
    assert torch.equal(pa0, pb0) and torch.equal(pa0, pc0)
    assert torch.equal(pa, pb) and torch.equal(pa, pc_) and not torch.equal(pa, pa0)


def test_the_checkpoint_loads_in_enjoy_on_its_own_levels_and_on_held_out_ones(tmp_path):
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    from sample_factory_amd.envs.env_utils import register_env
    import json
    snaps, p0, p1, runner = run(3, train_dir=str(tmp_path), experiment="pixel_catch_levels")
    runner.learner.save()
    saved = json.load(open(os.path.join(str(tmp_path), "pixel_catch_levels", "config.json")))
    assert {k: saved[k] for k in LEVELS} == LEVELS
    del runner
    made = []

    def factory(*args, **kw):
        made.append(pc.make_pixel_catch_env(*args, **kw))
        return made[-1]
    register_env("pixel_catch", factory)
    try:
        for flags, (lo, n) in (([], (S, L)),
                               (["--pixel_catch_start_level=1000000", "--pixel_catch_levels=100000"], (1000000, 100000))):
            argv = ["--env=pixel_catch", f"--train_dir={tmp_path}", "--experiment=pixel_catch_levels", "--max_num_episodes=128",
                    "--pixel_catch_agents=32"] + flags
            parser, _ = parse_sf_args(argv, evaluation=True)
            pc.add_pixel_catch_args(parser)
            status, avg = enjoy(parse_full_cfg(parser, argv))
            assert status == 0 and np.isfinite(avg) and -BALLS <= avg <= BALLS
            env = made[-1]
            assert (env.decoys, env.levels, env.start_level, env.num_agents) == (ND, n, lo, 32)
            lv = env.current_levels().astype(np.int64)
            assert ((lv >= lo) & (lv < lo + n)).all()
            # one more step of the env enjoy played: the frame shows the decoys of levels of that range
            assert int(env.state[:, 0].min()) > 1  # (it goes on from the episodes enjoy played)
            o = {"obs": torch.empty((32, K, SIZE, SIZE), dtype=torch.uint8, device="cuda")}
            env.step_into(torch.zeros(32, dtype=torch.int32, device="cuda"), o["obs"])
            st = env.state.cpu().numpy()
            lv = pc.episode_level(st, np.arange(32), SEED, BALLS, n, lo)
            assert ((lv.astype(np.int64) >= lo) & (lv.astype(np.int64) < lo + n)).all()
            frame = o["obs"].cpu().numpy()
            assert np.array_equal(frame, pc.render(st, SIZE, SIZE, K, 0, SEED, BALLS, ND, n, lo))
            dx, dy = pc.level_decoys(lv, ND, SIZE, SIZE)
            assert all(frame[e, K - 1, dy[e, d], dx[e, d]] == pc.BALL for e in range(32) for d in range(ND))
            print(f"enjoy on levels [{lo}, {lo + n}): average episode return {avg:.3f}")
        assert len(set(made[-1].current_levels().tolist())) > L  # held-out levels: more of them than the training set has
    finally:
        register_env("pixel_catch", pc.make_pixel_catch_env)
