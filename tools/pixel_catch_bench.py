"""PixelCatch measured: the step-and-render launch alone, the game behind the headline configuration, and its learning curves.

 * kernel:   sf_pixcatch_step at 4096 x 4 x 84 x 84 into rotating columns of a slab that does not fit the caches, HIP-event
             timed over windows of back-to-back launches, ALTERNATING with sf_synth_obs + sf_synth_step on the same columns
             (the launches that store the same bytes for the headline env); median and spread per window, TB/s on the
             115.6 MB written, share of the 8.0 TB/s HBM3E peak.
 * legs:     bench.py's c2 configuration (4096 agents, Nature CNN, rollout 32, 4 minibatches, sync) on `synthetic_atari` (S)
             and on the device game (P): same sizes, the legs alternating, each in a child process of its own.
 * learning: the run of tests/test_gpu_pixel_catch_e2e.py (36 x 36 x 4, 1024 agents, convnet_simple, rollout 8) for three
             seeds: (caught, landed) per iteration, and the smallest iteration count at which every seed's last 10
             iterations beat its first 10 and the random player by five binomial standard errors.

  python tools/pixel_catch_bench.py [--legs kernel,S,P] [--rounds 2] [--steps 30] [--warmup 3] [--out profiles/pixel_catch_bench.json]
  python tools/pixel_catch_bench.py --learning [--iters 400] [--seeds 1,2,3] [--learning_out profiles/pixel_catch_learning.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, K, H, W = 4096, 32, 4, 84, 84
FRAME_BYTES = K * H * W
HBM_PEAK_TBS = 8.0


def kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import lib
    Tk = 8  # columns: 4096 x 9 x 28 224 B = 1.04 GB
    slab = torch.zeros((B, Tk + 1, K, H, W), dtype=torch.uint8, device="cuda")
    state = torch.zeros((B, lib.pixcatch_state_words(K)), dtype=torch.int32, device="cuda")
    act = torch.randint(0, 3, (B,), dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float32, device="cuda")
    term = torch.zeros(B, dtype=torch.bool, device="cuda")
    lib.pixcatch_reset(state, slab[:, 0], 0, 0, 4)
    step = [0]

    def game(t):
        lib.pixcatch_step(state, act, slab[:, t + 1], rew, term, 0, 0, 4)

    def synth(t):
        lib.synth_step(act, 0, 6, 0, step[0], rew, term)
        step[0] += 1
        lib.synth_obs(slab[:, t + 1].data_ptr(), slab.stride(0), B, 0, FRAME_BYTES, 0, step[0])
    fns = dict(pixcatch_step=game, synth_obs_plus_synth_step=synth)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            for t in range(Tk):
                fn(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (args.reps * Tk)
    for fn in fns.values():
        window(fn)
    res = {name: [] for name in fns}
    for _ in range(args.windows):  # alternate: both see the same machine
        for name, fn in fns.items():
            res[name].append(window(fn))
    moved = B * FRAME_BYTES
    out = dict(leg="kernel", envs=B, frame=[K, H, W], bytes_written_per_step=moved, launches_per_window=args.reps * Tk,
               windows=args.windows, hbm_peak_tb_per_s=HBM_PEAK_TBS)
    for name, ms in res.items():
        med = sorted(ms)[len(ms) // 2]
        out[name] = dict(us_per_step_median=round(med * 1e3, 2), us_per_step_min=round(min(ms) * 1e3, 2),
                         us_per_step_max=round(max(ms) * 1e3, 2), tb_per_s_median=round(moved / (med * 1e-3) / 1e12, 3),
                         share_of_hbm_peak=round(moved / (med * 1e-3) / 1e12 / HBM_PEAK_TBS, 3))
    s = out["synth_obs_plus_synth_step"]
    out["expectation_us"] = round(s["us_per_step_median"] + s["us_per_step_max"] - s["us_per_step_min"], 2)
    out["pixcatch_within_expectation"] = out["pixcatch_step"]["us_per_step_median"] <= out["expectation_us"]
    print(json.dumps(out), flush=True)


def leg(args, which):
    sys.path.insert(0, ROOT)
    import tempfile

    import torch
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.pixel_catch import make_pixel_catch_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_atari", make_synthetic_env)
    register_env("pixel_catch", make_pixel_catch_env)
    cfg = default_cfg(
        env="synthetic_atari" if which == "S" else "pixel_catch", use_rnn=False, recurrence=1,
        encoder_conv_architecture="convnet_atari", nonlinearity="relu", encoder_conv_mlp_layers=[512], obs_scale=255.0,
        normalize_input=False, normalize_returns=True, gamma=0.99, gae_lambda=0.95, ppo_clip_ratio=0.1, ppo_clip_value=1.0,
        value_loss_coeff=0.5, exploration_loss_coeff=0.01, max_grad_norm=4.0, learning_rate=1e-4, adam_eps=1e-6,
        train_dir=tempfile.mkdtemp(prefix="sf_pixel_catch_bench_"), rollout=T, batch_size=B * T // 4, num_batches_per_epoch=4,
        num_epochs=1, async_rl=False, serial_mode=True, batched_sampling=True, num_workers=1, num_envs_per_worker=1,
        worker_num_splits=1, env_gpu_observations=True, env_gpu_actions=True, actor_worker_gpus=[0], seed=0,
        synthetic_num_agents=B, pixel_catch_agents=B, pixel_catch_size=H, pixel_catch_frames=K, pixel_catch_balls=4)
    cfg, runner = make_runner(cfg)
    assert runner.init() == 0
    for _ in range(args.warmup):
        runner.iteration()
    steps0 = runner.learner.env_steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        runner.iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(leg=which, env=cfg.env, env_steps_per_s=round((runner.learner.env_steps - steps0) / dt, 1),
                          wall_s=round(dt, 3), iterations=args.steps)), flush=True)


def learning_child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile

    import torch
    import test_gpu_pixel_catch_e2e as e2e
    t0 = time.perf_counter()
    extra = dict(learning_rate=args.lr) if args.lr is not None else {}
    curve, runner = e2e.learning_run(int(args.child_seed), args.iters, train_dir=tempfile.mkdtemp(prefix="sf_pixel_catch_learn_"),
                                     **extra)
    torch.cuda.synchronize()
    print(json.dumps(dict(seed=int(args.child_seed), wall_s=round(time.perf_counter() - t0, 2), curve=curve,
                          settings=dict(e2e.LEARN, **extra, size=e2e.SIZE, frames=e2e.K, rollout=e2e.T, balls=e2e.BALLS))), flush=True)


def learning(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import test_gpu_pixel_catch_e2e as e2e
    rnd = e2e.random_player_rate()
    runs = []
    for seed in args.seeds.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "learning", "--child_seed", seed, f"--iters={args.iters}"] + \
            ([f"--lr={args.lr}"] if args.lr is not None else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        runs.append(json.loads(line[-1]) if line and r.returncode == 0 else dict(seed=seed, rc=r.returncode, err=r.stderr[-800:]))
        print(json.dumps({k: v for k, v in runs[-1].items() if k != "curve"}), flush=True)
        if r.returncode != 0:
            break

    def passes(curve, n):
        first, last = e2e.rate(curve[:10]), e2e.rate(curve[n - 10:n])
        balls = sum(b for _, b in curve[n - 10:n])
        return last > first and last >= rnd + 5.0 * float(np.sqrt(rnd * (1 - rnd) / max(1, balls)))
    curves = [r["curve"] for r in runs if "curve" in r]
    smallest = next((n for n in range(20, args.iters + 1, 10) if curves and all(passes(c, n) for c in curves)), None)
    summary = dict(random_player_rate=round(rnd, 4), iterations_run=args.iters, smallest_count_all_seeds_pass=smallest,
                   catch_rate_by_50_iterations={str(r["seed"]): [round(e2e.rate(r["curve"][i:i + 50]), 4)
                                                                 for i in range(0, len(r["curve"]), 50)]
                                                for r in runs if "curve" in r},
                   wall_s={str(r["seed"]): r.get("wall_s") for r in runs})
    print(json.dumps(summary), flush=True)
    from sample_factory_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(args.learning_out)), exist_ok=True)
    with open(args.learning_out, "w") as f:
        json.dump(dict(source_sha16=build.source_sha16(), summary=summary, runs=runs), f)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--child_seed", default="1")
    p.add_argument("--legs", default="kernel,S,P")
    p.add_argument("--rounds", type=int, default=2, help="how often the S, P pair is repeated (alternating)")
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--timeout", type=int, default=300)
    p.add_argument("--learning", action="store_true")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--seeds", default="1,2,3")
    p.add_argument("--lr", type=float, default=None, help="learning rate of the learning runs (default: the test's)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_catch_bench.json"))
    p.add_argument("--learning_out", default=os.path.join(ROOT, "profiles", "pixel_catch_learning.json"))
    args = p.parse_args()
    if args.child:
        {"kernel": kernel, "learning": learning_child}.get(args.child, lambda a: leg(a, args.child))(args)
        return
    if args.learning:
        return learning(args)
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    legs = args.legs.split(",")
    order = [w for w in legs if w == "kernel"] + [w for _ in range(args.rounds) for w in legs if w != "kernel"]
    results = []
    for which in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [
            f"--{k}={getattr(args, k)}" for k in ("steps", "warmup", "reps", "windows")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        results.append(json.loads(line[-1]) if line and r.returncode == 0 else dict(leg=which, rc=r.returncode, err=r.stderr[-800:]))
        print(json.dumps(results[-1]), flush=True)
        if r.returncode != 0:
            break
    summary = {w: [r["env_steps_per_s"] for r in results if r.get("leg") == w and "env_steps_per_s" in r] for w in ("S", "P")}
    if summary["S"] and summary["P"]:
        summary["P_over_S_mean_rate"] = round(sum(summary["P"]) / len(summary["P"]) / (sum(summary["S"]) / len(summary["S"])), 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(source_sha16=build.source_sha16(), workload=f"{B} agents, {K} x {H} x {W} u8 frames, Nature CNN, rollout "
                       f"{T}, 4 minibatches, sync", order=order, steps=args.steps, warmup=args.warmup, summary=summary,
                       results=results), f, indent=1)


if __name__ == "__main__":
    main()
