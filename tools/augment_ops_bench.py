"""--augment_cutout / --augment_intensity / --augment_mix measured: what the two operations add to the shift's
gather launch, what they add to Learner.train, and what each augmentation does to the train / test gap on PixelCatch levels.
Every leg is a child process of its own on the same GPU; what is compared ALTERNATES.

 * kernel:   the protocol of tools/augment_shift_bench.py: 32768 samples of 4 x 84 x 84 u8 and of 3 x 72 x 128 u8 indexed out
             of a [4096, 33, ...] slab (3.8 GB: nothing stays in the caches); HIP events around windows of back-to-back
             launches after a warm-up window, all configurations alternating window by window.  sf_augment_gather with each op
             alone (pad 4 | cutout (8, 24) | intensity 64) and with all three; the yardsticks in the same run:
             sf_random_shift_gather at pad 4 and sf_copy_rows on the same bytes.  Medians, ranges, and every configuration as
             a ratio of the shift's median next to the shift's own window spread (max / min).
 * train:    bench.py's c2 workload; wall clock of the runner's train phase per iteration (4 SGD steps), shift + cutout +
             intensity against the shift alone, alternating.
 * learning: the protocol of profiles/pixel_catch_levels_learning.json unchanged (36 x 36 x 4, 1024 agents, convnet_simple,
             rollout 8, 400 iterations, seeds 1 - 3, 6 decoys, train levels [0, 8), held-out levels [1 000 000, 1 100 000),
             enjoy with sampled actions over at least 20 000 balls); arms, all with --augment_consistency_coeff=0.1: the shift
             (pad 4, the control), cutout (4, 12), intensity 64, and all three under --augment_mix=one.

  python tools/augment_ops_bench.py [--legs kernel,train,learning] [--commit TEXT] [--out profiles/augment_ops_bench.json]
                                    [--learning_out profiles/augment_ops_learning.json]"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_TBS = 8.0
E, T, N, PAD, CUT, AMP = 4096, 32, 32768, 4, (8, 24), 64
ALPHA = 0.1
ARMS = (("shift", dict(augment_random_shift=4)), ("cutout", dict(augment_cutout=[4, 12])), ("intensity", dict(augment_intensity=64)),
        ("mix_one", dict(augment_random_shift=4, augment_cutout=[4, 12], augment_intensity=64, augment_mix="one")))
TRAIN_ARMS = (("all_three", dict(augment_random_shift=PAD, augment_cutout=list(CUT), augment_intensity=AMP)),
              ("shift_only", dict(augment_random_shift=PAD)))
TEST_START, TEST_LEVELS, EVAL_BALLS = 1000000, 100000, 20000


def kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import lib
    out = dict(leg="kernel", samples=N, slab=[E, T + 1], pad=PAD, cutout=list(CUT), intensity=AMP, windows=args.windows,
               launches_per_window=args.reps, hbm_peak_tb_per_s=HBM_PEAK_TBS, device=torch.cuda.get_device_name(0), shapes={})
    for shape in ((4, 84, 84), (3, 72, 128)):
        C, H, W = shape
        S = C * H * W
        slab = torch.randint(0, 256, (E, T + 1, C, H, W), dtype=torch.uint8, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        index = torch.randperm(E * T, generator=g, device="cuda")[:N].to(torch.int32)
        dense, dense2 = (torch.empty((N, S), dtype=torch.uint8, device="cuda") for _ in range(2))
        step = [0]

        def shift():
            step[0] += 1
            lib.random_shift_gather(dense, slab, N, shape, index=index, traj_T=T, pad=PAD, seed=7, draw_id=step[0])

        def augment(**ops):
            def fn():
                step[0] += 1
                lib.augment_gather(dense, slab, N, shape, index=index, traj_T=T, seed=7, draw_id=step[0], **ops)
            return fn
        fns = dict(random_shift_gather=shift, copy_rows=lambda: lib.copy_rows(dense2, dense),
                   augment_shift_only=augment(pad=PAD), augment_cutout_only=augment(cutout=CUT),
                   augment_cutout_random_fill=augment(cutout=CUT, cutout_fill="random"),
                   augment_intensity_only=augment(intensity=AMP), augment_all_three=augment(pad=PAD, cutout=CUT, intensity=AMP))

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.reps
        for fn in fns.values():
            window(fn)  # warm-up
        res = {name: [] for name in fns}
        for _ in range(args.windows):  # alternate: all of them see the same machine
            for name, fn in fns.items():
                res[name].append(window(fn))
        moved = 2 * N * S
        sh = out["shapes"]["x".join(map(str, shape))] = dict(sample_bytes=S, bytes_read_plus_written_per_launch=moved)
        for name, ms in res.items():
            med = sorted(ms)[len(ms) // 2]
            sh[name] = dict(us_per_launch_median=round(med * 1e3, 2), us_per_launch_min=round(min(ms) * 1e3, 2),
                            us_per_launch_max=round(max(ms) * 1e3, 2), tb_per_s_median=round(moved / (med * 1e-3) / 1e12, 3),
                            share_of_hbm_peak=round(moved / (med * 1e-3) / 1e12 / HBM_PEAK_TBS, 3))
        yard = sh["random_shift_gather"]
        sh["random_shift_gather_window_spread_max_over_min"] = round(yard["us_per_launch_max"] / yard["us_per_launch_min"], 4)
        for name in fns:
            if name != "random_shift_gather":
                sh[name + "_over_random_shift_gather"] = round(sh[name]["us_per_launch_median"] / yard["us_per_launch_median"], 4)
        del slab, dense, dense2
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def train(args):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.train import make_runner
    bargs = argparse.Namespace(workload="c2", envs=E, rollout=T, num_batches=4, num_epochs=1, async_rl=False, env_instances=1,
                               normalize_input=False, rnn_type="lstm", host_env_sim_ms=0.0, env_workers=0)
    cfg, env_name, env_factory, _, _ = bench.workload_cfg(bargs, 0, 1)
    for k, v in dict(TRAIN_ARMS)[args.arm].items():
        setattr(cfg, k, v)
    register_env(env_name, env_factory)
    cfg, runner = make_runner(cfg)
    runner.init()
    for _ in range(args.warmup):
        runner.iteration()
    torch.cuda.synchronize()
    t_train0 = float(runner.timing.get("train", 0.0))
    step0, t0 = runner.learner.train_step, time.perf_counter()
    for _ in range(args.steps):
        runner.iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(leg="train", arm=args.arm, iterations=args.steps, sgd_steps=runner.learner.train_step - step0,
                          train_ms_per_iteration=round(1e3 * (float(runner.timing.get("train", 0.0)) - t_train0) / args.steps, 3),
                          wall_ms_per_iteration=round(1e3 * dt / args.steps, 3),
                          env_steps_per_s=round(args.steps * E * T / dt, 1), device=torch.cuda.get_device_name(0))), flush=True)


def learning(args):
    """one arm, one seed: train, save, and play the checkpoint on the train and on the held-out levels"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile

    import torch
    import test_gpu_pixel_catch_e2e as e2e
    from sample_factory_amd.cfg.arguments import parse_full_cfg, parse_sf_args
    from sample_factory_amd.enjoy import enjoy
    from sample_factory_amd.envs import pixel_catch as pc
    train_dir, t0 = tempfile.mkdtemp(prefix="sf_augment_ops_"), time.perf_counter()
    curve, runner = e2e.learning_run(int(args.child_seed), args.iters, train_dir=train_dir, experiment="ops",
                                     pixel_catch_decoys=args.decoys, pixel_catch_levels=args.levels, pixel_catch_start_level=0,
                                     augment_consistency_coeff=ALPHA, **dict(ARMS)[args.arm])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    runner.learner.save()
    runner.close_envs()
    del runner
    rates = {}
    episodes = -(-EVAL_BALLS // e2e.BALLS)
    for name, flags in (("train", []), ("test", [f"--pixel_catch_start_level={TEST_START}", f"--pixel_catch_levels={TEST_LEVELS}"])):
        argv = ["--env=pixel_catch", f"--train_dir={train_dir}", "--experiment=ops", f"--max_num_episodes={episodes}"] + flags
        parser, _ = parse_sf_args(argv, evaluation=True)
        pc.add_pixel_catch_args(parser)
        status, avg = enjoy(parse_full_cfg(parser, argv))
        assert status == 0
        rates[name] = round((avg / e2e.BALLS + 1.0) / 2.0, 4)
    print(json.dumps(dict(leg="learning", arm=args.arm, seed=int(args.child_seed), alpha=ALPHA, flags=dict(ARMS)[args.arm],
                          wall_s=round(wall, 2), train_rate=rates["train"], test_rate=rates["test"],
                          gap=round(rates["train"] - rates["test"], 4), eval_balls_at_least=episodes * e2e.BALLS,
                          catch_rate_by_50_iterations=[round(e2e.rate(curve[i:i + 50]), 4) for i in range(0, len(curve), 50)],
                          curve=curve)), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--legs", default="kernel,train,learning")
    p.add_argument("--arm", default="shift")
    p.add_argument("--decoys", type=int, default=6)
    p.add_argument("--levels", type=int, default=8)
    p.add_argument("--child_seed", default="1")
    p.add_argument("--seeds", default="1,2,3")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--rounds", type=int, default=2, help="how often the pair of the train leg is repeated")
    p.add_argument("--steps", type=int, default=12)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--timeout", type=int, default=300)
    p.add_argument("--commit", default="", help="what the measured tree is, e.g. '<parent commit> + this change'")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_ops_bench.json"))
    p.add_argument("--learning_out", default=os.path.join(ROOT, "profiles", "augment_ops_learning.json"))
    args = p.parse_args()
    if args.child:
        return dict(kernel=kernel, train=train, learning=learning)[args.child](args)
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    legs = args.legs.split(",")
    order = [("kernel", None, None)] if "kernel" in legs else []
    if "train" in legs:
        order += [("train", arm, None) for _ in range(args.rounds) for arm, _ in TRAIN_ARMS]
    if "learning" in legs:
        order += [("learning", arm, seed) for seed in args.seeds.split(",") for arm, _ in ARMS]
    results = []
    for which, arm, seed in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [
            f"--{k}={getattr(args, k)}" for k in ("steps", "warmup", "reps", "windows", "iters", "decoys", "levels")]
        cmd += [f"--arm={arm}"] if arm is not None else []
        cmd += [f"--child_seed={seed}"] if seed is not None else []
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            rc, line, err = r.returncode, [x for x in r.stdout.splitlines() if x.startswith("{")], r.stderr[-800:]
        except subprocess.TimeoutExpired:
            rc, line, err = 124, [], f"no result within {args.timeout} s"
        results.append(json.loads(line[-1]) if line and rc == 0 else dict(leg=which, arm=arm, seed=seed, rc=rc, err=err))
        print(json.dumps({k: v for k, v in results[-1].items() if k != "curve"}), flush=True)
        if rc != 0:  # nothing more is started on the device after a failed leg
            break
    stamp = dict(commit=args.commit, source_sha16=build.source_sha16(), host=socket.gethostname())
    kt = [r for r in results if r.get("leg") in ("kernel", "train")]
    if kt:
        summary = {}
        tr = [r for r in kt if "train_ms_per_iteration" in r]
        if tr:
            mean = lambda arm, k: round(sum(r[k] for r in tr if r["arm"] == arm) / max(1, sum(r["arm"] == arm for r in tr)), 3)  # noqa: E731
            summary["train"] = {f"{arm}_{k}": mean(arm, k) for arm, _ in TRAIN_ARMS for k in ("train_ms_per_iteration", "env_steps_per_s")}
            summary["train"]["all_three_minus_shift_only_ms_per_sgd_step"] = round(
                (summary["train"]["all_three_train_ms_per_iteration"] - summary["train"]["shift_only_train_ms_per_iteration"]) / 4, 3)
            summary["train"]["arms"] = {arm: flags for arm, flags in TRAIN_ARMS}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(stamp, summary=summary, results=kt), f, indent=1)
        print(json.dumps(summary), flush=True)
    lr = [r for r in results if r.get("leg") == "learning"]
    if lr:
        ok = [r for r in lr if "train_rate" in r]
        table = {f"{r['arm']}_seed{r['seed']}": dict(train=r["train_rate"], test=r["test_rate"], gap=r["gap"]) for r in ok}
        mean = {arm: {k: round(sum(r[k] for r in ok if r["arm"] == arm) / max(1, sum(r["arm"] == arm for r in ok)), 4)
                      for k in ("train_rate", "test_rate", "gap")} for arm, _ in ARMS if any(r["arm"] == arm for r in ok)}
        curves = {f"{r['arm']}_seed{r['seed']}": r["catch_rate_by_50_iterations"] for r in ok}
        os.makedirs(os.path.dirname(os.path.abspath(args.learning_out)), exist_ok=True)
        with open(args.learning_out, "w") as f:
            json.dump(dict(stamp, protocol="profiles/pixel_catch_levels_learning.json: 36 x 36 x 4, 1024 agents, convnet_simple, "
                                           "rollout 8; every arm with augment_consistency_coeff = 0.1",
                           game=dict(decoys=args.decoys, train_levels=[0, args.levels],
                                     test_levels=[TEST_START, TEST_START + TEST_LEVELS]),
                           arms={arm: dict(flags, augment_consistency_coeff=ALPHA) for arm, flags in ARMS},
                           iterations=args.iters, catch_rates=table, mean_over_seeds=mean, catch_rate_by_50_iterations=curves,
                           results=lr), f)
        print(json.dumps(dict(catch_rates=table, mean_over_seeds=mean)), flush=True)


if __name__ == "__main__":
    main()
