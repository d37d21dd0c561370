"""--augment_random_shift measured: the gather launch alone, Learner.train with the flag on against off, and
learning on PixelCatch with the flag on against off.  Every leg is a child process of its own on the same GPU; legs that are
compared ALTERNATE (on, off, on, off, ...).

 * kernel: sf_random_shift_gather (pad 4) on a shuffled minibatch of 32768 samples of 4 x 84 x 84 u8 indexed out of a
           [4096, 33, 4, 84, 84] slab (3.8 GB: nothing stays in the caches), and the same at 3 x 72 x 128; beside it, on the
           same bytes and alternating with it: the launch with pad 0 (the plain indexed gather), sf_copy_rows (dense to dense,
           no index, no shift) and a torch formulation (index_select of the rows, then the replicate-pad-and-crop as ONE
           advanced-index gather with clamped row / column indices).  HIP events around windows of back-to-back launches after
           a warm-up window, the median window; rates against the 8.0 TB/s HBM3E peak.
 * train:  bench.py's c2 workload (4096 envs, rollout 32, 4 minibatches of 32768, Nature CNN); wall clock of the runner's
           train phase per iteration (one Learner.train call = 4 SGD steps), flag on (pad 4) against off.
 * learning: the protocol of profiles/pixel_catch_learning.json (tests/test_gpu_pixel_catch_e2e.py's learning run, 36 x 36 x 4,
           1024 agents, 400 iterations), seeds 1, 2, 3, flag on (pad 4) against off: catch rate per 50 iterations.

  python tools/augment_shift_bench.py [--legs kernel,train,learning] [--out profiles/augment_shift_bench.json] [--label TEXT]"""
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
E, T, N, PAD = 4096, 32, 32768, 4


def kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import lib
    out = dict(leg="kernel", samples=N, slab=[E, T + 1], pad=PAD, windows=args.windows, launches_per_window=args.reps,
               hbm_peak_tb_per_s=HBM_PEAK_TBS, device=torch.cuda.get_device_name(0), shapes={})
    for shape in ((4, 84, 84), (3, 72, 128)):
        C, H, W = shape
        S = C * H * W
        slab = torch.randint(0, 256, (E, T + 1, C, H, W), dtype=torch.uint8, device="cuda")
        flat = slab.view(E * (T + 1), S)
        g = torch.Generator(device="cuda").manual_seed(1)
        index = torch.randperm(E * T, generator=g, device="cuda")[:N].to(torch.int32)
        dense, dense2 = (torch.empty((N, S), dtype=torch.uint8, device="cuda") for _ in range(2))
        rows = (index.long() + index.long() // T)
        ar_y, ar_x = torch.arange(H, device="cuda"), torch.arange(W, device="cuda")
        dy = torch.randint(0, 2 * PAD + 1, (N,), generator=g, device="cuda")
        dx = torch.randint(0, 2 * PAD + 1, (N,), generator=g, device="cuda")

        def torch_form():
            sel = flat.index_select(0, rows).view(N, C, H, W)
            ys = (ar_y[None, :] + dy[:, None] - PAD).clamp_(0, H - 1)
            xs = (ar_x[None, :] + dx[:, None] - PAD).clamp_(0, W - 1)
            return sel.gather(2, ys[:, None, :, None].expand(N, C, H, W)).gather(3, xs[:, None, None, :].expand(N, C, H, W))
        step = [0]

        def shift(pad):
            step[0] += 1
            lib.random_shift_gather(dense, slab, N, shape, index=index, traj_T=T, pad=pad, seed=7, draw_id=step[0])
        fns = dict(random_shift_gather=(lambda: shift(PAD), args.reps), indexed_gather_pad0=(lambda: shift(0), args.reps),
                   copy_rows=(lambda: lib.copy_rows(dense2, dense), args.reps), torch_formulation=(torch_form, max(1, args.reps // 5)))

        def window(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps
        for fn, reps in fns.values():
            window(fn, reps)  # warm-up
        res = {name: [] for name in fns}
        for _ in range(args.windows):  # alternate: all of them see the same machine
            for name, (fn, reps) in fns.items():
                res[name].append(window(fn, reps))
        moved = 2 * N * S
        sh = out["shapes"]["x".join(map(str, shape))] = dict(sample_bytes=S, bytes_read_plus_written_per_launch=moved)
        for name, ms in res.items():
            med = sorted(ms)[len(ms) // 2]
            sh[name] = dict(us_per_launch_median=round(med * 1e3, 2), us_per_launch_min=round(min(ms) * 1e3, 2),
                            us_per_launch_max=round(max(ms) * 1e3, 2), tb_per_s_median=round(moved / (med * 1e-3) / 1e12, 3),
                            share_of_hbm_peak=round(moved / (med * 1e-3) / 1e12 / HBM_PEAK_TBS, 3))
        for name in ("random_shift_gather", "indexed_gather_pad0", "torch_formulation"):
            sh[name + "_over_copy_rows_time"] = round(sh[name]["us_per_launch_median"] / sh["copy_rows"]["us_per_launch_median"], 3)
        del slab, flat, dense, dense2
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
    cfg.augment_random_shift = int(args.pad)
    register_env(env_name, env_factory)
    cfg, runner = make_runner(cfg)
    runner.init()
    for _ in range(args.warmup):
        runner.iteration()
    torch.cuda.synchronize()
    t_train0, t_roll0 = float(runner.timing.get("train", 0.0)), float(runner.timing.get("rollout", 0.0))
    step0, t0 = runner.learner.train_step, time.perf_counter()
    for _ in range(args.steps):
        runner.iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sgd = runner.learner.train_step - step0
    print(json.dumps(dict(leg="train", pad=int(args.pad), iterations=args.steps, sgd_steps=sgd,
                          train_ms_per_iteration=round(1e3 * (float(runner.timing.get("train", 0.0)) - t_train0) / args.steps, 3),
                          rollout_ms_per_iteration=round(1e3 * (float(runner.timing.get("rollout", 0.0)) - t_roll0) / args.steps, 3),
                          wall_ms_per_iteration=round(1e3 * dt / args.steps, 3),
                          env_steps_per_s=round(args.steps * E * T / dt, 1), reuse_stats=dict(runner.learner.reuse_stats),
                          device=torch.cuda.get_device_name(0))), flush=True)


def learning(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile

    import torch
    import test_gpu_pixel_catch_e2e as e2e
    t0 = time.perf_counter()
    curve, runner = e2e.learning_run(int(args.child_seed), args.iters, train_dir=tempfile.mkdtemp(prefix="sf_augment_learn_"),
                                     augment_random_shift=int(args.pad))
    torch.cuda.synchronize()
    print(json.dumps(dict(leg="learning", seed=int(args.child_seed), pad=int(args.pad), wall_s=round(time.perf_counter() - t0, 2),
                          catch_rate_by_50_iterations=[round(e2e.rate(curve[i:i + 50]), 4) for i in range(0, len(curve), 50)],
                          catch_rate_last_50=round(e2e.rate(curve[-50:]), 4), curve=curve)), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--legs", default="kernel,train,learning")
    p.add_argument("--pad", type=int, default=PAD)
    p.add_argument("--child_seed", default="1")
    p.add_argument("--seeds", default="1,2,3")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--rounds", type=int, default=2, help="how often the (on, off) pair of the train leg is repeated")
    p.add_argument("--steps", type=int, default=12)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--timeout", type=int, default=300)
    p.add_argument("--label", default="this tree")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_shift_bench.json"))
    args = p.parse_args()
    if args.child:
        return dict(kernel=kernel, train=train, learning=learning)[args.child](args)
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    legs = args.legs.split(",")
    order = [("kernel", None, None)] if "kernel" in legs else []
    if "train" in legs:
        order += [("train", pad, None) for _ in range(args.rounds) for pad in (args.pad, 0)]
    if "learning" in legs:
        order += [("learning", pad, seed) for seed in args.seeds.split(",") for pad in (args.pad, 0)]
    results = []
    for which, pad, seed in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [
            f"--{k}={getattr(args, k)}" for k in ("steps", "warmup", "reps", "windows", "iters")]
        cmd += [f"--pad={pad}"] if pad is not None else []
        cmd += [f"--child_seed={seed}"] if seed is not None else []
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        results.append(json.loads(line[-1]) if line and r.returncode == 0 else dict(leg=which, pad=pad, rc=r.returncode,
                                                                                   err=r.stderr[-800:]))
        print(json.dumps({k: v for k, v in results[-1].items() if k != "curve"}), flush=True)
        if r.returncode != 0:
            break
    summary = {}
    tr = [r for r in results if r.get("leg") == "train" and "train_ms_per_iteration" in r]
    if tr:
        mean = lambda pad, k: round(sum(r[k] for r in tr if bool(r["pad"]) == pad) / max(1, sum(bool(r["pad"]) == pad for r in tr)), 3)
        summary["train"] = dict(on_train_ms_per_iteration=mean(True, "train_ms_per_iteration"),
                                off_train_ms_per_iteration=mean(False, "train_ms_per_iteration"),
                                on_env_steps_per_s=mean(True, "env_steps_per_s"), off_env_steps_per_s=mean(False, "env_steps_per_s"))
        summary["train"]["on_minus_off_ms_per_sgd_step"] = round(
            (summary["train"]["on_train_ms_per_iteration"] - summary["train"]["off_train_ms_per_iteration"]) / 4, 3)
    lr = [r for r in results if r.get("leg") == "learning" and "catch_rate_last_50" in r]
    if lr:
        summary["learning"] = {("on" if r["pad"] else "off") + f"_seed{r['seed']}": r["catch_rate_by_50_iterations"] for r in lr}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(source_sha16=build.source_sha16(), tree=args.label, host=socket.gethostname(), order=order, summary=summary,
                       results=[{k: v for k, v in r.items() if k != "curve"} for r in results]), f, indent=1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
