"""--augment_consistency_coeff (DrAC) measured: the consistency-loss launch beside the PPO-loss launch,
Learner.train with the consistency loss on against off, and learning on PixelCatch.  Every leg is a child process of its own
on the same GPU; legs that are compared ALTERNATE.

 * kernel: sf_consistency_loss on the two halves of a [2 x 32768, 1 + A] heads matrix (A = 6 and A = 4096, Discrete), rows
           read through a shuffled index into a dataset of 131072 rows, and — alternating with it, on the same matrix, index
           and dataset — sf_ppo_loss on the first half.  HIP events around windows of back-to-back launches after a warm-up
           window, the median window.  Bytes: what the algorithm needs (two heads rows read, one gradient row written, the
           index and the validity byte), against the 8.0 TB/s HBM3E peak.
 * train:  bench.py's c2 workload (4096 envs, rollout 32, 4 minibatches of 32768, Nature CNN) with --augment_random_shift=4;
           wall clock of the runner's train phase per iteration (one Learner.train call = 4 SGD steps), alpha = 0.1 against
           alpha = 0, and the peak of torch's allocator.
 * learning: the protocol of profiles/pixel_catch_learning.json (tests/test_gpu_pixel_catch_e2e.py's learning run, 36 x 36 x 4,
           1024 agents, 400 iterations), seeds 1, 2, 3, three arms: shift 4 with alpha = 0.1 (DrAC), shift 4 alone (RAD), no
           augmentation.  Catch rate over iterations 0-50 / 100-150 / 200-250 / 350-400.  Written to a file of its own.

  python tools/drac_bench.py [--legs kernel,train,learning] [--out profiles/drac_bench.json]
                             [--learning_out profiles/drac_learning.json] [--label TEXT]"""
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
E, T, N, PAD, ALPHA = 4096, 32, 32768, 4, 0.1
WINDOWS = ((0, 50), (100, 150), (200, 250), (350, 400))


def kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import lib
    out = dict(leg="kernel", rows=N, dataset_rows=E * T, windows=args.windows, launches_per_window=args.reps,
               hbm_peak_tb_per_s=HBM_PEAK_TBS, device=torch.cuda.get_device_name(0), widths={})
    g = torch.Generator(device="cuda").manual_seed(1)
    D = E * T
    index = torch.randperm(D, generator=g, device="cuda")[:N].to(torch.int32)
    valids = torch.rand(D, generator=g, device="cuda") > 0.02
    for A in (6, 4096):
        ld = (1 + A + 3) // 4 * 4
        heads = torch.randn((2 * N, ld), generator=g, device="cuda") * 2.0
        g_heads = torch.zeros_like(heads)
        old_params = torch.randn((D, A), generator=g, device="cuda") * 2.0
        actions = torch.randint(0, A, (D, 1), generator=g, device="cuda").float()
        old_logp = torch.log_softmax(old_params, -1).gather(1, actions.long())[:, 0].contiguous()
        old_values, adv, targets = (torch.randn(D, generator=g, device="cuda") for _ in range(3))
        cfg = lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.2, value_loss_coeff=0.5, exploration_coeff=0.003, kl_coeff=0.0,
                              exploration_kind=1, action_kind=0, dense_adv=0)
        mom = torch.zeros(3, dtype=torch.float64, device="cuda")
        lib.moments(adv, valids, index, N, mom)
        sums, csums = (torch.zeros(8, dtype=torch.float64, device="cuda") for _ in range(2))
        ratio = torch.zeros(N, device="cuda")

        def ppo():
            lib.ppo_loss(heads[:N, 1:], ld, heads[:N, 0], ld, actions, old_logp, old_params, old_values, adv, targets, valids,
                         index, 0, N, A, cfg, mom, sums, g_heads[:N, 1:], g_heads[:N, 0], ratio_out=ratio)

        def cons():
            lib.consistency_loss(heads[:N, 1:], heads[N:, 1:], ld, heads[:N, 0], heads[N:, 0], ld, valids, index, 0, N, A, 0,
                                 ALPHA, ALPHA, mom, csums[:4], g_heads[N:, 1:], g_heads[N:, 0])
        fns = dict(consistency_loss=cons, ppo_loss=ppo)

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
        for _ in range(args.windows):  # alternate: both see the same machine
            for name, fn in fns.items():
                res[name].append(window(fn))
        row = 4 * (1 + A)
        moved = dict(consistency_loss=N * (3 * row + 5), ppo_loss=N * (2 * row + 4 * A + 4 * 7 + 5))
        w = out["widths"][str(A)] = dict(heads_ld=ld, kernel="k_consistency_loss_wide" if A > 128 else "k_consistency_loss")
        for name, ms in res.items():
            med = sorted(ms)[len(ms) // 2]
            w[name] = dict(us_per_launch_median=round(med * 1e3, 2), us_per_launch_min=round(min(ms) * 1e3, 2),
                           us_per_launch_max=round(max(ms) * 1e3, 2), bytes_needed_per_launch=moved[name],
                           tb_per_s_median=round(moved[name] / (med * 1e-3) / 1e12, 3),
                           share_of_hbm_peak=round(moved[name] / (med * 1e-3) / 1e12 / HBM_PEAK_TBS, 3))
        w["consistency_over_ppo_loss_time"] = round(w["consistency_loss"]["us_per_launch_median"] /
                                                    w["ppo_loss"]["us_per_launch_median"], 3)
        assert float(csums[3]) == float(valids[index.long()].sum()) and torch.isfinite(g_heads).all()
        del heads, g_heads, old_params
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
    cfg.augment_random_shift, cfg.augment_consistency_coeff = int(args.pad), float(args.alpha)
    register_env(env_name, env_factory)
    cfg, runner = make_runner(cfg)
    runner.init()
    for _ in range(args.warmup):
        runner.iteration()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t_train0, t_roll0 = float(runner.timing.get("train", 0.0)), float(runner.timing.get("rollout", 0.0))
    step0, t0 = runner.learner.train_step, time.perf_counter()
    for _ in range(args.steps):
        runner.iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sgd = runner.learner.train_step - step0
    train_ms = 1e3 * (float(runner.timing.get("train", 0.0)) - t_train0) / args.steps
    print(json.dumps(dict(leg="train", pad=int(args.pad), alpha=float(args.alpha), iterations=args.steps, sgd_steps=sgd,
                          train_ms_per_iteration=round(train_ms, 3), train_ms_per_sgd_step=round(train_ms * args.steps / sgd, 3),
                          rollout_ms_per_iteration=round(1e3 * (float(runner.timing.get("rollout", 0.0)) - t_roll0) / args.steps, 3),
                          wall_ms_per_iteration=round(1e3 * dt / args.steps, 3),
                          env_steps_per_s=round(args.steps * E * T / dt, 1),
                          peak_memory_allocated_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                          last_summary={k: v for k, v in dict(runner.learner.last_summary).items() if k.startswith("consistency")},
                          device=torch.cuda.get_device_name(0))), flush=True)


def learning(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile

    import torch
    import test_gpu_pixel_catch_e2e as e2e
    t0 = time.perf_counter()
    curve, runner = e2e.learning_run(int(args.child_seed), args.iters, train_dir=tempfile.mkdtemp(prefix="sf_drac_learn_"),
                                     augment_random_shift=int(args.pad), augment_consistency_coeff=float(args.alpha))
    torch.cuda.synchronize()
    print(json.dumps(dict(leg="learning", seed=int(args.child_seed), pad=int(args.pad), alpha=float(args.alpha),
                          wall_s=round(time.perf_counter() - t0, 2),
                          catch_rate_windows={f"{a}-{b}": round(e2e.rate(curve[a:b]), 4) for a, b in WINDOWS if b <= len(curve)},
                          catch_rate_by_50_iterations=[round(e2e.rate(curve[i:i + 50]), 4) for i in range(0, len(curve), 50)],
                          last_summary={k: v for k, v in dict(runner.learner.last_summary).items() if k.startswith("consistency")},
                          curve=curve)), flush=True)


def arm(r):
    return "drac" if r["alpha"] > 0 else ("rad" if r["pad"] else "off")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--legs", default="kernel,train,learning")
    p.add_argument("--pad", type=int, default=PAD)
    p.add_argument("--alpha", type=float, default=ALPHA)
    p.add_argument("--child_seed", default="1")
    p.add_argument("--seeds", default="1,2,3")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--rounds", type=int, default=3, help="how often the (on, off) pair of the train leg is repeated")
    p.add_argument("--steps", type=int, default=12)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--timeout", type=int, default=300)
    p.add_argument("--label", default="this tree")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "drac_bench.json"))
    p.add_argument("--learning_out", default=os.path.join(ROOT, "profiles", "drac_learning.json"))
    args = p.parse_args()
    if args.child:
        return dict(kernel=kernel, train=train, learning=learning)[args.child](args)
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    legs = args.legs.split(",")
    order = [("kernel", None, None, None)] if "kernel" in legs else []
    if "train" in legs:
        order += [("train", args.pad, alpha, None) for _ in range(args.rounds) for alpha in (args.alpha, 0.0)]
    if "learning" in legs:
        order += [("learning", pad, alpha, seed) for seed in args.seeds.split(",")
                  for pad, alpha in ((args.pad, args.alpha), (args.pad, 0.0), (0, 0.0))]
    results = []
    for which, pad, alpha, seed in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [
            f"--{k}={getattr(args, k)}" for k in ("steps", "warmup", "reps", "windows", "iters")]
        cmd += [f"--pad={pad}", f"--alpha={alpha}"] if pad is not None else []
        cmd += [f"--child_seed={seed}"] if seed is not None else []
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        results.append(json.loads(line[-1]) if line and r.returncode == 0 else dict(leg=which, pad=pad, alpha=alpha, rc=r.returncode,
                                                                                   err=r.stderr[-800:]))
        print(json.dumps({k: v for k, v in results[-1].items() if k != "curve"}), flush=True)
        if r.returncode != 0:  # nothing more is started on the device after a failed leg
            break
    stamp = dict(source_sha16=build.source_sha16(), tree=args.label, host=socket.gethostname())
    summary = {}
    tr = [r for r in results if r.get("leg") == "train" and "train_ms_per_iteration" in r]
    if tr:
        def median(on, k):
            v = sorted(r[k] for r in tr if (r["alpha"] > 0) == on)
            return v[len(v) // 2] if v else None
        s = summary["train"] = {f"{'on' if on else 'off'}_{k}": median(on, k) for on in (True, False)
                                for k in ("train_ms_per_iteration", "train_ms_per_sgd_step", "env_steps_per_s",
                                          "peak_memory_allocated_mib")}
        if s["on_train_ms_per_sgd_step"] and s["off_train_ms_per_sgd_step"]:
            s["on_over_off_sgd_step_time"] = round(s["on_train_ms_per_sgd_step"] / s["off_train_ms_per_sgd_step"], 3)
    kr = [r for r in results if r.get("leg") == "kernel" and "widths" in r]
    if kr:
        summary["kernel"] = {A: {k: w[k]["us_per_launch_median"] for k in ("consistency_loss", "ppo_loss")}
                             for A, w in kr[0]["widths"].items()}
    if tr or kr or any("rc" in r for r in results if r.get("leg") != "learning"):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(stamp, order=[o for o in order if o[0] != "learning"], summary=summary,
                           results=[r for r in results if r.get("leg") != "learning"]), f, indent=1)
    lr = [r for r in results if r.get("leg") == "learning"]
    if lr:
        table = {f"{arm(r)}_seed{r['seed']}": r["catch_rate_windows"] for r in lr if "catch_rate_windows" in r}
        summary["learning"] = table
        os.makedirs(os.path.dirname(os.path.abspath(args.learning_out)), exist_ok=True)
        with open(args.learning_out, "w") as f:
            json.dump(dict(stamp, protocol="profiles/pixel_catch_learning.json: 36 x 36 x 4, 1024 agents, convnet_simple, rollout 8",
                           arms=dict(drac=f"augment_random_shift={args.pad} augment_consistency_coeff={args.alpha}",
                                     rad=f"augment_random_shift={args.pad}", off="no augmentation"),
                           iterations=args.iters, catch_rate_windows=table,
                           results=[{k: v for k, v in r.items() if k != "curve"} for r in lr]), f, indent=1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
