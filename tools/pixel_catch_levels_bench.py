"""PixelCatch levels measured: what the decoys cost the step-and-render launch, and whether a policy trained
on a handful of levels plays held-out levels worse, with and without the random shift and DrAC.

 * kernel:   sf_pixcatch_step_levels with 8 decoys at 4096 x 4 x 84 x 84 into rotating columns of a slab that does not fit
             the caches, HIP-event timed over windows of back-to-back launches, ALTERNATING with sf_pixcatch_step on the same
             columns (the protocol of tools/pixel_catch_bench.py); median and spread per window and the ratio of the medians.
 * learning: the protocol of profiles/pixel_catch_learning.json (the learning run of tests/test_gpu_pixel_catch_e2e.py:
             36 x 36 x 4, 1024 agents, convnet_simple, rollout 8, 400 iterations), seeds 1, 2, 3, on 6 decoys and the train
             levels [0, 8); three arms: no augmentation, --augment_random_shift=4, and the shift with
             --augment_consistency_coeff=0.1.  Every final checkpoint is played by enjoy() (sampled actions) on the train
             levels and on the held-out levels [1 000 000, 1 100 000) until at least 20 000 balls have landed (binomial
             standard error at most 0.004); catch rate = (mean episode return / balls + 1) / 2.  Each run is a child process.

  python tools/pixel_catch_levels_bench.py [--legs kernel,learning] [--decoys 6] [--levels 8] [--seeds 1,2,3] [--iters 400]
                                           [--out profiles/pixel_catch_levels_bench.json]
                                           [--learning_out profiles/pixel_catch_levels_learning.json] [--commit TEXT]"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K, H, W = 4096, 4, 84, 84
FRAME_BYTES = K * H * W
HBM_PEAK_TBS = 8.0
ARMS = (("off", 0, 0.0), ("shift", 4, 0.0), ("shift_drac", 4, 0.1))
TEST_START, TEST_LEVELS, EVAL_BALLS = 1000000, 100000, 20000


def kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import lib
    Tk, nd = 8, 8  # columns: 4096 x 9 x 28 224 B = 1.04 GB
    slab = torch.zeros((B, Tk + 1, K, H, W), dtype=torch.uint8, device="cuda")
    state, state_lv = (torch.zeros((B, lib.pixcatch_state_words(K)), dtype=torch.int32, device="cuda") for _ in range(2))
    act = torch.randint(0, 3, (B,), dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float32, device="cuda")
    term = torch.zeros(B, dtype=torch.bool, device="cuda")
    lib.pixcatch_reset(state, slab[:, 0], 0, 0, 4)
    lib.pixcatch_reset_levels(state_lv, slab[:, 0], 0, 0, 4, nd, 0, 0)

    def plain(t):
        lib.pixcatch_step(state, act, slab[:, t + 1], rew, term, 0, 0, 4)

    def levels(t):
        lib.pixcatch_step_levels(state_lv, act, slab[:, t + 1], rew, term, 0, 0, 4, nd, 0, 0)
    fns = dict(pixcatch_step=plain, pixcatch_step_levels=levels)

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
    assert torch.equal(state, state_lv)  # the same game: decoys change frames only
    moved = B * FRAME_BYTES
    out = dict(leg="kernel", envs=B, frame=[K, H, W], decoys=nd, levels=0, bytes_written_per_step=moved,
               launches_per_window=args.reps * Tk, windows=args.windows, hbm_peak_tb_per_s=HBM_PEAK_TBS,
               device=torch.cuda.get_device_name(0))
    for name, ms in res.items():
        med = sorted(ms)[len(ms) // 2]
        out[name] = dict(us_per_step_median=round(med * 1e3, 2), us_per_step_min=round(min(ms) * 1e3, 2),
                         us_per_step_max=round(max(ms) * 1e3, 2), tb_per_s_median=round(moved / (med * 1e-3) / 1e12, 3),
                         share_of_hbm_peak=round(moved / (med * 1e-3) / 1e12 / HBM_PEAK_TBS, 3))
    out["levels_over_plain_median"] = round(out["pixcatch_step_levels"]["us_per_step_median"] /
                                            out["pixcatch_step"]["us_per_step_median"], 4)
    print(json.dumps(out), flush=True)


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
    train_dir, t0 = tempfile.mkdtemp(prefix="sf_pixel_catch_levels_"), time.perf_counter()
    curve, runner = e2e.learning_run(int(args.child_seed), args.iters, train_dir=train_dir, experiment="levels",
                                     pixel_catch_decoys=args.decoys, pixel_catch_levels=args.levels, pixel_catch_start_level=0,
                                     augment_random_shift=int(args.pad), augment_consistency_coeff=float(args.alpha))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    runner.learner.save()
    runner.close_envs()
    del runner
    rates = {}
    episodes = -(-EVAL_BALLS // e2e.BALLS)
    for name, flags in (("train", []), ("test", [f"--pixel_catch_start_level={TEST_START}", f"--pixel_catch_levels={TEST_LEVELS}"])):
        argv = ["--env=pixel_catch", f"--train_dir={train_dir}", "--experiment=levels", f"--max_num_episodes={episodes}"] + flags
        parser, _ = parse_sf_args(argv, evaluation=True)
        pc.add_pixel_catch_args(parser)
        status, avg = enjoy(parse_full_cfg(parser, argv))
        assert status == 0
        rates[name] = round((avg / e2e.BALLS + 1.0) / 2.0, 4)
    print(json.dumps(dict(leg="learning", arm=args.arm, seed=int(args.child_seed), pad=int(args.pad), alpha=float(args.alpha),
                          decoys=args.decoys, train_levels=[0, args.levels], test_levels=[TEST_START, TEST_START + TEST_LEVELS],
                          wall_s=round(wall, 2), train_rate=rates["train"], test_rate=rates["test"],
                          gap=round(rates["train"] - rates["test"], 4), eval_balls_at_least=episodes * e2e.BALLS,
                          catch_rate_by_50_iterations=[round(e2e.rate(curve[i:i + 50]), 4) for i in range(0, len(curve), 50)],
                          curve=curve)), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--legs", default="kernel,learning")
    p.add_argument("--arm", default="off")
    p.add_argument("--pad", type=int, default=0)
    p.add_argument("--alpha", type=float, default=0.0)
    p.add_argument("--decoys", type=int, default=6)
    p.add_argument("--levels", type=int, default=8)
    p.add_argument("--child_seed", default="1")
    p.add_argument("--seeds", default="1,2,3")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--timeout", type=int, default=300)
    p.add_argument("--commit", default="", help="what the measured tree is, e.g. '<parent commit> + this change'")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_catch_levels_bench.json"))
    p.add_argument("--learning_out", default=os.path.join(ROOT, "profiles", "pixel_catch_levels_learning.json"))
    args = p.parse_args()
    if args.child:
        return dict(kernel=kernel, learning=learning)[args.child](args)
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    legs = args.legs.split(",")
    order = [("kernel", None, None, None, None)] if "kernel" in legs else []
    if "learning" in legs:
        order += [("learning", arm, pad, alpha, seed) for seed in args.seeds.split(",") for arm, pad, alpha in ARMS]
    results = []
    for which, arm, pad, alpha, seed in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [
            f"--{k}={getattr(args, k)}" for k in ("reps", "windows", "iters", "decoys", "levels")]
        cmd += [f"--arm={arm}", f"--pad={pad}", f"--alpha={alpha}", f"--child_seed={seed}"] if arm is not None else []
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        results.append(json.loads(line[-1]) if line and r.returncode == 0 else dict(leg=which, arm=arm, seed=seed, rc=r.returncode,
                                                                                   err=r.stderr[-800:]))
        print(json.dumps({k: v for k, v in results[-1].items() if k != "curve"}), flush=True)
        if r.returncode != 0:  # nothing more is started on the device after a failed leg
            break
    stamp = dict(commit=args.commit, source_sha16=build.source_sha16(), host=socket.gethostname())
    kr = [r for r in results if r.get("leg") == "kernel"]
    if kr:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(stamp, yardstick="sf_pixcatch_step, 28.0 us in profiles/pixel_catch_bench.json, re-measured here",
                           results=kr), f, indent=1)
    lr = [r for r in results if r.get("leg") == "learning"]
    if lr:
        ok = [r for r in lr if "train_rate" in r]
        table = {f"{r['arm']}_seed{r['seed']}": dict(train=r["train_rate"], test=r["test_rate"], gap=r["gap"]) for r in ok}
        mean = {arm: {k: round(sum(r[k] for r in ok if r["arm"] == arm) / max(1, sum(r["arm"] == arm for r in ok)), 4)
                      for k in ("train_rate", "test_rate", "gap")} for arm, _, _ in ARMS if any(r["arm"] == arm for r in ok)}
        os.makedirs(os.path.dirname(os.path.abspath(args.learning_out)), exist_ok=True)
        with open(args.learning_out, "w") as f:
            json.dump(dict(stamp, protocol="profiles/pixel_catch_learning.json: 36 x 36 x 4, 1024 agents, convnet_simple, rollout 8",
                           game=dict(decoys=args.decoys, train_levels=[0, args.levels],
                                     test_levels=[TEST_START, TEST_START + TEST_LEVELS]),
                           arms={arm: dict(augment_random_shift=pad, augment_consistency_coeff=alpha) for arm, pad, alpha in ARMS},
                           iterations=args.iters, catch_rates=table, mean_over_seeds=mean, results=lr), f)
        print(json.dumps(dict(catch_rates=table, mean_over_seeds=mean)), flush=True)


if __name__ == "__main__":
    main()
