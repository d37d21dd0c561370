"""Host-env ingest with the frame stack kept on the device (--device_framestack) against stacks delivered by the env, each
leg in a child process of its own on the same GPU:

 * leg A: HostFrameVecEnv frames (4, 84, 84), device_framestack=1 — every step ships the whole stack over PCIe;
 * leg B: HostFrameVecEnv frames (1, 84, 84), device_framestack=4 — every step ships one frame, sf_framestack_step
          completes the stack in the slab;
 * kernel: sf_framestack_step on the columns of a [1024, 33, 4, 84, 84] u8 slab against sf_copy_rows moving the same
          bytes (the k - 1 shifted slots of every row), HIP-event timed over back-to-back launches, alternating.

Workload of the legs: bench.py's c3 line — 1024 agents (4 env worker processes x 2 instances x 128 agents, 2 sampling
splits), Nature CNN, rollout 32, async APPO.

  python tools/framestack_bench.py [--legs A,B,kernel] [--steps 40] [--warmup 3] [--out profiles/framestack_bench.json]

`--legs A` runs on a tree without the flag as well (the parent's path).  The stand-in env is env-bound: the legs report what
is moved and how long the DMA engine and the kernel take, not a PCIe-bound speed-up."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, K, FRAME = 1024, 32, 4, (1, 84, 84)
FRAME_BYTES = FRAME[0] * FRAME[1] * FRAME[2]


def leg(args, which):
    sys.path.insert(0, ROOT)
    import tempfile

    import torch
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_host_frame_env
    from sample_factory_amd.train import make_runner
    register_env("host_atari", make_host_frame_env)
    W = args.env_workers
    extra = dict(device_framestack=K, host_env_obs_shape=list(FRAME)) if which == "B" else {}
    cfg = default_cfg(
        env="host_atari", use_rnn=False, recurrence=1, encoder_conv_architecture="convnet_atari", nonlinearity="relu",
        encoder_conv_mlp_layers=[512], obs_scale=255.0, normalize_input=False, normalize_returns=False,
        exploration_loss_coeff=0.01, max_grad_norm=0.5, learning_rate=0.00025, adam_eps=1e-5,
        train_dir=tempfile.mkdtemp(prefix="sf_framestack_bench_"), rollout=T, batch_size=B * T // 4, num_batches_per_epoch=4,
        num_epochs=4, async_rl=True, serial_mode=False, batched_sampling=True, env_workers_mode="process", num_workers=W,
        num_envs_per_worker=2, worker_num_splits=2, synthetic_num_agents=B // (2 * W), env_gpu_observations=False,
        env_gpu_actions=False, seed=0, **extra)
    cfg, runner = make_runner(cfg)
    assert runner.init() == 0
    try:
        for _ in range(args.warmup):
            runner.iteration()
        for sm in runner.samplers:
            sm.ingest_prof, sm.h2d_bytes = {}, 0
        steps0, rounds0 = runner.learner.env_steps, runner.sampling_rounds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            runner.iteration()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        env_steps_done = runner.learner.env_steps - steps0
        runner.stop_sampler_thread()
        torch.cuda.synchronize()
        rounds = max(1, runner.sampling_rounds - rounds0)
        h2d = sum(sm.h2d_bytes for sm in runner.samplers)
        dma_ms = dma_bytes = 0.0
        dma_rows = 0  # env steps whose observation the timed DMAs carried (one DMA = one step of one split's agents)
        host = dict(act_wait_s=0.0, env_step_s=0.0, stage_s=0.0)
        for sm in runner.samplers:
            for k in host:
                host[k] += sm.ingest_prof.get(k, 0.0)
            for e0, e1, nbytes in sm.ingest_prof.get("dma_events", []):
                dma_ms += e0.elapsed_time(e1)
                dma_bytes += nbytes
                dma_rows += sm.B
            sm.ingest_prof = None
        out = dict(leg=which, frames=list(FRAME) if which == "B" else [4, 84, 84],
                   device_framestack=int(getattr(cfg, "device_framestack", 1)),
                   env_steps_per_s=round(env_steps_done / dt, 1), wall_s=round(dt, 3),
                   sampling_rounds=rounds, obs_h2d_bytes_per_env_step=round(dma_bytes / max(1, dma_rows), 1),
                   h2d_bytes_all_kinds_in_region=int(h2d),
                   obs_dma_ms_per_rollout_step=round(B * dma_ms / max(1, dma_rows), 4),
                   obs_dma_gbs=round(dma_bytes / (dma_ms * 1e-3) / 1e9, 2) if dma_ms else None,
                   dma_share_of_wall_clock=round(dma_ms * 1e-3 / dt, 4), host_s={k: round(v, 3) for k, v in host.items()},
                   obs_dma_from_worker_pages_in_place=[sm._direct_ok.get("obs") for sm in runner.samplers])
        if which == "B":  # after the timed region: two more iterations with a HIP-event pair around every frame-stack launch
            from sample_factory_amd import lib
            key = ("framestack_step", B // 2, K, FRAME_BYTES)  # one launch per split and step: 512 rows
            lib.PROFILE, lib.PROFILE_ONLY = {}, {key}
            for _ in range(2):
                runner.iteration()
            runner.stop_sampler_thread()
            torch.cuda.synchronize()
            prof, lib.PROFILE, lib.PROFILE_ONLY = lib.PROFILE, None, None
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in prof.get(key, []))
            moved = 2 * (B // 2) * (K - 1) * FRAME_BYTES
            out["framestack_launches_timed"] = len(ms)
            if ms:
                med = ms[len(ms) // 2]
                out["framestack_us_per_launch_median"] = round(med * 1e3, 2)
                out["framestack_us_per_rollout_step"] = round(2 * med * 1e3, 2)  # 2 splits
                out["framestack_tb_per_s_median"] = round(moved / (med * 1e-3) / 1e12, 3)
    finally:
        runner.close_envs()
    print(json.dumps(out), flush=True)


def kernel(args):
    """sf_framestack_step (in-place frame, no row done: the steady state) against sf_copy_rows on the same bytes"""
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import lib
    slab = torch.randint(0, 256, (B, T + 1, K * FRAME[0], FRAME[1], FRAME[2]), dtype=torch.uint8, device="cuda")
    term = torch.zeros(B, dtype=torch.bool, device="cuda")
    moved = 2 * B * (K - 1) * FRAME_BYTES  # read + written per launch

    def fs(t):
        lib.framestack_step(slab[:, t + 1], slab[:, t], K, None, term, term)

    def cp(t):
        lib.copy_rows(slab[:, t + 1, :(K - 1) * FRAME[0]], slab[:, t, FRAME[0]:])

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(args.reps):
            for t in range(T):  # walks the whole 0.95 GB slab: the columns do not stay in the caches
                fn(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (args.reps * T)
    for fn in (fs, cp):
        window(fn)
    res = dict(framestack=[], copy_rows=[])
    for _ in range(args.windows):  # alternate: both see the same machine
        res["framestack"].append(window(fs))
        res["copy_rows"].append(window(cp))
    out = dict(leg="kernel", rows=B, k=K, frame_bytes=FRAME_BYTES, bytes_read_plus_written_per_launch=moved,
               launches_per_window=args.reps * T, windows=args.windows)
    for name, ms in res.items():
        med = sorted(ms)[len(ms) // 2]
        out[name] = dict(us_per_launch_median=round(med * 1e3, 2), us_per_launch_min=round(min(ms) * 1e3, 2),
                         us_per_launch_max=round(max(ms) * 1e3, 2), tb_per_s_median=round(moved / (med * 1e-3) / 1e12, 3))
    out["framestack_over_copy_rows_time"] = round(out["framestack"]["us_per_launch_median"] /
                                                  out["copy_rows"]["us_per_launch_median"], 3)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--legs", default="A,B,kernel")
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--env_workers", type=int, default=4)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--timeout", type=int, default=400)
    p.add_argument("--label", default="this tree")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "framestack_bench.json"))
    args = p.parse_args()
    if args.child:
        kernel(args) if args.child == "kernel" else leg(args, args.child)
        return
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    results = []
    for which in args.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [
            f"--{k}={getattr(args, k)}" for k in ("steps", "warmup", "env_workers", "reps", "windows")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        results.append(json.loads(line[-1]) if line and r.returncode == 0 else dict(leg=which, rc=r.returncode, err=r.stderr[-800:]))
        print(json.dumps(results[-1]), flush=True)
        if r.returncode != 0:
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(source_sha16=build.source_sha16(), tree=args.label, workload=f"{B} agents, Nature CNN, rollout {T}, "
                       f"async APPO, {args.env_workers} env worker processes x 2 instances", steps=args.steps,
                       warmup=args.warmup, results=results), f, indent=1)


if __name__ == "__main__":
    main()
