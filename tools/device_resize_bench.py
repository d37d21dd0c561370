"""Raw frames resized and grey-scaled on the device (--device_resize / --device_grayscale) against the preprocessing a user
does in the env workers today, each leg in a child process of its own on the same GPU, the legs ALTERNATING (A, B, A, B, ...):

 * leg A: HostFrameVecEnv(hwc=True) frames [210, 160, 3] u8 behind a wrapper that preprocesses every frame inside the env
          worker with Pillow — Image.resize((84, 84), BOX) then convert("L") — and delivers [1, 84, 84]; flags off.  Pillow
          is a C-speed STAND-IN for OpenCV's INTER_AREA + COLOR_RGB2GRAY: it times the host work, its pixels are NOT
          bit-identical to the device's (float box filter, other luma rounding).  Skipped with a note where Pillow is absent;
 * leg B: the same env, raw, with --hwc_observations --device_resize 84 84 --device_grayscale=True: the native frame goes
          from the env workers' pages to the staging buffer untouched, sf_frame_resize writes the slab slot;
 * kernel: sf_frame_resize (area, grey) on 1024 such frames from a staging buffer into the last slot of a stacked slab
          column, HIP-event timed over back-to-back launches on buffers that do not fit the caches, beside sf_copy_rows
          moving the same source bytes from the same staging buffers, alternating; rates against the 8.0 TB/s HBM3E peak.

Both legs keep the 4-frame stack on the device (--device_framestack=4).  Workload: bench.py's c3 line — 1024 agents (4 env
worker processes x 2 instances x 128 agents, 2 sampling splits), Nature CNN, rollout 32 — once as async APPO (rollouts
overlap training: the pipeline's rate) and once synchronous (the rollout's own wall clock is exposed: `rollout_step_ms`).

  python tools/device_resize_bench.py [--legs A,B,kernel] [--rounds 2] [--steps 30] [--warmup 3] [--out profiles/device_resize_bench.json]

The stand-in env costs nothing but the preprocessing: leg A shows the host work at its most visible, leg B pays 14.3 x the
PCIe bytes per frame."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, K = 1024, 32, 4
NATIVE, OUT = (210, 160, 3), (84, 84)   # H, W, C as the env renders; OH, OW
NATIVE_BYTES, OUT_BYTES = NATIVE[0] * NATIVE[1] * NATIVE[2], OUT[0] * OUT[1]
HBM_PEAK_TBS = 8.0


def have_pillow() -> bool:
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


class HostPillowEnv:
    """what a user of a raw-pixel env does without the flags: every frame resized and grey-scaled on the host, in the env
    worker, with a C library"""

    def __init__(self, env):
        import numpy as np
        from PIL import Image

        sys.path.insert(0, ROOT)
        from sample_factory_amd.envs import spaces
        self.env, self.num_agents, self.action_space = env, env.num_agents, env.action_space
        self.observation_space = spaces.Dict({"obs": spaces.Box(0, 255, (1,) + OUT, np.uint8)})
        self._np, self._Image = np, Image
        self._out = np.empty((env.num_agents, 1) + OUT, np.uint8)

    def _small(self, o):
        Image, out = self._Image, self._out
        for i, frame in enumerate(o["obs"]):
            out[i, 0] = self._np.asarray(Image.fromarray(frame, "RGB").resize((OUT[1], OUT[0]), Image.BOX).convert("L"))
        return {"obs": out}

    def reset(self, **kwargs):
        o, info = self.env.reset(**kwargs)
        return self._small(o), info

    def step(self, actions):
        o, rew, te, tr, info = self.env.step(actions)
        return self._small(o), rew, te, tr, info

    def close(self):
        self.env.close()


def make_host_pillow_env(full_env_name, cfg=None, env_config=None, render_mode=None):
    sys.path.insert(0, ROOT)
    from sample_factory_amd.envs.synthetic import make_host_frame_env
    return HostPillowEnv(make_host_frame_env(full_env_name, cfg, env_config, render_mode))


def leg(args, which):
    sys.path.insert(0, ROOT)
    import tempfile

    import torch
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_host_frame_env
    from sample_factory_amd.train import make_runner
    register_env("host_raw", make_host_frame_env)
    register_env("host_raw_pillow_in_worker", make_host_pillow_env)
    W = args.env_workers
    flags = dict(hwc_observations=True, device_resize=list(OUT), device_grayscale=True) if which == "B" else {}
    cfg = default_cfg(
        env="host_raw" if which == "B" else "host_raw_pillow_in_worker", device_framestack=K,
        host_env_hwc=True, host_env_obs_shape=[NATIVE[2], NATIVE[0], NATIVE[1]],
        use_rnn=False, recurrence=1, encoder_conv_architecture="convnet_atari", nonlinearity="relu",
        encoder_conv_mlp_layers=[512], obs_scale=255.0, normalize_input=False, normalize_returns=False,
        exploration_loss_coeff=0.01, max_grad_norm=0.5, learning_rate=0.00025, adam_eps=1e-5,
        train_dir=tempfile.mkdtemp(prefix="sf_device_resize_bench_"), rollout=T, batch_size=B * T // 4, num_batches_per_epoch=4,
        num_epochs=4, async_rl=not args.sync_rl, serial_mode=False, batched_sampling=True, env_workers_mode="process",
        num_workers=W, num_envs_per_worker=2, worker_num_splits=2, synthetic_num_agents=B // (2 * W),
        env_gpu_observations=False, env_gpu_actions=False, seed=0, **flags)
    cfg, runner = make_runner(cfg)
    assert runner.init() == 0
    try:
        for _ in range(args.warmup):
            runner.iteration()
        for sm in runner.samplers:
            sm.ingest_prof, sm.h2d_bytes = {}, 0
        steps0, rounds0 = runner.learner.env_steps, runner.sampling_rounds
        rollout_s0 = float(runner.timing.get("rollout", 0.0))
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
        host = dict(act_wait_s=0.0, env_step_s=0.0, stage_s=0.0)
        for sm in runner.samplers:
            for k in host:
                host[k] += sm.ingest_prof.get(k, 0.0)
            sm.ingest_prof = None
        out = dict(leg=which, mode="sync" if args.sync_rl else "async", env_frames=list(runner.env.observation_space["obs"].shape),
                   slab_frames=list(runner.env_info.obs_space["obs"].shape),
                   device_resize=list(getattr(cfg, "device_resize", []) or []),
                   env_steps_per_s=round(env_steps_done / dt, 1), wall_s=round(dt, 3), sampling_rounds=rounds,
                   # wall clock per rollout step of all 1024 agents: async, rounds overlap training and this is the
                   # pipeline's period; sync, the host clock around the rollouts alone (every step ends in an event wait)
                   rollout_step_ms=round(1e3 * ((float(runner.timing.get("rollout", 0.0)) - rollout_s0) if args.sync_rl
                                                else dt) / (rounds * T), 4),
                   host_s_per_rollout_step_ms={k: round(1e3 * v / (rounds * T), 4) for k, v in host.items()},
                   h2d_bytes_per_env_step=round(sum(sm.h2d_bytes for sm in runner.samplers) / max(1, rounds * T * B), 1),
                   obs_dma_from_worker_pages_in_place=[sm._direct_ok.get("obs") for sm in runner.samplers])
        if which == "B":  # after the timed region: two more iterations with a HIP-event pair around every resize launch
            from sample_factory_amd import lib
            key = ("frame_resize", B // 2, NATIVE[0], NATIVE[1], NATIVE[2], 1, OUT[0], OUT[1], "area", 1)  # per split and step
            lib.PROFILE, lib.PROFILE_ONLY = {}, {key}
            for _ in range(2):
                runner.iteration()
            runner.stop_sampler_thread()
            torch.cuda.synchronize()
            prof, lib.PROFILE, lib.PROFILE_ONLY = lib.PROFILE, None, None
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in prof.get(key, []))
            out["frame_resize_launches_timed"] = len(ms)
            if ms:
                med = ms[len(ms) // 2]
                out["frame_resize_us_per_launch_median"] = round(med * 1e3, 2)
                out["frame_resize_us_per_rollout_step"] = round(2 * med * 1e3, 2)  # 2 splits
    finally:
        runner.close_envs()
    print(json.dumps(out), flush=True)


def kernel(args):
    """the new launch beside the library's plain byte mover on the same source bytes"""
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import lib
    H, W, C = NATIVE
    Tk = 8  # staging buffers: 8 x 1024 x 100800 = 0.83 GB, they do not stay in the caches
    stage = torch.randint(0, 256, (Tk, B, H, W, C), dtype=torch.uint8, device="cuda")
    slab = torch.zeros((B, Tk + 1, K, OUT[0], OUT[1]), dtype=torch.uint8, device="cuda")
    copy = torch.zeros((2, B, H, W, C), dtype=torch.uint8, device="cuda")
    fns = dict(
        frame_resize=(lambda t: lib.frame_resize(slab[:, t + 1, K - 1:], stage[t], True, "area", True),
                      B * (NATIVE_BYTES + OUT_BYTES)),
        frame_resize_nearest=(lambda t: lib.frame_resize(slab[:, t + 1, K - 1:], stage[t], True, "nearest", True),
                              B * (NATIVE_BYTES + OUT_BYTES)),
        copy_rows=(lambda t: lib.copy_rows(copy[t & 1], stage[t]), 2 * B * NATIVE_BYTES))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(args.reps):
            for t in range(Tk):
                fn(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (args.reps * Tk)
    for fn, _ in fns.values():
        window(fn)
    res = {name: [] for name in fns}
    for _ in range(args.windows):  # alternate: all see the same machine
        for name, (fn, _) in fns.items():
            res[name].append(window(fn))
    out = dict(leg="kernel", rows=B, k=K, frame=[H, W, C], out=list(OUT), frame_bytes=NATIVE_BYTES,
               launches_per_window=args.reps * Tk, windows=args.windows, hbm_peak_tb_per_s=HBM_PEAK_TBS)
    for name, ms in res.items():
        med, moved = sorted(ms)[len(ms) // 2], fns[name][1]
        out[name] = dict(bytes_read_plus_written_per_launch=moved, us_per_launch_median=round(med * 1e3, 2),
                         us_per_launch_min=round(min(ms) * 1e3, 2), us_per_launch_max=round(max(ms) * 1e3, 2),
                         tb_per_s_median=round(moved / (med * 1e-3) / 1e12, 3),
                         share_of_hbm_peak=round(moved / (med * 1e-3) / 1e12 / HBM_PEAK_TBS, 3))
    out["frame_resize_over_copy_rows_time"] = round(out["frame_resize"]["us_per_launch_median"] /
                                                    out["copy_rows"]["us_per_launch_median"], 3)
    out["frame_resize_nearest_over_copy_rows_time"] = round(out["frame_resize_nearest"]["us_per_launch_median"] /
                                                            out["copy_rows"]["us_per_launch_median"], 3)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--legs", default="A,B,kernel")
    p.add_argument("--rounds", type=int, default=2, help="how often the A, B pair is repeated (alternating)")
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--env_workers", type=int, default=4)
    p.add_argument("--modes", default="async,sync")
    p.add_argument("--sync_rl", action="store_true", help="(child) the synchronous mode of a leg")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--timeout", type=int, default=300)
    p.add_argument("--label", default="this tree")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_resize_bench.json"))
    args = p.parse_args()
    if args.child:
        kernel(args) if args.child == "kernel" else leg(args, args.child)
        return
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    legs, notes = args.legs.split(","), []
    if "A" in legs and not have_pillow():
        legs.remove("A")
        notes.append("leg A skipped: Pillow is not installed here, there is no host preprocessing to time against")
    order = [(w, m) for m in args.modes.split(",") for _ in range(args.rounds) for w in legs if w != "kernel"] + \
        [(w, "") for w in legs if w == "kernel"]
    results = []
    for which, mode in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + (["--sync_rl"] if mode == "sync" else []) + [
            f"--{k}={getattr(args, k)}" for k in ("steps", "warmup", "env_workers", "reps", "windows")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        results.append(json.loads(line[-1]) if line and r.returncode == 0 else dict(leg=which, rc=r.returncode, err=r.stderr[-800:]))
        print(json.dumps(results[-1]), flush=True)
        if r.returncode != 0:
            break
    summary = {}
    for mode in args.modes.split(","):
        sm = summary[mode] = {}
        for which in ("A", "B"):
            runs = [r for r in results if r.get("leg") == which and r.get("mode") == mode and "env_steps_per_s" in r]
            if runs:
                sm[which] = dict(env_steps_per_s=[r["env_steps_per_s"] for r in runs],
                                 rollout_step_ms=[r["rollout_step_ms"] for r in runs])
        if "A" in sm and "B" in sm:
            sm["B_over_A_mean_rate"] = round(sum(sm["B"]["env_steps_per_s"]) / len(sm["B"]["env_steps_per_s"]) /
                                             (sum(sm["A"]["env_steps_per_s"]) / len(sm["A"]["env_steps_per_s"])), 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(source_sha16=build.source_sha16(), tree=args.label,
                       workload=f"{B} agents, native frames {list(NATIVE)} u8 -> [1, {OUT[0]}, {OUT[1]}] grey, device_framestack "
                       f"{K}, Nature CNN, rollout {T}, {args.env_workers} env worker processes x 2 instances",
                       leg_A="Pillow resize(BOX) + convert('L') in the env workers: timing stand-in for OpenCV, not bit-identical "
                       "to the device arithmetic", leg_B="--hwc_observations --device_resize 84 84 --device_grayscale=True",
                       notes=notes, order=order, steps=args.steps, warmup=args.warmup, summary=summary, results=results),
                  f, indent=1)


if __name__ == "__main__":
    main()
