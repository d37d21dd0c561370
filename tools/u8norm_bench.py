"""Time u8 image models with normalize_input=True (the reference's default) on two paths, each in a child process of its own
on the same GPU:

 * fused:       the first conv reads the u8 frames in place and normalises them in its loader (sf_conv_fwd_norm /
                sf_res_conv_fwd_norm and their weight gradients);
 * materialise: SF_CONV1_NORM=0 — the normalised f32 NHWC batch is written (sf_obsnorm_apply), then the first conv reads it.

Cases: (a) convnet_simple on 3x72x128 with fc 512, (b) convnet_impala on 4x84x84, (c) resnet_impala on 3x72x96 (all elu,
Discrete(6)).  Per case and path: one rollout inference step at n samples and one Learner.train over E x T samples in
`minibatches` minibatches (1024 x 32 for the resnet, as tools/resnet_bench.py), timed with HIP events after warm-up, and
torch.cuda.max_memory_allocated() of the child.  The loop stops at the first child that fails; each child runs under its
own time limit.

  python tools/u8norm_bench.py [--cases a,b,c] [--n 4096] [--out profiles/u8norm_bench.json]

For per-kernel time run a child under `rocprofv3 --kernel-trace --stats -- python tools/u8norm_bench.py --child fused
--case a`."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {  # name: (architecture, frame shape, fc layers, training envs)
    "a": ("convnet_simple", (3, 72, 128), [512], 4096),
    "b": ("convnet_impala", (4, 84, 84), [512], 4096),
    "c": ("resnet_impala", (3, 72, 96), [512], 1024),
}
PATHS = {"fused": "1", "materialise": "0"}


def child(args):
    sys.path.insert(0, ROOT)
    import tempfile
    import numpy as np
    import torch
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.algo.utils.shared_buffers import alloc_trajectory_tensors
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    arch, shape, fc, E = CASES[args.case]
    T, nb = args.train_t, args.minibatches
    cfg = default_cfg(encoder_conv_architecture=arch, nonlinearity="elu", obs_scale=255.0, normalize_input=True,
                      encoder_conv_mlp_layers=fc, use_rnn=False, recurrence=1, rollout=T, batch_size=E * T // nb,
                      num_batches_per_epoch=nb, num_epochs=1, seed=0, serial_mode=True,
                      train_dir=tempfile.mkdtemp(prefix="sf_u8norm_bench_"), experiment="b")
    obs_space = spaces.Dict({"obs": spaces.Box(0, 255, shape, np.uint8)})
    env_info = EnvInfo(obs_space, spaces.Discrete(6), E)
    pv = torch.zeros(1, dtype=torch.int32)
    learner = Learner(cfg, env_info, pv, 0, ParameterServer(0, pv))
    learner.init()
    ac = learner.actor_critic
    tower = ac.encoders["obs"] if hasattr(ac, "encoders") else ac
    out = dict(case=args.case, arch=arch, shape=list(shape), path=args.child, model=type(ac).__name__,
               fused_norm=bool(getattr(tower, "_fused_norm", False)), n=args.n, train_samples=E * T, minibatches=nb)
    frames = torch.randint(0, 256, (args.n,) + shape, dtype=torch.uint8, device="cuda")
    ac.obs_normalizer.update(frames, ac.obs_elems, args.n)  # statistics of the frames: a realistic share of clamped pixels
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.no_grad():
        for _ in range(3):
            ac.forward({"obs": frames})
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(args.reps):
            ac.forward({"obs": frames})
        ev[1].record()
        torch.cuda.synchronize()
    out["rollout_step_ms"] = round(ev[0].elapsed_time(ev[1]) / args.reps, 4)
    out["rollout_max_mem_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    batch = alloc_trajectory_tensors(env_info, E, T, 1, "cuda")
    for e0 in range(0, E, 256):  # (filled in slices: the host staging copy stays small)
        part = batch["obs"]["obs"][e0:e0 + 256]
        part.copy_(torch.randint(0, 256, part.shape, dtype=torch.uint8, device="cuda"))
    batch["actions"].copy_(torch.randint(0, 6, batch["actions"].shape).float())
    batch["log_prob_actions"].fill_(-1.79)
    batch["rewards"].copy_(torch.randn(batch["rewards"].shape))
    batch["dones"].zero_()
    batch["policy_id"].zero_()
    batch["policy_version"].zero_()
    times = []
    for i in range(args.train_reps + 1):
        learner.train_step = 0
        ev[0].record()
        learner.train(batch)
        ev[1].record()
        torch.cuda.synchronize()
        if i:  # the first call is the warm-up
            times.append(ev[0].elapsed_time(ev[1]))
    out["train_ms"] = round(sorted(times)[len(times) // 2], 2)
    out["train_ms_all"] = [round(t, 2) for t in times]
    out["max_mem_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--case", default="a")
    p.add_argument("--cases", default="a,b,c")
    p.add_argument("--paths", default="fused,materialise")
    p.add_argument("--n", type=int, default=4096)
    p.add_argument("--train_t", type=int, default=32)
    p.add_argument("--minibatches", type=int, default=4)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--train_reps", type=int, default=3)
    p.add_argument("--timeout", type=int, default=240)
    p.add_argument("--out", default=None, help="write the collected result lines to this JSON file")
    args = p.parse_args()
    if args.child:
        child(args)
        return
    results, ok = [], True
    for case in args.cases.split(","):
        for path in args.paths.split(","):
            env = dict(os.environ, SF_CONV1_NORM=PATHS[path])
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--case", case] + [
                f"--{k}={getattr(args, k)}" for k in ("n", "train_t", "minibatches", "reps", "train_reps")]
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
                rc, so, se = r.returncode, r.stdout, r.stderr
            except subprocess.TimeoutExpired as e:
                rc, so, se = 124, "", f"time limit of {args.timeout} s: {e}"
            line = [x for x in so.splitlines() if x.startswith("{")]
            res = json.loads(line[-1]) if line and rc == 0 else dict(case=case, path=path, rc=rc, err=se[-800:])
            results.append(res)
            print(json.dumps(res), flush=True)
            if rc != 0:  # nothing more is started on the GPU after a child that failed
                ok = False
                break
        if not ok:
            break
    if args.out:
        sys.path.insert(0, ROOT)
        from sample_factory_amd import build
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(source_sha16=build.source_sha16(), results=results), f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
