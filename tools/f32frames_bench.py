"""Time the Nature CNN (convnet_atari, relu, fc 512, Discrete(6)) on float32 4x84x84 frames with normalize_input=True (the
reference's default) on three paths, each in a child process of its own on the same GPU:

 * native:      conv1 reads the f32 frames in place and normalises them in its loader (sf_conv_fwd_norm / _wgrad_norm);
 * materialise: SF_CONV1_NORM=0 — the normalised f32 NHWC batch is written (sf_obsnorm_apply), then conv1 reads it;
 * torch:       SF_NATIVE_F32FRAMES=0 — the network under torch autograd (model/torch_policy.py).

  python tools/f32frames_bench.py [--n 4096] [--train_e 4096] [--train_t 32] [--minibatches 4]

Per path: one rollout inference step at n samples, and one Learner.train over E x T samples (minibatches, 1 epoch), timed
with HIP events after warm-up; achieved TFLOP/s from the model's arithmetic (forward MACs per sample below, backward 2x the
forward).  For per-kernel time run a child under `rocprofv3 --kernel-trace --stats -- python tools/f32frames_bench.py
--child native ...`."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# per sample: conv1 400 x 256 x 32, conv2 81 x 512 x 64, conv3 49 x 576 x 64, fc 3136 x 512, heads 512 x 7 MACs
FWD_FLOP = 2 * (400 * 256 * 32 + 81 * 512 * 64 + 49 * 576 * 64 + 3136 * 512 + 512 * 7)
PATHS = {"native": dict(SF_CONV1_NORM="1", SF_NATIVE_F32FRAMES="1"),
         "materialise": dict(SF_CONV1_NORM="0", SF_NATIVE_F32FRAMES="1"),
         "torch": dict(SF_CONV1_NORM="1", SF_NATIVE_F32FRAMES="0")}


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.algo.utils.shared_buffers import alloc_trajectory_tensors
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    E, T, nb = args.train_e, args.train_t, args.minibatches
    import tempfile
    cfg = default_cfg(encoder_conv_architecture="convnet_atari", nonlinearity="relu", obs_scale=1.0, normalize_input=True,
                      encoder_conv_mlp_layers=[512], use_rnn=False, recurrence=1, rollout=T, batch_size=E * T // nb,
                      num_batches_per_epoch=nb, num_epochs=1, seed=0, serial_mode=True,
                      train_dir=tempfile.mkdtemp(prefix="sf_f32frames_bench_"), experiment="b")
    obs_space = spaces.Dict({"obs": spaces.Box(0, 1, (4, 84, 84), np.float32)})
    env_info = EnvInfo(obs_space, spaces.Discrete(6), E)
    pv = torch.zeros(1, dtype=torch.int32)
    learner = Learner(cfg, env_info, pv, 0, ParameterServer(0, pv))
    learner.init()
    ac = learner.actor_critic
    out = dict(path=args.child, model=type(ac).__name__, fused_norm=bool(getattr(ac, "_fused_norm", False)))
    # rollout step: one inference forward on n frames
    frames = torch.rand((args.n, 4, 84, 84), device="cuda")
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
    ms = ev[0].elapsed_time(ev[1]) / args.reps
    out["rollout_step_ms"] = round(ms, 3)
    out["rollout_tflops"] = round(args.n * FWD_FLOP / (ms * 1e-3) / 1e12, 2)
    # one Learner.train on E x T samples
    batch = alloc_trajectory_tensors(env_info, E, T, 1, "cuda")
    batch["obs"]["obs"].copy_(torch.rand(batch["obs"]["obs"].shape, device="cuda"))
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
    ms = sorted(times)[len(times) // 2]
    out["train_ms"] = round(ms, 1)
    out["train_tflops"] = round(E * T * FWD_FLOP * 3 / (ms * 1e-3) / 1e12, 2)  # forward + backward (2x the forward)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", default=None)
    p.add_argument("--n", type=int, default=4096)
    p.add_argument("--train_e", type=int, default=4096)
    p.add_argument("--train_t", type=int, default=32)
    p.add_argument("--minibatches", type=int, default=4)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--train_reps", type=int, default=2)
    p.add_argument("--timeout", type=int, default=240)
    args = p.parse_args()
    if args.child:
        child(args)
        return
    for path in PATHS:
        env = dict(os.environ, **PATHS[path])
        cmd = [sys.executable, os.path.abspath(__file__), "--child", path] + [
            f"--{k}={getattr(args, k)}" for k in ("n", "train_e", "train_t", "minibatches", "reps", "train_reps")]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
        line = [x for x in r.stdout.splitlines() if x.startswith("{")]
        print(line[-1] if line and r.returncode == 0 else json.dumps(dict(path=path, rc=r.returncode,
                                                                          err=r.stderr[-800:])), flush=True)
        if r.returncode != 0:
            break


if __name__ == "__main__":
    main()
