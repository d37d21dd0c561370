"""The two launches --track_inactive_agents puts in the place of their siblings, against those siblings on the same buffers:

 * sf_traj_write_env_step_active against sf_traj_write_env_step, B = 4096 rows, T = 32 (one launch per slab column);
 * sf_rnn_store_state_held against sf_rnn_store_state, B = 4096, H = 512, GRU and LSTM, on columns t -> t + 1 of a
   [B, T + 1, S] state slab, with no row and with a quarter of the rows recorded with policy_id = -1 (a held row reads
   its previous state on top of what the plain kernel moves).

HIP-event timed windows of back-to-back launches, replayed from launch programs as the rollout replays them, the two
kernels alternating window by window (both see the same machine).  For the kernels' own durations run it under
`rocprofv3 --kernel-trace --stats` (k_traj_write_env[_active], k_rnn_store_state[_held]; --kinds picks GRU or LSTM).

  python tools/inactive_agents_bench.py [--reps 20] [--windows 7] [--kinds gru,lstm] [--out profiles/inactive_agents_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, H = 4096, 32, 512


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--kinds", default="gru,lstm")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "inactive_agents_bench.json"))
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from sample_factory_amd import build, lib
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rew = torch.randn(B, device=dev, generator=g)
    term = torch.rand(B, device=dev, generator=g) < 0.02
    trunc = torch.rand(B, device=dev, generator=g) < 0.01
    active_in = torch.rand(B, device=dev, generator=g) < 0.75
    state = torch.ones(B, dtype=torch.uint8, device=dev)
    tr = dict(rewards=torch.zeros(B, T, device=dev), dones=torch.zeros(B, T, dtype=torch.bool, device=dev),
              time_outs=torch.zeros(B, T, dtype=torch.bool, device=dev),
              policy_id=torch.zeros(B, T, dtype=torch.int32, device=dev))
    ep_ret, ep_len = torch.zeros(B, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    ep_stats = torch.zeros(3, dtype=torch.float64, device=dev)

    def write_plain(t):
        lib.traj_write_env_step(rew, term, trunc, T, t, 1.0, 10.0, 0, tr["rewards"], tr["dones"], tr["time_outs"],
                                tr["policy_id"], ep_ret, ep_len, ep_stats)

    def write_active(t):
        lib.traj_write_env_step_active(rew, term, trunc, T, t, 1.0, 10.0, 0, tr["rewards"], tr["dones"], tr["time_outs"],
                                       tr["policy_id"], ep_ret, ep_len, ep_stats, active_in, state)

    def program(fn):
        """the T launches as a launch program: a replay costs one foreign call per launch, as in the rollout — through the
        wrappers the host needs longer per launch than either kernel runs and the window would time the host"""
        with lib.record_launches() as prog:
            for t in range(T):
                fn(t)
        assert prog.unsafe is None and len(prog.calls) == T
        return prog

    def window(prog):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            prog.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (args.reps * T)

    def compare(plain, new):
        plain, new = program(plain), program(new)
        for fn in (plain, new):
            window(fn)
        ms = dict(plain=[], new=[])
        for _ in range(args.windows):
            ms["plain"].append(window(plain))
            ms["new"].append(window(new))
        out = {}
        for name, v in ms.items():
            out[name] = dict(us_per_launch_median=round(sorted(v)[len(v) // 2] * 1e3, 2), us_per_launch_min=round(min(v) * 1e3, 2),
                             us_per_launch_max=round(max(v) * 1e3, 2))
        out["new_over_plain_time"] = round(out["new"]["us_per_launch_median"] / out["plain"]["us_per_launch_median"], 3)
        return out

    results = dict(traj_write_env_step=compare(write_plain, write_active))
    for kind, parts in (("gru", 1), ("lstm", 2)):
        if kind not in args.kinds.split(","):
            continue
        S = parts * H
        states = torch.randn(B, T + 1, S, device=dev, generator=g)
        h = torch.randn(B, H, device=dev, generator=g)
        c = torch.randn(B, H, device=dev, generator=g) if parts == 2 else None

        def store_plain(t):
            lib.rnn_store_state(h, c, tr["dones"][:, t], states[:, t + 1])

        def store_held(t):
            lib.rnn_store_state_held(h, c, tr["dones"][:, t], states[:, t], tr["policy_id"][:, t], states[:, t + 1])

        for held in (0.0, 0.25):
            tr["policy_id"].copy_(torch.where(torch.rand(B, T, device=dev, generator=g) < held, -1, 0))
            key = f"rnn_store_state_{kind}_held_{held:g}"
            results[key] = compare(store_plain, store_held)
            results[key]["bytes_written_per_launch"] = B * S * 4
    out = dict(source_sha16=build.source_sha16(), rows=B, T=T, H=H, launches_per_window=args.reps * T, windows=args.windows,
               results=results)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
