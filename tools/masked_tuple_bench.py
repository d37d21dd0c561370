"""Launch times of the action samplers around the masked Tuple sampler, 4096 rows, HIP events around every launch as in
tools/many_heads_bench.py (median of --reps launches after a warm-up):

  sf_sample_write_step_tuple         [21] * 8 (168 parameters: one wave per row) and [5] * 8 (40: one lane per row)
  sf_sample_write_step_masked        Discrete(6) (one lane per row) and Discrete(300) (one wave per row)
  sf_sample_write_step_tuple_masked  the two head lists above under a random half-allowed mask (skipped where the loaded
                                     library has no such entry point: SF_HIP_LIB=... times another build of the sources)

Two figures per launch.  `median_us`: HIP events around every single call of the Python binding, as above; for a kernel
shorter than the binding's own host time (~20 us) this is the host's time to issue a launch, not the kernel's.
`burst_us`: the launch recorded once as a launch program and replayed --burst times back to back between ONE pair of
events, over --burst: the host issues a replayed launch in a few microseconds, so this is the GPU's time per launch.

  python tools/masked_tuple_bench.py [--reps 400] [--burst 2000] [--out FILE.json]
Run it several times per build, alternating builds, and compare a build's medians with the spread of the other's runs:
these launches take a few microseconds and nothing else says what their run-to-run spread is."""
from __future__ import annotations

import argparse
import json
import os
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 4096, 8


def time_launch(fn, reps, warmup=20):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return round(median(s.elapsed_time(e) for s, e in ev) * 1e3, 3)  # microseconds


def time_burst(lib, fn, burst, rounds=5):
    """GPU microseconds per launch: fn recorded as a launch program, replayed `burst` times between one pair of events"""
    import torch
    fn()
    with lib.record_launches() as prog:
        fn()
    assert len(prog.calls) == 1 and prog.unsafe is None
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(burst):
            prog.replay()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / burst)
    return round(median(out), 3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=400)
    p.add_argument("--burst", type=int, default=2000)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("masked_tuple_bench: needs an MI355X; a CPU run gives no time")
    from sample_factory_amd import lib
    L = lib.load()
    g = torch.Generator(device="cuda").manual_seed(3)
    res, burst = {}, {}

    def both(key, fn):
        res[key] = time_launch(fn, args.reps)
        burst[key] = time_burst(lib, fn, args.burst)

    def slab(nact, A):
        z = lambda *s: torch.zeros(s, device="cuda")
        return z(B, T, nact), z(B, T, A), z(B, T), z(B, T + 1), z(B, T)

    for hs in ([21] * 8, [5] * 8):
        A, H = sum(hs), len(hs)
        ld = (1 + A + 3) // 4 * 4
        heads = torch.randn((B, ld), device="cuda", generator=g) * 3
        mask = (torch.rand((B, T + 1, A), device="cuda", generator=g) < 0.5).to(torch.uint8)
        mask[:, :, ::hs[0]] = 1  # every member keeps its first action
        mk = mask[:, 3]
        tr = slab(H, A)
        env_a = torch.zeros((B, H), dtype=torch.int32, device="cuda")
        name = f"{hs[0]}x{H}"
        both(f"tuple_{name}_us",
             lambda: lib.sample_write_step_tuple(heads[:, 1:], ld, heads[:, 0], ld, B, hs, T, 3, 7, 11, 0, 1.0, False, *tr,
                                                 env_a))
        if hasattr(L, "sf_sample_write_step_tuple_masked"):
            both(f"tuple_masked_{name}_us",
                 lambda: lib.sample_write_step_tuple_masked(heads[:, 1:], ld, heads[:, 0], ld, mk, mk.stride(0), B, hs, T, 3,
                                                            7, 11, 0, 1.0, False, *tr, env_a))
    for A in (6, 300):
        ld = (1 + A + 3) // 4 * 4
        heads = torch.randn((B, ld), device="cuda", generator=g) * 3
        mask = (torch.rand((B, T + 1, A), device="cuda", generator=g) < 0.5).to(torch.uint8)
        mask[:, :, 0] = 1
        mk = mask[:, 3]
        tr = slab(1, A)
        env_a = torch.zeros(B, dtype=torch.int32, device="cuda")
        both(f"masked_{A}_us",
             lambda: lib.sample_write_step_masked(heads[:, 1:], ld, heads[:, 0], ld, mk, mk.stride(0), B, A, T, 3, 7, 11, 0,
                                                  1.0, False, *tr, env_a))
    out = dict(lib=os.path.basename(lib.LIB_PATH), rows=B, reps=args.reps, burst=args.burst, median_us=res,
               burst_us=burst)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
