"""Time the fully connected layers on bf16 MFMA (csrc/sf_linear_bf16.hip) against the fp32 kernels a flag-off model launches
for the same layer, on an MI355X:

  python tools/linear_bf16_bench.py [--n 4096 32768] [--windows 5] [--reps 3] [--window_ms 200] [--commit SHA]

(K, N) in {(3136, 512), (512, 512), (256, 256), (64, 64)}, the three passes each, ReLU, on the same N(0, 1) values:
sf_linear_fwd_bf16 against sf_conv_fwd_t where it takes the launch (else sf_conv_fwd), sf_linear_dgrad_bf16 against
sf_conv_dgrad, sf_linear_wgrad_bf16 against sf_conv_wgrad, the fp32 side on the layer's sf_conv_desc (H = W = KH = KW = 1) as
the model calls it.  Measurement as tools/resnet_wide_bench.py: device events around a window of calls after a warm-up call
of every contender, windows sized to `window_ms` of device work, the contenders ALTERNATE over `windows` windows, median
and (min, max) per contender; TFLOP/s from 2 * n * K * N per pass.

Writes profiles/linear_bf16_bench.json, stamped with the kernel sources' hash (and --commit).  Not in it: Learner.train
with the flag on against off.  Every number is a measurement of the GPU it ran on; none is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [(3136, 512), (512, 512), (256, 256), (64, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_bf16_bench.json"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
    import torch
    from resnet_wide_bench import _measure
    from sample_factory_amd import lib
    from sample_factory_amd.build import source_sha16
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for n in args.n:
        for K, N in LAYERS:
            d = lib.sf_conv_desc(Cin=K, H=1, W=1, Cout=N, KH=1, KW=1, stride=1, OH=1, OW=1, in_u8=0, relu=1, traj_T=0,
                                 sub_mean=0.0, inv_scale=1.0)
            x, gy = torch.randn(n, K, device="cuda"), torch.randn(n, N, device="cuda")
            w, b = torch.randn(K, N, device="cuda") / K ** 0.5, torch.zeros(N, device="cuda")
            wt = w.t().contiguous()  # the [N, K] copy sf_conv_fwd_t reads
            out, gx, gw, gb = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
            ws16 = torch.empty(lib.linear_wgrad_bf16_workspace(n, K, N), dtype=torch.uint8, device="cuda")
            fwd_t = bool(lib.conv_fwd_t_supported(n, d))  # the model's choice (ActorCritic._gemm), split-K workspace included
            fws = lib.conv_fwd_t_workspace(n, d) if fwd_t else lib.conv_fwd_workspace(n, d)
            ws32 = torch.empty(max(16, lib.conv_wgrad_workspace(n, d), fws), dtype=torch.uint8, device="cuda")
            fwd32 = (lambda: lib.conv_fwd_t(x, K, wt, b, out, n, d, ws32 if fws else None)) if fwd_t else \
                (lambda: lib.conv_fwd_raw(x, K, None, 0, w, b, out, n, d, ws32 if fws else None))
            flop = 2.0 * n * K * N
            row = dict(K=K, N=N, n=n, act="relu", flop_per_pass=flop, fp32_fwd="sf_conv_fwd_t" if fwd_t else "sf_conv_fwd",
                       wgrad_parts=ws16.numel() // (4 * (K * N + N)))
            row["fwd"] = _measure(dict(bf16=lambda: lib.linear_fwd_bf16(x, w, b, out, n, K, N, 1), fp32=fwd32), flop, args, ev)
            row["dgrad"] = _measure(dict(bf16=lambda: lib.linear_dgrad_bf16(gy, w, x, gx, n, K, N, 1),
                                         fp32=lambda: lib.conv_dgrad(gy, w, x, gx, n, d)), flop, args, ev)
            row["wgrad"] = _measure(dict(bf16=lambda: lib.linear_wgrad_bf16(x, gy, gw, gb, n, K, N, ws16),
                                         fp32=lambda: lib.conv_wgrad_raw(x, K, None, 0, gy, gw, gb, n, d, ws32)), flop, args, ev)
            for p in ("fwd", "dgrad", "wgrad"):
                row[p]["bf16"].pop("share_of_mfma_peak", None)  # (the shared helper's share is of the fp32 peak)
                row[p]["fp32_over_bf16"] = round(row[p]["fp32"]["ms"] / row[p]["bf16"]["ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            with open(args.out, "w") as f:
                json.dump(dict(tool="tools/linear_bf16_bench.py", device=torch.cuda.get_device_name(0), commit=args.commit,
                               source_sha16=source_sha16(), windows=args.windows, window_ms=args.window_ms, kernels=rows,
                               not_measured=["Learner.train flag on / off"]), f, indent=1)
            del x, gy, out, gx, ws16, ws32
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
