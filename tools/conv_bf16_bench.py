"""Time the inner convs of convnet_simple / convnet_atari on bf16 MFMA (csrc/sf_conv_bf16.hip) against the fp32 kernels a
flag-off model launches for the same layer, on an MI355X:

  python tools/conv_bf16_bench.py [--n 4096 32768] [--windows 5] [--reps 3] [--window_ms 200] [--commit SHA]

The three layers at the 84 x 84 geometries (conv2 32 -> 64 4x4/2 on 20 x 20; convnet_atari conv3 64 -> 64 3x3/1 on 9 x 9;
convnet_simple conv3 64 -> 128 3x3/2 on 9 x 9), the three passes each, on the same N(0, 1) values: sf_conv_fwd_bf16 against
sf_conv_fwd_t where it takes the launch (else sf_conv_fwd), sf_conv_dgrad_bf16 against sf_conv_dgrad, sf_conv_wgrad_bf16
against sf_conv_wgrad.  Measurement as tools/resnet_wide_bench.py: device events around a window of calls after a warm-up
call of every contender, windows sized to `window_ms` of device work, the contenders ALTERNATE over `windows` windows,
median and (min, max) per contender; TFLOP/s from 2 * K*K * Cin * Cout * n * OH * OW per pass.

Writes profiles/conv_bf16_bench.json, stamped with the kernel sources' hash (and --commit).  Not in it: Learner.train and a
rollout step with the flag on against off.  Every number is a measurement of the GPU it ran on; none is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [("conv2", 32, 64, 4, 2, 20, 20), ("conv3_atari", 64, 64, 3, 1, 9, 9), ("conv3_simple", 64, 128, 3, 2, 9, 9)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_bf16_bench.json"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
    import torch
    from resnet_wide_bench import _measure
    from sample_factory_amd import lib
    from sample_factory_amd.build import source_sha16
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for n in args.n:
        for name, cin, cout, k, s, h, w in LAYERS:
            oh, ow = (h - k) // s + 1, (w - k) // s + 1
            d = lib.sf_conv_desc(Cin=cin, H=h, W=w, Cout=cout, KH=k, KW=k, stride=s, OH=oh, OW=ow, in_u8=0, relu=1, traj_T=0,
                                 sub_mean=0.0, inv_scale=1.0)
            x, gy = torch.randn(n, h, w, cin, device="cuda"), torch.randn(n, oh, ow, cout, device="cuda")
            wt, b = torch.randn(k * k * cin, cout, device="cuda") / (k * k * cin) ** 0.5, torch.zeros(cout, device="cuda")
            wtt = wt.t().contiguous()  # the [Cout, K] copy sf_conv_fwd_t reads
            out, gx, gw, gb = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(wt), torch.empty_like(b)
            ws16 = torch.empty(lib.conv_wgrad_bf16_workspace(n, d), dtype=torch.uint8, device="cuda")
            ws32 = torch.empty(max(16, lib.conv_wgrad_workspace(n, d)), dtype=torch.uint8, device="cuda")
            stride = h * w * cin
            fwd_t = lib.conv_fwd_t_supported(n, d) and not lib.conv_fwd_t_workspace(n, d)
            fwd32 = (lambda: lib.conv_fwd_t(x, stride, wtt, b, out, n, d)) if fwd_t else \
                (lambda: lib.conv_fwd_raw(x, stride, None, 0, wt, b, out, n, d))
            flop = 2.0 * k * k * cin * cout * n * oh * ow
            row = dict(layer=name, cin=cin, cout=cout, kernel=k, stride=s, h=h, w=w, n=n, act="relu", flop_per_pass=flop,
                       fp32_fwd="sf_conv_fwd_t" if fwd_t else "sf_conv_fwd")
            row["fwd"] = _measure(dict(bf16=lambda: lib.conv_fwd_bf16(x, stride, None, 0, wt, b, out, n, d), fp32=fwd32),
                                  flop, args, ev)
            row["dgrad"] = _measure(dict(bf16=lambda: lib.conv_dgrad_bf16(gy, wt, x, gx, n, d),
                                         fp32=lambda: lib.conv_dgrad(gy, wt, x, gx, n, d)), flop, args, ev)
            row["wgrad"] = _measure(dict(bf16=lambda: lib.conv_wgrad_bf16(x, stride, None, 0, gy, gw, gb, n, d, ws16),
                                         fp32=lambda: lib.conv_wgrad_raw(x, stride, None, 0, gy, gw, gb, n, d, ws32)),
                                    flop, args, ev)
            for p in ("fwd", "dgrad", "wgrad"):
                row[p]["bf16"].pop("share_of_mfma_peak", None)  # (the shared helper's share is of the fp32 peak)
                row[p]["fp32_over_bf16"] = round(row[p]["fp32"]["ms"] / row[p]["bf16"]["ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            with open(args.out, "w") as f:
                json.dump(dict(tool="tools/conv_bf16_bench.py", device=torch.cuda.get_device_name(0), commit=args.commit,
                               source_sha16=source_sha16(), windows=args.windows, window_ms=args.window_ms, kernels=rows,
                               not_measured=["Learner.train flag on / off", "rollout step flag on / off"]), f, indent=1)
            del x, gy, out, gx, ws16, ws32
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
