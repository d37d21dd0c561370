"""Time the resnet 3x3 conv family on bf16 MFMA (csrc/sf_resnet_bf16.hip) against the fp32-MFMA family, on an MI355X:

  python tools/resnet_bf16_bench.py [--n 32768] [--windows 5] [--reps 3] [--window_ms 200]

The three passes (sf_res_conv_fwd / _dgrad / _wgrad, _bf16 against _mfma) at the shapes of DESIGN.md 3.22's table that the
bf16 family serves, on the same N(0, 1) values.  Measurement as tools/resnet_wide_bench.py: device events around a window
of calls after a warm-up call of every contender, windows sized to `window_ms` of device work, the two contenders
ALTERNATE over `windows` windows, median and (min, max) per contender; TFLOP/s from 2 * 9 * Cin * Cout * n * H * W per pass.

`--c16` times the 16-channel layers of the width-1 tower instead (16 -> 16 and 16 -> 32 at 36 x 48 and 32 x 32, csrc/
sf_resnet_bf16_c16.hip) against the path they take with the flag off, the plain sf_res_conv_* entry points, and writes
profiles/resnet_bf16_c16_bench.json.

Writes profiles/resnet_bf16_bench.json.  Not in it yet: MIOpen fp32, torch autocast bf16 and Learner.train with the flag on
against off.  Every number is a measurement of the GPU it ran on; none is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 32, 32, 32), (32, 32, 16, 16), (32, 32, 8, 8), (32, 64, 32, 32), (64, 64, 32, 32), (64, 64, 16, 16),
          (64, 64, 8, 8), (64, 128, 32, 32), (128, 128, 16, 16), (128, 128, 8, 8)]
C16_SHAPES = [(16, 16, 36, 48), (16, 32, 36, 48), (16, 16, 32, 32), (16, 32, 32, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--c16", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    other = "plain" if args.c16 else "mfma_f32"
    args.out = args.out or os.path.join(ROOT, "profiles", "resnet_bf16_c16_bench.json" if args.c16 else "resnet_bf16_bench.json")
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
    import torch
    from resnet_wide_bench import _measure
    from sample_factory_amd import lib
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows, n = [], args.n
    for cin, cout, h, w in (C16_SHAPES if args.c16 else SHAPES):
        x, gy = torch.randn(n, h, w, cin, device="cuda"), torch.randn(n, h, w, cout, device="cuda")
        wt, b = torch.randn(9 * cin, cout, device="cuda") / (9 * cin) ** 0.5, torch.zeros(cout, device="cuda")
        out, gx, gw, gb = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(wt), torch.empty_like(b)
        d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=3, traj_T=0, sub_mean=0.0, inv_scale=1.0)
        ws = torch.empty(max(lib.res_conv_wgrad_bf16_workspace(n, d), lib.res_conv_wgrad_mfma_workspace(n, d),
                             lib.res_conv_wgrad_workspace(n, d)), dtype=torch.uint8, device="cuda")
        flop = 2.0 * 9 * cin * cout * n * h * w
        row = dict(cin=cin, cout=cout, h=h, w=w, n=n, act_in="elu", flop_per_pass=flop)
        fams = dict(bf16=(lib.res_conv_fwd_bf16, lib.res_conv_dgrad_bf16, lib.res_conv_wgrad_bf16),
                    **({"plain": (lib.res_conv_fwd, lib.res_conv_dgrad, lib.res_conv_wgrad)} if args.c16 else
                       {"mfma_f32": (lib.res_conv_fwd_mfma, lib.res_conv_dgrad_mfma, lib.res_conv_wgrad_mfma)}))
        row["fwd"] = _measure({k: (lambda f=f: f[0](x, h * w * cin, None, 0, wt, b, out, n, d)) for k, f in fams.items()},
                              flop, args, ev)
        row["dgrad"] = _measure({k: (lambda f=f: f[1](gy, wt, x, gx, n, d)) for k, f in fams.items()}, flop, args, ev)
        row["wgrad"] = _measure({k: (lambda f=f: f[2](x, h * w * cin, None, 0, gy, gw, gb, n, d, ws)) for k, f in fams.items()},
                                flop, args, ev)
        for p in ("fwd", "dgrad", "wgrad"):  # the share column of the shared helper is of the fp32 peak: meaningless here
            for c in row[p].values():
                c.pop("share_of_mfma_peak", None)
            row[p][other + "_over_bf16"] = round(row[p][other]["ms"] / row[p]["bf16"]["ms"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/resnet_bf16_bench.py", device=torch.cuda.get_device_name(0), windows=args.windows,
                           window_ms=args.window_ms, kernels=rows,
                           not_measured=["MIOpen fp32", "torch autocast bf16", "Learner.train flag on / off"]), f, indent=1)
        del x, gy, out, gx, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
