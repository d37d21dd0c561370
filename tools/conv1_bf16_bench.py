"""Time the raw-frame conv layer on bf16 MFMA (csrc/sf_conv1_bf16.hip) against what a flag-off model launches for the same
layer, on an MI355X:

  python tools/conv1_bf16_bench.py [--n 4096 32768] [--windows 5] [--reps 3] [--window_ms 200] [--commit SHA]

Four layers: the Nature layer on u8 frames with the normaliser's tables, convnet_simple on 3 x 72 x 128 u8 frames without
tables, convnet_impala (16 channels) on 4 x 84 x 84 u8 frames with tables, and the Nature layer on f32 frames with tables;
forward and weight gradient each.  sf_conv1_fwd_bf16 / sf_conv1_wgrad_bf16 against sf_conv_fwd_norm / sf_conv_wgrad_norm
(with tables) or sf_conv_fwd / sf_conv_wgrad (without), whose sources this change does not touch.  Measurement as
tools/conv_bf16_bench.py: device events around a window of calls after a warm-up call of every contender, windows sized to
`window_ms` of device work, the contenders ALTERNATE over `windows` windows, median and (min, max) per contender.
hbm_floor_bytes is what the pass must move: the frames once plus the output (forward) or dout (weight gradient) once, fp32;
share_of_hbm_floor = hbm_floor_bytes / 8 TB/s over the median time.

Writes profiles/conv1_bf16_bench.json, stamped with the kernel sources' hash (and --commit).  Not in it: Learner.train and
a rollout step with the flag on against off.  Every number is a measurement of the GPU it ran on; none is asserted."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
# (name, Cin, H, W, Cout, u8 frames, tables)
LAYERS = [("atari_u8_norm", 4, 84, 84, 32, True, True), ("simple_72x128_u8", 3, 72, 128, 32, True, False),
          ("impala_u8_norm", 4, 84, 84, 16, True, True), ("atari_f32_norm", 4, 84, 84, 32, False, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1_bf16_bench.json"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
    import torch
    from resnet_wide_bench import _measure
    from sample_factory_amd import lib
    from sample_factory_amd.build import source_sha16
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for n in args.n:
        for name, cin, h, w, cout, u8, tabs in LAYERS:
            oh, ow, elems = (h - 8) // 4 + 1, (w - 8) // 4 + 1, cin * h * w
            d = lib.sf_conv_desc(Cin=cin, H=h, W=w, Cout=cout, KH=8, KW=8, stride=4, OH=oh, OW=ow, in_u8=1 if u8 else 2, relu=1,
                                 traj_T=0, sub_mean=0.0, inv_scale=1.0 / 255.0 if u8 else 1.0)
            x = torch.randint(0, 256, (n, elems), dtype=torch.uint8, device="cuda") if u8 else torch.rand(n, elems, device="cuda")
            mu = torch.rand(elems, device="cuda") * 0.4 + 0.3 if tabs else None
            rstd = torch.rand(elems, device="cuda") * 4.0 + 2.0 if tabs else None
            gy = torch.randn(n, oh, ow, cout, device="cuda")
            wt, b = torch.randn(64 * cin, cout, device="cuda") / (64 * cin) ** 0.5, torch.zeros(cout, device="cuda")
            out, gw, gb = torch.empty_like(gy), torch.empty_like(wt), torch.empty_like(b)
            ws16 = torch.empty(lib.conv1_wgrad_bf16_workspace(n, d), dtype=torch.uint8, device="cuda")
            ws32 = torch.empty(max(16, lib.conv_wgrad_workspace(n, d)), dtype=torch.uint8, device="cuda")
            if tabs:
                fwd32 = lambda: lib.conv_fwd_norm(x, elems, None, 0, mu, rstd, wt, b, out, n, d)  # noqa: E731
                wg32 = lambda: lib.conv_wgrad_norm(x, elems, None, 0, mu, rstd, gy, gw, gb, n, d, ws32)  # noqa: E731
            else:
                fwd32 = lambda: lib.conv_fwd_raw(x, elems, None, 0, wt, b, out, n, d)  # noqa: E731
                wg32 = lambda: lib.conv_wgrad_raw(x, elems, None, 0, gy, gw, gb, n, d, ws32)  # noqa: E731
            flop = 2.0 * 64 * cin * cout * n * oh * ow
            floor = float(n) * (elems * (1 if u8 else 4) + oh * ow * cout * 4)
            row = dict(layer=name, cin=cin, h=h, w=w, cout=cout, frames="u8" if u8 else "f32", tables=tabs, n=n,
                       flop_per_pass=flop, hbm_floor_bytes=floor,
                       fp32_entry="sf_conv_*_norm" if tabs else "sf_conv_fwd / sf_conv_wgrad")
            row["fwd"] = _measure(dict(bf16=lambda: lib.conv1_fwd_bf16(x, elems, None, 0, mu, rstd, wt, b, out, n, d), fp32=fwd32),
                                  flop, args, ev)
            row["wgrad"] = _measure(dict(bf16=lambda: lib.conv1_wgrad_bf16(x, elems, None, 0, mu, rstd, gy, gw, gb, n, d, ws16),
                                         fp32=wg32), flop, args, ev)
            for p in ("fwd", "wgrad"):
                for c in ("bf16", "fp32"):
                    row[p][c].pop("share_of_mfma_peak", None)  # (the shared helper's share is of the fp32 matrix peak)
                    row[p][c]["share_of_hbm_floor"] = round(floor / HBM_BYTES_PER_S * 1e3 / row[p][c]["ms"], 3)
                row[p]["fp32_over_bf16"] = round(row[p]["fp32"]["ms"] / row[p]["bf16"]["ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            with open(args.out, "w") as f:
                json.dump(dict(tool="tools/conv1_bf16_bench.py", device=torch.cuda.get_device_name(0), commit=args.commit,
                               source_sha16=source_sha16(), windows=args.windows, window_ms=args.window_ms,
                               hbm_bytes_per_s=HBM_BYTES_PER_S, kernels=rows,
                               not_measured=["Learner.train flag on / off", "rollout step flag on / off", "learning curves"]),
                          f, indent=1)
            del x, gy, out, ws16, ws32
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
