"""Time the resnet 3x3 conv family on fp32 MFMA (csrc/sf_resnet_mfma.hip) and the wide towers, on an MI355X:

  python tools/resnet_wide_bench.py [--n 32768] [--windows 5] [--reps 3] [--window_ms 200] [--train_e 256] [--train_t 32] [--parent DIR]
                                    [--widths 1,2,4] [--skip_first_layer] [--skip_kernels] [--skip_train]

1. Kernels: the inner 3x3 layers of the tower at 3 x 64 x 64 frames, n samples, width k = 1, 2, 4: sf_res_conv_fwd_mfma /
   _dgrad_mfma / _wgrad_mfma against torch (MIOpen) conv2d forward / input gradient / weight gradient on the same values
   (NCHW, torch's layout of choice), and at the (16,16), (16,32), (32,32) shapes also against the fp32 FMA entry points.
   Device events around a window of calls, after a warm-up call of every contender; a window holds as many calls as fill
   `window_ms` of device work (at least `reps`); the contenders of a shape ALTERNATE over `windows` windows; median and
   (min, max) per contender.  FLOP/s from the shapes (2 * 9 * Cin * Cout * n * H * W per pass) and the share of the
   157.3 TFLOP/s fp32-MFMA peak.  The raw u8 frames' layer (FMA kernels, 16k output channels) is timed against torch too.
2. Learner.train at k = 2 and 4, native against SF_NATIVE_RESNET=0, and at k = 1 against the tree given by --parent (a
   checkout of the parent commit with its library built; without it that column says "not measured"); each in a child
   process, alternating, `windows` windows.

Writes profiles/resnet_wide_bench.json, merging into what earlier runs left there (MIOpen searches its algorithms at
every new shape, minutes each, so a run can be split by --widths).  Every number is a measurement of the GPU it ran on; none is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TFLOPS = 157.3  # fp32 MFMA, MI355X


def layers(k):
    """(Cin, Cout, H, W) of the f32 3x3 layers of a 64 x 64 tower at width k: stage convs 2 and 3, the residual convs"""
    c = (16 * k, 32 * k, 32 * k)
    return [(c[0], c[0], 32, 32), (c[0], c[1], 32, 32), (c[1], c[1], 16, 16), (c[2], c[2], 8, 8)]


def _time(fn, reps, ev):
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _stats(ts, flop):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return dict(ms=round(med, 4), ms_min=round(ts[0], 4), ms_max=round(ts[-1], 4), tflops=round(flop / med / 1e9, 2),
                share_of_mfma_peak=round(flop / med / 1e9 / PEAK_TFLOPS, 3))


def _measure(cont, flop, args, ev):
    """warm every contender up, size each one's calls per window to --window_ms of device work (at least --reps), then
    alternate the contenders over --windows windows"""
    import torch
    for fn in cont.values():
        fn()
    torch.cuda.synchronize()
    reps = {c: max(args.reps, min(2000, int(args.window_ms / max(_time(fn, 2, ev), 1e-3)) + 1)) for c, fn in cont.items()}
    ts = {c: [] for c in cont}
    for _ in range(args.windows):
        for c, fn in cont.items():
            ts[c].append(_time(fn, reps[c], ev))
    return {c: dict(_stats(t, flop), calls_per_window=reps[c]) for c, t in ts.items()}


def first_layers(args):
    """the raw u8 frames' layer (3 x 64 x 64 -> 16k channels) on the FMA kernels, forward and weight gradient, against
    torch conv2d on the same frames as f32 NCHW (torch is handed the conversion for free)"""
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from sample_factory_amd import lib
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    n, cin, h, w = args.n, 3, 64, 64
    x = torch.randint(0, 256, (n, cin, h, w), dtype=torch.uint8, device="cuda")
    xt = x.float() / 255.0
    for k in args.widths:
        cout = 16 * k
        gy = torch.randn(n, h, w, cout, device="cuda")
        gyt = gy.permute(0, 3, 1, 2).contiguous()
        wt = torch.randn(9 * cin, cout, device="cuda") / (9 * cin) ** 0.5
        wtt = wt.view(3, 3, cin, cout).permute(3, 2, 0, 1).contiguous()
        b, out = torch.zeros(cout, device="cuda"), torch.empty_like(gy)
        gw, gb = torch.empty_like(wt), torch.empty_like(b)
        d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=1, act_in=0, traj_T=0, sub_mean=0.0, inv_scale=1.0 / 255.0)
        ws = torch.empty(lib.res_conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
        flop = 2.0 * 9 * cin * cout * n * h * w
        row = dict(cin=cin, cout=cout, h=h, w=w, n=n, flop_per_pass=flop)
        row["fwd"] = _measure(dict(fma=lambda: lib.res_conv_fwd(x, cin * h * w, None, 0, wt, b, out, n, d),
                                   torch=lambda: F.conv2d(xt, wtt, b, padding=1)), flop, args, ev)
        row["wgrad"] = _measure(dict(fma=lambda: lib.res_conv_wgrad(x, cin * h * w, None, 0, gy, gw, gb, n, d, ws),
                                     torch=lambda: torch.nn.grad.conv2d_weight(xt, wtt.shape, gyt, padding=1)), flop, args, ev)
        rows.append(row)
        print(json.dumps(row), flush=True)
        save(args, first_layer=rows)
        del gy, gyt, out, ws
        torch.cuda.empty_cache()
    return rows


def kernels(args):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from sample_factory_amd import lib
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows, seen = [], set()
    for k in args.widths:
        for cin, cout, h, w in layers(k):
            if (cin, cout, h, w) in seen:
                continue
            seen.add((cin, cout, h, w))
            n = args.n
            x = torch.randn(n, h, w, cin, device="cuda")
            gy = torch.randn(n, h, w, cout, device="cuda")
            wt = torch.randn(9 * cin, cout, device="cuda") / (9 * cin) ** 0.5
            b = torch.zeros(cout, device="cuda")
            out, gx = torch.empty_like(gy), torch.empty_like(x)
            gw, gb = torch.empty_like(wt), torch.empty_like(b)
            d = lib.sf_res_desc(Cin=cin, H=h, W=w, Cout=cout, in_u8=0, act_in=0, traj_T=0, sub_mean=0.0, inv_scale=1.0)
            ws = torch.empty(max(lib.res_conv_wgrad_mfma_workspace(n, d), lib.res_conv_wgrad_workspace(n, d)),
                             dtype=torch.uint8, device="cuda")
            xt, gyt = x.permute(0, 3, 1, 2).contiguous(), gy.permute(0, 3, 1, 2).contiguous()
            wtt = wt.view(3, 3, cin, cout).permute(3, 2, 0, 1).contiguous()
            passes = {
                "fwd": dict(mfma=lambda: lib.res_conv_fwd_mfma(x, h * w * cin, None, 0, wt, b, out, n, d),
                            fma=lambda: lib.res_conv_fwd(x, h * w * cin, None, 0, wt, b, out, n, d),
                            torch=lambda: F.conv2d(xt, wtt, b, padding=1)),
                "dgrad": dict(mfma=lambda: lib.res_conv_dgrad_mfma(gy, wt, None, gx, n, d),
                              fma=lambda: lib.res_conv_dgrad(gy, wt, None, gx, n, d),
                              torch=lambda: torch.nn.grad.conv2d_input(xt.shape, wtt, gyt, padding=1)),
                "wgrad": dict(mfma=lambda: lib.res_conv_wgrad_mfma(x, h * w * cin, None, 0, gy, gw, gb, n, d, ws),
                              fma=lambda: lib.res_conv_wgrad(x, h * w * cin, None, 0, gy, gw, gb, n, d, ws),
                              torch=lambda: torch.nn.grad.conv2d_weight(xt, wtt.shape, gyt, padding=1)),
            }
            flop = 2.0 * 9 * cin * cout * n * h * w
            row = dict(cin=cin, cout=cout, h=h, w=w, n=n, flop_per_pass=flop)
            for name, cont in passes.items():
                if cin > 32 or cout > 32:  # the plain entry points route these to the same MFMA kernels
                    cont.pop("fma")
                row[name] = _measure(cont, flop, args, ev)
            rows.append(row)
            print(json.dumps(row), flush=True)
            save(args, kernels=rows)  # MIOpen's search makes a shape take minutes: keep what is measured
            del x, gy, out, gx, xt, gyt, ws
            torch.cuda.empty_cache()
    return rows


def save(args, **parts):
    """merge into the result file: kernel rows by shape, anything else replaced"""
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    res["peak_fp32_mfma_tflops"] = PEAK_TFLOPS
    for part in parts:  # how each part of the file was measured: parts can come from different runs
        res.setdefault("settings", {})[part] = dict(windows=args.windows, window_ms=args.window_ms, min_calls_per_window=args.reps)
    key = lambda r: (r["cin"], r["cout"], r["h"], r["w"], r["n"])
    if "kernels" in parts:
        rows = {key(r): r for r in res.get("kernels", [])}
        rows.update({key(r): r for r in parts.pop("kernels")})
        res["kernels"] = [rows[k] for k in sorted(rows)]
    res.update(parts)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def train_child(args):
    root = args.tree or ROOT
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from sample_factory_amd.algo.learning.learner import Learner, ParameterServer
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.algo.utils.shared_buffers import alloc_trajectory_tensors
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    E, T, nb = args.train_e, args.train_t, 4
    kw = dict(encoder_resnet_width=args.width) if args.width != 1 else {}
    cfg = default_cfg(encoder_conv_architecture="resnet_impala", nonlinearity="elu", obs_scale=255.0, normalize_input=False,
                      use_rnn=False, recurrence=1, rollout=T, batch_size=E * T // nb, num_batches_per_epoch=nb, num_epochs=1,
                      seed=0, serial_mode=True, train_dir="/tmp/sf_resnet_wide_bench", experiment="b", **kw)
    env_info = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (3, 64, 64), np.uint8)}), spaces.Discrete(15), E)
    pv = torch.zeros(1, dtype=torch.int32)
    learner = Learner(cfg, env_info, pv, 0, ParameterServer(0, pv))
    learner.init()
    batch = alloc_trajectory_tensors(env_info, E, T, 1, "cuda")
    batch["obs"]["obs"].copy_(torch.randint(0, 256, batch["obs"]["obs"].shape, dtype=torch.uint8))
    batch["actions"].copy_(torch.randint(0, 15, batch["actions"].shape).float())
    batch["log_prob_actions"].fill_(-2.7)
    batch["rewards"].copy_(torch.randn(batch["rewards"].shape))
    for k in ("dones", "policy_id", "policy_version"):
        batch[k].zero_()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(args.reps + 1):  # the first call is the warm-up
        learner.train_step = 0
        t = _time(lambda: learner.train(batch), 1, ev)
        if i:
            times.append(t)
    print(json.dumps(dict(model=type(learner.actor_critic).__name__, train_ms=sorted(times)[len(times) // 2])), flush=True)


def trains(args):
    def run(width, native, tree):
        env = dict(os.environ, SF_NATIVE_RESNET="1" if native else "0")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", f"--width={width}", f"--reps={args.reps}",
               f"--train_e={args.train_e}", f"--train_t={args.train_t}"] + ([f"--tree={tree}"] if tree else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise RuntimeError(f"train child width={width} native={native}: rc {r.returncode}\n{r.stderr[-800:]}")
        return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])

    out = []
    for width in [w for w in (2, 4, 1) if w in args.widths]:
        if width == 1 and not args.parent:
            out.append(dict(width=1, a="this tree", b="parent commit", ratio="not measured (no --parent tree given)"))
            continue
        pair = dict(a=(True, None), b=(True, args.parent) if width == 1 else (False, None))
        ts, model = {c: [] for c in pair}, {}
        for _ in range(args.windows):
            for c, (native, tree) in pair.items():
                res = run(width, native, tree)
                ts[c].append(res["train_ms"])
                model[c] = res["model"]
        med = {c: sorted(t)[len(t) // 2] for c, t in ts.items()}
        row = dict(width=width, samples=args.train_e * args.train_t, a="native", b="parent commit" if width == 1 else "SF_NATIVE_RESNET=0",
                   model=model, train_ms={c: dict(median=round(med[c], 2), min=round(min(t), 2), max=round(max(t), 2)) for c, t in ts.items()},
                   ratio_b_over_a=round(med["b"] / med["a"], 3))
        out.append(row)
        print(json.dumps(row), flush=True)
        save(args, learner_train=out)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--width", type=int, default=1)
    p.add_argument("--tree", default=None)
    p.add_argument("--parent", default=None)
    p.add_argument("--n", type=int, default=32768)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--window_ms", type=float, default=200.0)
    p.add_argument("--train_e", type=int, default=256)
    p.add_argument("--train_t", type=int, default=32)
    p.add_argument("--timeout", type=int, default=300)
    p.add_argument("--skip_train", action="store_true")
    p.add_argument("--skip_kernels", action="store_true")
    p.add_argument("--skip_first_layer", action="store_true")
    p.add_argument("--widths", type=lambda s: [int(x) for x in s.split(",")], default=[1, 2, 4])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_wide_bench.json"))
    args = p.parse_args()
    if args.child:
        train_child(args)
        return
    if not args.skip_first_layer:
        first_layers(args)
    if not args.skip_kernels:
        kernels(args)
    if not args.skip_train:
        save(args, learner_train=trains(args))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
