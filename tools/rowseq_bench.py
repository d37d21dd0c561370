"""Learner.train on small recurrent cores: the row-owned sequence passes (csrc/sf_rnn_rowseq.h) against the per-step
launches they replace, and against a build of the parent commit.

Model: synthetic_ant (obs f32[27], Box(8)), MLP encoder [64] tanh + GRU / LSTM of width H in --widths, rollout =
recurrence = 32, one minibatch of Cn chunks per dataset (Cn in --chunks: 64 / 512 / 2048 chunks = 2048 / 16384 / 65536
samples).  What is timed is `Learner.train` on one collected dataset: chunk setup, bootstrap forward, GAE, the SGD step
(forward, loss, BPTT, Adam) — host clock around calls that end in a device synchronise, no profiler.

Every (kind, H, Cn, path) runs in a fresh child process: one rollout + train as warm-up, `--warmup` more train calls,
then `--windows` windows of as many calls as fill `--window_s` seconds; the child reports the mean call time of each
window.  The two paths of this tree — SF_LSTM_SEQ=0 (per-step launches) and the default (row-owned passes) — alternate
`--repeats` times; `--parent_tree DIR` (a built checkout of the parent commit: its `sample_factory_amd/` with
libsf_hip.so) is timed once per configuration in between, to show that SF_LSTM_SEQ=0 on this tree is the parent's time.

Per configuration the result holds every window of every child, the median per path, the spread (max - min over the
windows of all repeats, relative to the median) and `faster`: the row-owned median is below the per-step median by more
than the larger of the two spreads.  That flag is what sf_rnn_rowseq_supported's offer rests on.

  python tools/rowseq_bench.py [--parent_tree DIR] [--out profiles/rowseq_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 32


def child(args) -> None:
    """one configuration on the package found in --tree; prints one JSON line"""
    sys.path.insert(0, args.tree)
    import torch
    if not torch.cuda.is_available():
        sys.exit("rowseq_bench: needs an MI355X; a CPU run gives no time")
    import sample_factory_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(sample_factory_amd.__file__))) == os.path.abspath(args.tree)
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_continuous_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_ant", make_synthetic_continuous_env)
    Cn, H = args.Cn, args.H
    cfg = default_cfg(env="synthetic_ant", use_rnn=True, rnn_type=args.kind, rnn_size=H, nonlinearity="tanh", normalize_input=True,
                      encoder_mlp_layers=[64], rollout=R, recurrence=R, batch_size=Cn * R, num_batches_per_epoch=1, num_epochs=1,
                      num_workers=1, num_envs_per_worker=1, async_rl=False, serial_mode=True, seed=3, synthetic_num_agents=Cn,
                      normalize_returns=False, learning_rate=1e-5, max_policy_lag=10 ** 8)
    cfg, runner = make_runner(cfg)
    runner.init()
    seen = []
    train_dataset = runner._train_dataset
    runner._train_dataset = lambda ds: (seen.append(ds), train_dataset(ds))[1]
    runner.iteration()  # one rollout, one trained dataset: every shape below has run once
    ds = seen[-1]
    ac = runner.learner.actor_critic
    family = (getattr(ac, "_rnn_saved", None) or {}).get("family") or ("fused" if ac._rnn_saved.get("fused") else "per_step")

    def call():
        stats = runner.learner.train(runner.traj[ds])
        assert stats is not None and "train" in stats, "the dataset was not trained on"
        return stats
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    calls = max(3, int(args.window_s / max(time.perf_counter() - t0, 1e-4)))
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            stats = call()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / calls * 1e3)
    loss = float(stats["train"]["loss"])
    assert loss == loss, "the loss is NaN"
    print("ROWSEQ " + json.dumps(dict(family=family, calls_per_window=calls, ms=[round(w, 4) for w in windows], loss=loss)), flush=True)


def run_child(tree, kind, H, Cn, seq, args):
    env = dict(os.environ, SF_LSTM_SEQ=seq)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--kind", kind, "--H", str(H), "--Cn", str(Cn),
           "--warmup", str(args.warmup), "--windows", str(args.windows), "--window_s", str(args.window_s)]
    out = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=args.child_timeout)
    if out.returncode != 0:
        sys.exit(f"rowseq_bench: child failed ({out.returncode}): {' '.join(cmd[3:])}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    line = [l for l in out.stdout.splitlines() if l.startswith("ROWSEQ ")][-1]
    return json.loads(line[len("ROWSEQ "):])


def median(x):
    s = sorted(x)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def summarise(runs):
    ms = [w for r in runs for w in r["ms"]]
    med = median(ms)
    return dict(median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), spread=round((max(ms) - min(ms)) / med, 4),
                family=runs[0]["family"], runs=runs)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--tree", default=ROOT)
    p.add_argument("--kind", default="gru")
    p.add_argument("--H", type=int, default=64)
    p.add_argument("--Cn", type=int, default=512)
    p.add_argument("--kinds", default="gru,lstm")
    p.add_argument("--widths", default="32,64,128")
    p.add_argument("--chunks", default="64,512,2048")
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--windows", type=int, default=4)
    p.add_argument("--window_s", type=float, default=0.3)
    p.add_argument("--child_timeout", type=float, default=240.0)
    p.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit, timed once per configuration")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.child:
        return child(args)
    results = []
    for kind in args.kinds.split(","):
        for H in (int(x) for x in args.widths.split(",")):
            for Cn in (int(x) for x in args.chunks.split(",")):
                runs = dict(per_step=[], row_owned=[], parent=[])
                for rep in range(args.repeats):
                    runs["per_step"].append(run_child(ROOT, kind, H, Cn, "0", args))
                    if rep == 0 and args.parent_tree:
                        runs["parent"].append(run_child(os.path.abspath(args.parent_tree), kind, H, Cn, "1", args))
                    runs["row_owned"].append(run_child(ROOT, kind, H, Cn, "1", args))
                res = dict(kind=kind, H=H, Cn=Cn, samples=Cn * R, **{k: summarise(v) for k, v in runs.items() if v})
                a, b = res["per_step"], res["row_owned"]
                res["ratio"] = round(b["median_ms"] / a["median_ms"], 4)
                res["faster"] = bool(a["median_ms"] - b["median_ms"] > max(a["spread"] * a["median_ms"], b["spread"] * b["median_ms"]))
                results.append(res)
                print(json.dumps({k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median_ms", "spread", "family")})
                                  for k, v in res.items()}), flush=True)
                if args.out:  # rewritten after every configuration: a run that is cut short leaves what it measured
                    sys.path.insert(0, ROOT)
                    from sample_factory_amd import build
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as f:
                        json.dump(dict(source_sha16=build.source_sha16(), recurrence=R, repeats=args.repeats, windows=args.windows,
                                       window_s=args.window_s, warmup=args.warmup, results=results), f, indent=1)


if __name__ == "__main__":
    main()
