"""Learner.train on recurrent cores that used to fall to the per-step launches: width 1024 (csrc/sf_rnn_wideseq.h) and
chunk counts beyond one launch at 256 / 512 (row slabs, csrc/sf_rnn.hip) — the fused passes against the per-step launches
they replace, and against a build of the parent commit.

Model: synthetic_ant (obs f32[27], Box(8)), MLP encoder [64] tanh + GRU / LSTM core, one minibatch of Cn chunks per
dataset.  Cells (kind:H:Cn:R, --cells): {gru, lstm}-1024 at 64 / 512 / 2048 chunks with rollout = recurrence = 32;
{gru, lstm}-{256, 512} at 4096 / 8192 chunks with rollout = recurrence = 8.  What is timed is `Learner.train` on one collected
dataset: chunk setup, bootstrap forward, GAE, the SGD step (forward, loss, BPTT, Adam) — host clock around calls that end
in a device synchronise, no profiler.

Every (cell, path) runs in a fresh child process: one rollout + train as warm-up, `--warmup` more train calls, then
`--windows` windows of as many calls as fill `--window_s` seconds; the child reports the mean call time of each window.
The paths of this tree — SF_LSTM_SEQ=0 (per-step launches) and the default (fused passes) — alternate `--repeats` times;
`--parent_tree DIR` (a built checkout of the parent commit) is timed once per cell in between; `--variant_lib SO` (a build
with tools/experiments/sf_rnn_bwd_slab_regw_not_kept.patch and -DSF_SEQ_BWD_SLAB_REGW=1: 1024-row backward slabs on the
register-resident kernels, tools/build_variant.sh) is timed once per 256 / 512 cell as the second candidate slab height.
The fused children run with the offer FORCED (the `supported` queries replaced by what the entry points can run), so that a
cell the library does not offer is still measured on the fused kernels; a fused child whose model reports the per-step
family is an error.

Per cell the result holds every window of every child, the median per path, the spread (max - min over the windows of all
repeats, relative to the median) and `faster`: the fused median is below the per-step median by more than the larger of the
two spreads.  That flag is what the `supported` queries' offer rests on.  `--c5 STEPS` adds
`bench.py --workload c5` of this tree and of the parent tree to the same file (their launches are unchanged).

  python tools/wideseq_bench.py [--parent_tree DIR] [--variant_lib SO] [--out profiles/wideseq_bench.json] [--append]"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ",".join([f"{k}:1024:{c}:32" for k in ("gru", "lstm") for c in (64, 512, 2048)] +
                 [f"{k}:{h}:{c}:8" for k in ("gru", "lstm") for h in (256, 512) for c in (4096, 8192)])


def child(args) -> None:
    """one configuration on the package found in --tree; prints one JSON line"""
    sys.path.insert(0, args.tree)
    import torch
    if not torch.cuda.is_available():
        sys.exit("wideseq_bench: needs an MI355X; a CPU run gives no time")
    import sample_factory_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(sample_factory_amd.__file__))) == os.path.abspath(args.tree)
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_continuous_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_ant", make_synthetic_continuous_env)
    Cn, H, R = args.Cn, args.H, args.R
    if args.force_offer:  # measure the kernels whatever the library offers: the entry points run any Cn > 0 at these widths
        from sample_factory_amd import lib
        lib.lstm_seq_supported = lambda Cn_, H_: Cn_ > 0 and H_ in (256, 512)
        if hasattr(lib, "rnn_wideseq_supported"):
            lib.rnn_wideseq_supported = lambda kind_, Cn_, H_: kind_ in (0, 1) and Cn_ > 0 and H_ == 1024
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
    if args.force_offer:
        assert family != "per_step", "the fused child ran the per-step path"

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
    assert not ac.rnn_pass_aborted(), "a fused pass aborted: the times are not those of a complete pass"
    print("WIDESEQ " + json.dumps(dict(family=family, calls_per_window=calls, ms=[round(w, 4) for w in windows], loss=loss)), flush=True)


def run_child(tree, cell, seq, args, lib=None):
    kind, H, Cn, R = cell
    env = dict(os.environ, SF_LSTM_SEQ=seq)
    if lib:
        env["SF_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--kind", kind, "--H", str(H), "--Cn", str(Cn),
           "--R", str(R), "--warmup", str(args.warmup), "--windows", str(args.windows), "--window_s", str(args.window_s)]
    if seq == "1" and os.path.abspath(tree) == ROOT:
        cmd.append("--force_offer")
    out = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=args.child_timeout)
    if out.returncode != 0:  # (nothing more is started on the GPU after a child that failed)
        sys.exit(f"wideseq_bench: child failed ({out.returncode}): {' '.join(cmd[3:])}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    line = [l for l in out.stdout.splitlines() if l.startswith("WIDESEQ ")][-1]
    return json.loads(line[len("WIDESEQ "):])


def run_c5(tree, steps, timeout):
    cmd = [sys.executable, "bench.py", "--workload", "c5", "--gpus", "1", "--steps", str(steps), "--warmup", "3"]
    out = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        sys.exit(f"wideseq_bench: bench.py failed ({out.returncode}) in {tree}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return {k: res[k] for k in ("metric", "value", "unit", "steps", "ms_per_step") if k in res}


def median(x):
    s = sorted(x)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def summarise(runs):
    ms = [w for r in runs for w in r["ms"]]
    med = median(ms)
    return dict(median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), spread=round((max(ms) - min(ms)) / med, 4),
                family=runs[0]["family"], runs=runs)


def beats(a, b):
    """path b is faster than path a by more than the larger of the two spreads"""
    return bool(a["median_ms"] - b["median_ms"] > max(a["spread"] * a["median_ms"], b["spread"] * b["median_ms"]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--force_offer", action="store_true", help="child: replace the supported queries by what the entry points run")
    p.add_argument("--tree", default=ROOT)
    p.add_argument("--kind", default="gru")
    p.add_argument("--H", type=int, default=1024)
    p.add_argument("--Cn", type=int, default=512)
    p.add_argument("--R", type=int, default=32)
    p.add_argument("--cells", default=CELLS, help="kind:H:Cn:R, comma separated")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--windows", type=int, default=4)
    p.add_argument("--window_s", type=float, default=0.3)
    p.add_argument("--child_timeout", type=float, default=240.0)
    p.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit, timed once per cell")
    p.add_argument("--variant_lib", default=None, help="libsf_hip built with -DSF_SEQ_BWD_SLAB_REGW=1 (256 / 512 cells)")
    p.add_argument("--c5", type=int, default=0, metavar="STEPS", help="also run bench.py --workload c5 here and in --parent_tree")
    p.add_argument("--out", default=None)
    p.add_argument("--append", action="store_true", help="keep the cells --out already holds (a run split over several calls)")
    args = p.parse_args()
    if args.child:
        return child(args)
    doc = dict(results=[])
    if args.out and args.append and os.path.exists(args.out):
        doc = json.load(open(args.out))

    def save():
        if not args.out:
            return
        sys.path.insert(0, ROOT)
        from sample_factory_amd import build
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc.update(source_sha16=build.source_sha16(), repeats=args.repeats, windows=args.windows, window_s=args.window_s,
                   warmup=args.warmup)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    for spec in [c for c in args.cells.split(",") if c]:
        kind, H, Cn, R = spec.split(":")
        cell = (kind, int(H), int(Cn), int(R))
        variant = args.variant_lib if cell[1] != 1024 else None
        runs = dict(per_step=[], fused=[], parent=[], fused_bwd_slab_1024=[])
        for rep in range(args.repeats):
            runs["per_step"].append(run_child(ROOT, cell, "0", args))
            if rep == 0 and args.parent_tree:
                runs["parent"].append(run_child(os.path.abspath(args.parent_tree), cell, "1", args))
            runs["fused"].append(run_child(ROOT, cell, "1", args))
            if variant and rep == 0:
                runs["fused_bwd_slab_1024"].append(run_child(ROOT, cell, "1", args, lib=variant))
        res = dict(kind=kind, H=cell[1], Cn=cell[2], R=cell[3], samples=cell[2] * cell[3], **{k: summarise(v) for k, v in runs.items() if v})
        res["ratio"] = round(res["fused"]["median_ms"] / res["per_step"]["median_ms"], 4)
        res["faster"] = beats(res["per_step"], res["fused"])
        if variant:
            res["bwd_slab_1024_faster_than_default"] = beats(res["fused"], res["fused_bwd_slab_1024"])
        doc["results"] = [r for r in doc["results"] if (r["kind"], r["H"], r["Cn"], r["R"]) != cell] + [res]
        print(json.dumps({k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median_ms", "spread", "family")})
                          for k, v in res.items()}), flush=True)
        save()  # rewritten after every cell: a run that is cut short leaves what it measured
    if args.c5:
        doc["c5"] = dict(this_tree=run_c5(ROOT, args.c5, args.child_timeout))
        if args.parent_tree:
            doc["c5"]["parent"] = run_c5(os.path.abspath(args.parent_tree), args.c5, args.child_timeout)
        print(json.dumps(doc["c5"]), flush=True)
        save()


if __name__ == "__main__":
    main()
