"""Launch times of the PPO loss (forward + backward in one launch) under an action mask next to the unmasked loss, on the
protocol of tools/masked_tuple_bench.py: 32768 rows read through a shuffled index, HIP events around every call of the
Python binding, median of --reps launches after a warm-up.

  sf_ppo_loss / sf_ppo_loss_heads   [6] (k_ppo_loss<8>), [5] * 8 (k_ppo_loss_md), [21] * 8 and [300] (k_ppo_loss_wide)
  sf_ppo_loss_masked                the same lists under a random half-allowed mask that keeps the taken action, read from
                                    a [E, T + 1, A] slab in place (k_masked_ppo_loss_md for the first two,
                                    k_masked_ppo_loss_wide for the others)

A call is the memset of the eight sums plus the loss kernel; entropy exploration and the KL term are on, so the old
logits are read too.  Each run is one process; --out appends the run to a JSON list, so three runs give three entries:

  python tools/masked_loss_bench.py [--reps 30] [--out profiles/masked_loss_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, T = 32768, 32
HEAD_LISTS = ([6], [5] * 8, [21] * 8, [300])


def time_launch(fn, reps, warmup=10):
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("masked_loss_bench: needs an MI355X; a CPU run gives no time")
    from sample_factory_amd import lib
    lib.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    n, N = N_ROWS, 2 * N_ROWS
    E = N // T
    res = {}
    for hs in HEAD_LISTS:
        A, H = sum(hs), len(hs)
        ld = (1 + A + 3) // 4 * 4
        heads = torch.randn((n, ld), device="cuda", generator=g) * 1.5
        g_heads = torch.zeros((n, ld), device="cuda")
        old_params = torch.randn((N, A), device="cuda", generator=g)
        actions = torch.stack([torch.randint(0, h, (N,), device="cuda", generator=g) for h in hs], 1).float().contiguous()
        offs = torch.tensor([sum(hs[:i]) for i in range(H)], device="cuda")
        flat = (torch.rand((N, A), device="cuda", generator=g) < 0.5).to(torch.uint8)
        flat.scatter_(1, actions.long() + offs, 1)  # the taken action is allowed
        mask = torch.ones((E, T + 1, A), dtype=torch.uint8, device="cuda")
        mask[:, :T] = flat.view(E, T, A)
        old_logp = torch.randn(N, device="cuda", generator=g) * 0.1 - 2.0
        old_values = torch.randn((E, T + 1), device="cuda", generator=g)
        adv, tgt = torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)
        valids = torch.rand(N, device="cuda", generator=g) > 0.05
        index = torch.randperm(N, device="cuda", generator=g)[:n].to(torch.int32)
        cfg = lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.5, value_loss_coeff=0.5, exploration_coeff=0.01, kl_coeff=0.2,
                              exploration_kind=1, action_kind=0, dense_adv=0, old_values_T=T)
        if 1 < H <= 8:
            cfg.num_heads = H
            for i, h in enumerate(hs):
                cfg.head_n[i] = h
        mom = torch.zeros(3, dtype=torch.float64, device="cuda")
        sums = torch.zeros(8, dtype=torch.float64, device="cuda")
        ratio = torch.zeros(n, device="cuda")
        lib.moments(adv, valids, index, n, mom)

        def loss(**kw):
            lib.ppo_loss(heads[:, 1:], ld, heads[:, 0], ld, actions, old_logp, old_params, old_values, adv, tgt, valids,
                         index, 0, n, A, cfg, mom, sums, g_heads[:, 1:], g_heads[:, 0], ratio_out=ratio,
                         head_sizes=hs if H > 1 else None, **kw)

        name = f"{hs[0]}x{H}"
        res[f"loss_{name}_us"] = time_launch(loss, args.reps)
        res[f"loss_masked_{name}_us"] = time_launch(lambda: loss(mask=mask, mask_T=T), args.reps)
        assert torch.isfinite(g_heads).all() and torch.isfinite(sums).all()
    out = dict(lib=os.path.basename(lib.LIB_PATH), rows=n, reps=args.reps, median_us=res)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        runs = json.load(open(args.out)) if os.path.exists(args.out) else []
        runs.append(out)
        with open(args.out, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
