"""Time the wave-per-row kernels for action spaces wider than 128 (csrc/sf_rl.hip: k_ppo_loss_wide, k_vtrace_ratio_wide,
k_sample_write_wide) next to torch-ROCm's own evaluation of the same quantities, on the same GPU and the same shapes.

Per width A in --widths (Discrete(A)):
 * sf_ppo_loss at n minibatch rows of the fused heads matrix [n, 1 + A] (entropy exploration, KL term, gradients),
   against torch: log_softmax of the new and the old logits, gather, entropy, KL, clipped surrogate, clipped value loss,
   backward to the logits and the values;
 * sf_vtrace at n rows, recurrence 32, against torch's log_softmax + gather + clamped ratio (the recursion itself is left
   out of the torch side: it does not depend on A);
 * sf_sample_write_step at B rows, against torch: softmax, multinomial, log_softmax, gather and the copy of the logits
   into the trajectory.
The two sides alternate inside one timed loop (HIP events around every call, after warm-up); the median is reported.

Two figures per shape: the native-to-torch time ratio, and `hbm_share`: the bytes the algorithm must move (4 n A each
for the parameters, the old parameters and the gradient of the loss; parameters only for V-trace; parameters + recorded
logits for the sampler) over the native time, as a share of the 8.0 TB/s HBM3E peak of an MI355X.  It is a share of
peak of the REQUIRED traffic, not a measured bandwidth.

  python tools/wide_heads_bench.py [--widths 256,1024,4096] [--n 32768] [--B 4096] [--out profiles/wide_heads_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # bytes / s (MI355X HBM3E specification)


def median(x):
    return sorted(x)[len(x) // 2]


def alternate(native, other, reps, warmup=3):
    """median milliseconds of native() and other(), called in turn"""
    import torch
    for _ in range(warmup):
        native()
        other()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record()
        native()
        e[1].record()
        other()
        e[2].record()
    torch.cuda.synchronize()
    return median([e[0].elapsed_time(e[1]) for e in ev]), median([e[1].elapsed_time(e[2]) for e in ev])


def bench_width(lib, A, n, B, reps):
    import torch
    g = torch.Generator(device="cuda").manual_seed(A)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)
    ld = (1 + A + 3) // 4 * 4
    heads = rnd(n, ld)
    old_params = heads[:, 1:1 + A].contiguous() + 0.3 * rnd(n, A)
    actions = torch.randint(0, A, (n, 1), device="cuda", generator=g).float()
    old_logp = torch.log_softmax(old_params, 1).gather(1, actions.long())[:, 0].contiguous()
    old_values, adv, targets = rnd(n), rnd(n) * 3 + 0.5, rnd(n)
    valids = torch.rand(n, device="cuda", generator=g) > 0.07
    rewards, dones = rnd(n), torch.rand(n, device="cuda", generator=g) < 0.1
    out = dict(A=A, n=n, B=B)

    # ---- PPO loss
    cfg = lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.5, value_loss_coeff=0.5, exploration_coeff=0.01, kl_coeff=0.2,
                          exploration_kind=1, action_kind=0, dense_adv=0)
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    grad = torch.zeros_like(heads)
    lib.moments(adv, valids, None, n, mom)

    def native_loss():
        lib.ppo_loss(heads[:, 1:], ld, heads[:, 0], ld, actions, old_logp, old_params, old_values, adv, targets, valids,
                     None, 0, n, A, cfg, mom, sums, grad[:, 1:], grad[:, 0])

    vmask = valids.float()
    nv = vmask.sum()
    advn = (adv - adv[valids].mean()) / adv[valids].std().clamp_min(1e-7)

    def torch_loss():
        h = heads.detach().requires_grad_(True)
        z, v = h[:, 1:1 + A], h[:, 0]
        lsm, lso = torch.log_softmax(z, 1), torch.log_softmax(old_params, 1)
        p = lsm.exp()
        lp = lsm.gather(1, actions.long())[:, 0]
        ent = -(p * lsm).sum(1)
        kl = (p * (lsm - lso)).sum(1)
        ratio = torch.exp(lp - old_logp).clamp(0.05, 20.0)
        policy = -torch.min(ratio * advn, ratio.clamp(1 / 1.1, 1.1) * advn)
        vclip = old_values + (v - old_values).clamp(-0.5, 0.5)
        value = torch.max((v - targets) ** 2, (vclip - targets) ** 2)
        loss = ((policy - 0.01 * ent + 0.2 * kl + 0.5 * value) * vmask).sum() / nv
        loss.backward()
        return h.grad

    t_nat, t_torch = alternate(native_loss, torch_loss, reps)
    # same quantity on both sides: the gradient of the logits
    g_t = torch_loss()
    native_loss()
    torch.cuda.synchronize()
    err = float((grad[:, 1:1 + A] - g_t[:, 1:1 + A]).abs().max() / g_t[:, 1:1 + A].abs().max())
    need = 3 * 4 * n * A
    out["ppo_loss"] = dict(native_ms=round(t_nat, 4), torch_ms=round(t_torch, 4), ratio=round(t_nat / t_torch, 4),
                           required_bytes=need, hbm_share=round(need / (t_nat * 1e-3) / HBM_PEAK, 4),
                           grad_max_rel_diff=err)

    # ---- V-trace
    vs, va = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    params = heads[:, 1:]

    def native_vtrace():
        lib.vtrace(params, ld, heads[:, 0], ld, actions, old_logp, rewards, dones, None, 0, n, A, 0, 32, 0.99, 1.0, 1.0, vs,
                   va)

    def torch_ratio():
        lp = torch.log_softmax(heads[:, 1:1 + A], 1).gather(1, actions.long())[:, 0]
        return torch.exp(lp - old_logp).clamp(0.05, 20.0)

    t_nat, t_torch = alternate(native_vtrace, torch_ratio, reps)
    need = 4 * n * A
    out["vtrace"] = dict(native_ms=round(t_nat, 4), torch_ms=round(t_torch, 4), ratio=round(t_nat / t_torch, 4),
                         required_bytes=need, hbm_share=round(need / (t_nat * 1e-3) / HBM_PEAK, 4))

    # ---- sampler
    T = 8
    hb = heads[:B]
    tr = dict(actions=torch.zeros(B, T, 1, device="cuda"), logits=torch.zeros(B, T, A, device="cuda"),
              logp=torch.zeros(B, T, device="cuda"), values=torch.zeros(B, T + 1, device="cuda"),
              ver=torch.zeros(B, T, device="cuda"))
    env_a = torch.zeros(B, dtype=torch.int32, device="cuda")

    def native_sample():
        lib.sample_write_step(hb[:, 1:], ld, hb[:, 0], ld, B, A, T, 3, 7, 11, 0, 1.0, False, tr["actions"], tr["logits"],
                              tr["logp"], tr["values"], tr["ver"], env_a)

    t2 = dict(logits=torch.zeros(B, T, A, device="cuda"), actions=torch.zeros(B, T, 1, device="cuda"),
              logp=torch.zeros(B, T, device="cuda"))

    def torch_sample():
        z = hb[:, 1:1 + A]
        a = torch.multinomial(torch.softmax(z, 1), 1)
        t2["logp"][:, 3] = torch.log_softmax(z, 1).gather(1, a)[:, 0]
        t2["actions"][:, 3] = a.float()
        t2["logits"][:, 3] = z

    t_nat, t_torch = alternate(native_sample, torch_sample, reps)
    need = 2 * 4 * B * A
    out["sample"] = dict(native_ms=round(t_nat, 4), torch_ms=round(t_torch, 4), ratio=round(t_nat / t_torch, 4),
                         required_bytes=need, hbm_share=round(need / (t_nat * 1e-3) / HBM_PEAK, 4))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--widths", default="256,1024,4096")
    p.add_argument("--n", type=int, default=32768)
    p.add_argument("--B", type=int, default=4096)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--out", default=None, help="write the collected result lines to this JSON file")
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("wide_heads_bench: needs an MI355X; a CPU run gives no time")
    from sample_factory_amd import build, lib
    lib.load()
    results = []
    for A in (int(x) for x in args.widths.split(",")):
        res = bench_width(lib, A, args.n, args.B, args.reps)
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(source_sha16=build.source_sha16(), hbm_peak_bytes_per_s=HBM_PEAK, reps=args.reps,
                           results=results), f, indent=1)


if __name__ == "__main__":
    main()
