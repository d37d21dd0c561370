"""Time the loss, V-trace and sampler kernels of csrc/sf_rl.hip on Tuple action spaces of MANY members next to
torch-ROCm's own evaluation of the same quantities, on the same GPU and the same shapes: the protocol of
tools/wide_heads_bench.py (both sides alternate inside one timed loop, HIP events around every call, median of --reps).

Per list `m x H` in --lists (H Discrete(m) members; 21x8 is the anchor the struct of sf_ppo_loss already held):
 * the PPO loss at n minibatch rows of the fused heads matrix [n, 1 + A] (entropy exploration, KL term, gradients) —
   sf_ppo_loss up to 8 members, sf_ppo_loss_heads above — against torch: log_softmax over the [n, H, m] view of the new
   and the old logits, gather, entropy, KL, clipped surrogate, clipped value loss, backward to the logits and values;
 * sf_vtrace at n rows, recurrence 32, against torch's log_softmax + gather + sum + clamped ratio;
 * sf_sample_write_step_tuple at B rows, against torch: softmax, multinomial per member, log_softmax, gather, sum and
   the copy of the logits into the trajectory.
Per cell: the native-to-torch time ratio and `ps_per_param`, the native time over n * A (B * A) in picoseconds, which
puts a 17- or 24-member list next to the eight-member anchor.

  python tools/many_heads_bench.py [--lists 21x8,5x17,11x17,21x24] [--n 32768] [--B 4096] [--out FILE.json]
(SF_HIP_LIB=... times another build of the same sources, e.g. one of tools/build_variant.sh)"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from wide_heads_bench import alternate  # noqa: E402


def bench_list(lib, m, H, n, B, reps):
    import torch
    heads_list = [m] * H
    A = m * H
    g = torch.Generator(device="cuda").manual_seed(A + H)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)
    ld = (1 + A + 3) // 4 * 4
    heads = rnd(n, ld)
    old_params = heads[:, 1:1 + A].contiguous() + 0.3 * rnd(n, A)
    actions = torch.randint(0, m, (n, H), device="cuda", generator=g).float()
    ai = actions.long().unsqueeze(-1)
    old_logp = torch.log_softmax(old_params.view(n, H, m), -1).gather(-1, ai).squeeze(-1).sum(1).contiguous()
    old_values, adv, targets = rnd(n), rnd(n) * 3 + 0.5, rnd(n)
    valids = torch.rand(n, device="cuda", generator=g) > 0.07
    rewards, dones = rnd(n), torch.rand(n, device="cuda", generator=g) < 0.1
    out = dict(list=f"{m}x{H}", A=A, n=n, B=B)
    cell = lambda t_nat, t_torch, rows: dict(native_ms=round(t_nat, 4), torch_ms=round(t_torch, 4),
                                             ratio=round(t_nat / t_torch, 4),
                                             ps_per_param=round(t_nat * 1e9 / (rows * A), 3))

    # ---- PPO loss
    cfg = lib.sf_loss_cfg(clip_ratio=0.1, clip_value=0.5, value_loss_coeff=0.5, exploration_coeff=0.01, kl_coeff=0.2,
                          exploration_kind=1, action_kind=0, dense_adv=0)
    if H <= len(cfg.head_n):
        cfg.num_heads = H
        for i in range(H):
            cfg.head_n[i] = m
    mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    grad = torch.zeros_like(heads)
    lib.moments(adv, valids, None, n, mom)

    def native_loss():
        lib.ppo_loss(heads[:, 1:], ld, heads[:, 0], ld, actions, old_logp, old_params, old_values, adv, targets, valids,
                     None, 0, n, A, cfg, mom, sums, grad[:, 1:], grad[:, 0], head_sizes=heads_list)

    vmask = valids.float()
    nv = vmask.sum()
    advn = (adv - adv[valids].mean()) / adv[valids].std().clamp_min(1e-7)

    def torch_loss():
        h = heads.detach().requires_grad_(True)
        z, v = h[:, 1:1 + A].reshape(n, H, m), h[:, 0]
        lsm, lso = torch.log_softmax(z, -1), torch.log_softmax(old_params.view(n, H, m), -1)
        p = lsm.exp()
        lp = lsm.gather(-1, ai).squeeze(-1).sum(1)
        ent = -(p * lsm).sum((1, 2))
        kl = (p * (lsm - lso)).sum((1, 2))
        ratio = torch.exp(lp - old_logp).clamp(0.05, 20.0)
        policy = -torch.min(ratio * advn, ratio.clamp(1 / 1.1, 1.1) * advn)
        vclip = old_values + (v - old_values).clamp(-0.5, 0.5)
        value = torch.max((v - targets) ** 2, (vclip - targets) ** 2)
        loss = ((policy - 0.01 * ent + 0.2 * kl + 0.5 * value) * vmask).sum() / nv
        loss.backward()
        return h.grad

    t_nat, t_torch = alternate(native_loss, torch_loss, reps)
    g_t = torch_loss()
    native_loss()
    torch.cuda.synchronize()
    out["ppo_loss"] = cell(t_nat, t_torch, n)
    out["ppo_loss"]["grad_max_rel_diff"] = float((grad[:, 1:1 + A] - g_t[:, 1:1 + A]).abs().max() / g_t[:, 1:1 + A].abs().max())

    # ---- V-trace
    vs, va = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")

    def native_vtrace():
        lib.vtrace(heads[:, 1:], ld, heads[:, 0], ld, actions, old_logp, rewards, dones, None, 0, n, A, 0, 32, 0.99, 1.0,
                   1.0, vs, va, head_sizes=heads_list)

    def torch_ratio():
        lp = torch.log_softmax(heads[:, 1:1 + A].reshape(n, H, m), -1).gather(-1, ai).squeeze(-1).sum(1)
        return torch.exp(lp - old_logp).clamp(0.05, 20.0)

    out["vtrace"] = cell(*alternate(native_vtrace, torch_ratio, reps), n)

    # ---- sampler
    T = 8
    hb = heads[:B]
    tr = dict(actions=torch.zeros(B, T, H, device="cuda"), logits=torch.zeros(B, T, A, device="cuda"),
              logp=torch.zeros(B, T, device="cuda"), values=torch.zeros(B, T + 1, device="cuda"),
              ver=torch.zeros(B, T, device="cuda"))
    env_a = torch.zeros((B, H), dtype=torch.int32, device="cuda")

    def native_sample():
        lib.sample_write_step_tuple(hb[:, 1:], ld, hb[:, 0], ld, B, heads_list, T, 3, 7, 11, 0, 1.0, False, tr["actions"],
                                    tr["logits"], tr["logp"], tr["values"], tr["ver"], env_a)

    t2 = dict(logits=torch.zeros(B, T, A, device="cuda"), actions=torch.zeros(B, T, H, device="cuda"),
              logp=torch.zeros(B, T, device="cuda"))

    def torch_sample():
        z = hb[:, 1:1 + A]
        zz = z.reshape(B * H, m)
        a = torch.multinomial(torch.softmax(zz, 1), 1)
        t2["logp"][:, 3] = torch.log_softmax(zz, 1).gather(1, a).view(B, H).sum(1)
        t2["actions"][:, 3] = a.view(B, H).float()
        t2["logits"][:, 3] = z

    out["sample"] = cell(*alternate(native_sample, torch_sample, reps), B)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lists", default="21x8,5x17,11x17,21x24", help="comma-separated m x H: H Discrete(m) members")
    p.add_argument("--n", type=int, default=32768)
    p.add_argument("--B", type=int, default=4096)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--out", default=None, help="write the collected result lines to this JSON file")
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("many_heads_bench: needs an MI355X; a CPU run gives no time")
    from sample_factory_amd import build, lib
    lib.load()
    results = []
    for spec in args.lists.split(","):
        m, H = (int(x) for x in spec.split("x"))
        res = bench_list(lib, m, H, args.n, args.B, args.reps)
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(source_sha16=build.source_sha16(), lib=lib.LIB_PATH, reps=args.reps, results=results), f, indent=1)


if __name__ == "__main__":
    main()
