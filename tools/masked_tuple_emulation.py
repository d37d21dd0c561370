"""How many rows of tests/test_gpu_masked_tuple_heads.py can differ from the float64 first crossing for arithmetic reasons
alone: the masked Tuple sampler's float32 arithmetic restated in numpy (needs no GPU) on the test's own inputs, with the
Philox uniforms the kernel draws.  Per Discrete member, as k_sample_write_masked_tuple computes it: max and sequential
float32 sum of exp over z + (mask ? 0 : -1e9), p = exp((z - mx) - lse) * inv / tot on the allowed columns, a sequential
float32 CDF, the first k with u < cdf (else the last k with p > 0).  The wave-per-row kernel adds the same float32 terms
in another order (64-column scans plus a carry); its head lists are emulated in the sequential order too.

  python tools/masked_tuple_emulation.py        -> one line per head list and member: rows of 4096 that differ"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

f32 = np.float32


def emulate_member(z, m, u):
    """z f32 [B, n], m bool [B, n], u f64 [B] (24-bit uniforms, exact in f32) -> drawn actions [B]"""
    B, n = z.shape
    zp = (z + np.where(m, f32(0), f32(-1e9))).astype(f32)
    mx = zp.max(1)
    se = np.zeros(B, f32)
    for k in range(n):
        se = (se + np.exp((zp[:, k] - mx).astype(f32)).astype(f32)).astype(f32)
    lse = np.log(se).astype(f32)
    with np.errstate(over="ignore"):  # (an all-zero slice: mx = max - 1e9, e = inf on columns that are never added)
        e = np.exp(((z - mx[:, None]).astype(f32) - lse[:, None]).astype(f32)).astype(f32)
    psum = np.zeros(B, f32)
    for k in range(n):
        psum = (psum + np.where(m[:, k], e[:, k], f32(0))).astype(f32)
    all_zero = psum == 0
    inv = (f32(1) / (psum + f32(1e-13)).astype(f32)).astype(f32)
    tot = np.where(all_zero, f32(n) * f32(1e-6), (psum * inv).astype(f32)).astype(f32)
    uf = u.astype(f32)
    acc = np.zeros(B, f32)
    a = np.full(B, -1)
    last_pos = np.full(B, -1)
    for k in range(n):
        w = np.where(all_zero, f32(1e-6), np.where(m[:, k], (e[:, k] * inv).astype(f32), f32(0))).astype(f32)
        p = (w / tot).astype(f32)
        acc = (acc + p).astype(f32)
        last_pos = np.where(p > 0, k, last_pos)
        a = np.where((a < 0) & (uf < acc), k, a)
    return np.where(a < 0, np.where(last_pos >= 0, last_pos, n - 1), a)


def main():
    from test_gpu_action_heads import uniforms_discrete
    from test_gpu_masked_tuple_heads import B, HEAD_LISTS, make_case
    from test_masked_tuple_cpu import masked_tuple_ref, n_params
    worst = 0
    for hs in HEAD_LISTS:
        seed, step, row0 = 31 + len(hs), 12, 70001 + n_params(hs)  # test_masked_tuple_sampler_vs_float64's
        logits, _, mask, _ = make_case(hs)
        rows = np.arange(row0, row0 + B, dtype=np.uint32)
        ref = masked_tuple_ref(logits, mask, hs)
        off, counts = 0, []
        for h_i, h in enumerate(hs):
            if h < 0:
                off += -2 * h
                continue
            u = uniforms_discrete(seed, step, rows, head=h_i)
            a = emulate_member(logits[:, off:off + h], mask[:, off:off + h] != 0, u)
            p = ref[h_i][0]
            want = np.minimum((np.cumsum(p, 1) <= u[:, None]).sum(1), h - 1)
            assert np.all(ref[h_i][2][np.arange(B), a]), "the emulation drew a masked-out action"
            counts.append(int((a != want).sum()))
            off += h
        worst = max(worst, max(counts))
        print(f"{hs}: rows of {B} that differ from the float64 first crossing, per Discrete member: {counts}")
    print(f"largest count: {worst} (the test's cap is {int(5e-3 * B)})")


if __name__ == "__main__":
    main()
