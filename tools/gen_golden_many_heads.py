"""Generate tests/golden/action_dist_many_heads.npz by RUNNING THE REFERENCE: get_action_distribution
(sample_factory/algo/utils/action_distributions.py:45-61) on Tuple spaces of more than eight members, evaluated in float64
on fixed logits, old logits and actions: log_prob, entropy, kl_divergence and (all-Discrete lists)
symmetric_kl_with_uniform_prior per row.  tests/test_many_heads_cpu.py holds the float64 restatement that judges the GPU
kernels (dist_terms of tests/test_gpu_action_heads.py) to these numbers, where no other fixture reaches.

Build machine only (the reference is not present where the GPU tests run); the fixture is committed.  Inputs are stored
as float32 (the file stays under 64 KB) and widened to float64 before the reference sees them.
Usage:  python tools/gen_golden_many_heads.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LISTS = {  # entry n > 0: Discrete(n); -D: Box(D)
    "h17x5": (5,) * 17,
    "h17x11": (11,) * 17,
    "h9x3_box2_4": (3,) * 9 + (-2, 4),
}
ROWS = 16


def main():
    from oracle import ref_import  # noqa: F401  (stubs for the reference's third-party imports)
    if not ref_import.reference_available():
        raise SystemExit("the reference is not present on this machine: the committed fixture stays as it is")
    import gymnasium as gym
    from sample_factory.algo.utils.action_distributions import get_action_distribution

    out = {}
    for li, (tag, heads) in enumerate(LISTS.items()):
        rng = np.random.default_rng(500 + li)
        space = gym.spaces.Tuple([gym.spaces.Discrete(h) if h > 0 else gym.spaces.Box(-1.0, 1.0, (-h,), np.float32)
                                  for h in heads])
        A = sum(h if h > 0 else -2 * h for h in heads)
        z = (rng.standard_normal((ROWS, A)) * 2.0).astype(np.float32)
        zo = (rng.standard_normal((ROWS, A)) * 2.0).astype(np.float32)
        z[::4, ::7] -= 60.0  # gaps that underflow a float32 softmax
        cols, off = [], 0
        for h in heads:
            if h > 0:
                cols.append(rng.integers(0, h, (ROWS, 1)))
                off += h
            else:  # log_std inside the clamp, and one row beyond each end of it
                for a in (z, zo):
                    a[:, off - h:off - 2 * h] = rng.uniform(-1.5, 1.0, (ROWS, -h))
                z[1, off - h], z[2, off - h] = -11.0, 10.5
                cols.append(rng.standard_normal((ROWS, -h)))
                off += -2 * h
        act = np.concatenate(cols, 1).astype(np.float32)
        t = lambda x: torch.tensor(x, dtype=torch.float64)
        new, old = get_action_distribution(space, t(z)), get_action_distribution(space, t(zo))
        out[f"{tag}.heads"] = np.asarray(heads, np.int32)
        out[f"{tag}.logits"], out[f"{tag}.old_logits"], out[f"{tag}.actions"] = z, zo, act
        out[f"{tag}.log_prob"] = new.log_prob(t(act)).numpy()
        out[f"{tag}.entropy"] = new.entropy().numpy()
        out[f"{tag}.kl"] = new.kl_divergence(old).numpy()
        if all(h > 0 for h in heads):  # ContinuousActionDistribution has no symmetric_kl_with_uniform_prior
            out[f"{tag}.symmetric_kl"] = new.symmetric_kl_with_uniform_prior().numpy()
        for k in ("log_prob", "entropy", "kl"):
            assert out[f"{tag}.{k}"].dtype == np.float64 and out[f"{tag}.{k}"].shape == (ROWS,)
    path = os.path.join(ROOT, "tests", "golden", "action_dist_many_heads.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
