"""Fixture of the conv2 weight gradient (k_wgrad_img<32, 20, 20, 4, 2, 2>, selected for n >= 512):
    python tools/gen_golden_wgrad_conv2.py [out.npz]
draws x [n, 20, 20, 32] and dY [n, 9, 9, 64] on the HOST from numpy.random.default_rng(seed) (identical on every machine),
runs lib.conv_wgrad on the conv2 descriptor and stores dW [512, 64] and db [64] per n with the seeds.  The committed
tests/golden/wgrad_conv2_parent.npz was written by the commit BEFORE the staggered kernel: tests/test_gpu_wgrad_conv2.py
asks for bit equality with it (same operands in the same order into every accumulator).  Needs a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CIN, H, W, COUT, KS, ST, OH, OW = 32, 20, 20, 64, 4, 2, 9, 9
# 512: 2 samples per work-group; 513: per = 3, trailing work-groups short or empty; 1025: per = 5, odd, crosses both stages
NS = (512, 513, 1025)


def seed_of(n):
    return 20000 + n


def conv2_desc(lib):
    return lib.sf_conv_desc(Cin=CIN, H=H, W=W, Cout=COUT, KH=KS, KW=KS, stride=ST, OH=OH, OW=OW, in_u8=0, relu=1, traj_T=0,
                            sub_mean=0.0, inv_scale=1.0)


def make_inputs(n, seed):
    """(x [n, 20, 20, 32], dY [n, 9, 9, 64]) float32, NHWC, drawn on the host"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, H, W, CIN), dtype=np.float32)
    dy = rng.standard_normal((n, OH, OW, COUT), dtype=np.float32)
    return x, dy


def run_wgrad(lib, x_dev, dy_dev, n, ws=None):
    """(dW [512, 64], db [64]) of lib.conv_wgrad on device tensors x [n, 20, 20, 32] and dY [n * 81, 64]"""
    import torch
    d = conv2_desc(lib)
    dw = torch.zeros((KS * KS * CIN, COUT), device="cuda")
    db = torch.zeros(COUT, device="cuda")
    if ws is None:
        ws = torch.empty(lib.conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
    lib.conv_wgrad(x_dev, CIN * H * W, None, 0, dy_dev.view(n * OH * OW, COUT), dw, db, n, d, ws)
    return dw, db


def main():
    import torch
    from sample_factory_amd import lib
    lib.load()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "wgrad_conv2_parent.npz")
    rec = {}
    for n in NS:
        x, dy = make_inputs(n, seed_of(n))
        dw, db = run_wgrad(lib, torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda(), n)
        torch.cuda.synchronize()
        rec[f"dw_{n}"], rec[f"db_{n}"], rec[f"seed_{n}"] = dw.cpu().numpy(), db.cpu().numpy(), np.int64(seed_of(n))
        print(f"n={n}: |dW|max {np.abs(rec[f'dw_{n}']).max():.4f} |db|max {np.abs(rec[f'db_{n}']).max():.4f}", flush=True)
    np.savez(out, **rec)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
