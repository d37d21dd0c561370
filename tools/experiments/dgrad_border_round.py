"""conv2 data gradient: what the last round (512 border tiles) costs.  A 20 x 4 image (two group columns, OW = 1) has only the
two border classes: at n = 32768 that is exactly one round of 512 border tiles with the chunk count of conv2's border tiles
(same H walk, same Cout), timed alone; conv2 itself = 4 interior rounds + that round."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
sys.path.insert(0, ROOT)
from sample_factory_amd import lib
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kbench import desc, timeit
n = 32768
res = {}
for name, geom in (("conv2 20x20", (32, 20, 20, 64, 4, 2)), ("border only 20x4", (32, 20, 4, 64, 4, 2))):
    d = desc(*geom)
    K = d.KH * d.KW * d.Cin; M = n * d.OH * d.OW
    w = torch.randn((K, d.Cout), device="cuda") / np.sqrt(K); dy = torch.randn((M, d.Cout), device="cuda")
    din = torch.empty((n, d.H, d.W, d.Cin), device="cuda")
    print(name, lib.conv_kernel_name(2, n, d), flush=True)
    res[name] = (d, w, dy, din)
for r in range(3):
    for name, (d, w, dy, din) in res.items():
        t = timeit(lambda: lib.conv_dgrad(dy, w, None, din, n, d), 20)
        print(f"round {r + 1} {name:18s} {t * 1e3:8.1f} us", flush=True)
