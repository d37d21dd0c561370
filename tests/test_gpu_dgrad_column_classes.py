"""The row order of the strided data gradient (k_dgrad_quadrow / k_dgrad_quadrow_z, sf_nn_glds.h): rows (sample, group
column) are tiled per COLUMN CLASS (the group columns that have the same tap columns inside dY), so that no tile
multiplies the zero tap columns of the image border.  The cases are the smallest launches at which that order can go
wrong: every class ending inside a tile, only border classes, an interior class one column wide, a non-square image,
one tap column (a single class) and three (five classes).

Every case, with and without the producer's ReLU mask:
  * the kernel-name query reports the row-walking kernel,
  * din against a float64 data gradient on the CPU at the ledger's tolerances (tests/test_gpu_kernel_ledger.py),
  * din allocated NaN-filled inside a guard band: finite everywhere afterwards (every element written), band intact,
  * for the cases of tests/golden/dgrad_column_classes.json: sha256 of din's bytes equal to the digest recorded with the
    kernel that still multiplied the zero columns (tools/gen_golden_dgrad_classes.py wrote the file on that commit).  The
    skipped products are exact zeros added to sums that start at +0, so the bytes may not change.
"""
import functools
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_kernel_ledger import DGRAD, F32, Case, Guarded, _elementwise, _maxnorm, make_desc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dgrad_column_classes.json")

# (Cin, H, W, Cout, K, S), n.  n >= 1024: below it the dispatcher does not pick the LDS-DMA data gradients.
CASES = [
    ((32, 20, 20, 64, 4, 2), 1024),  # conv2 of the Nature CNN, whole tiles: 1024 = 8 * 128 rows per group column
    ((32, 20, 20, 64, 4, 2), 1025),  # ... every class ends inside a tile
    ((32, 6, 4, 64, 4, 2), 1025),    # two group columns, OW = 1: only the two border classes, one tap column each
    ((32, 6, 6, 64, 4, 2), 1025),    # interior class one column wide
    ((32, 10, 14, 64, 4, 2), 1025),  # the ledger's non-square geometry
    ((32, 8, 8, 64, 2, 2), 1025),    # one tap column: a single class, nothing to skip
    ((32, 12, 12, 64, 6, 2), 1025),  # three tap columns: five classes
]
GOLDEN_CASES = CASES[:5]
MODES = ("mask", "nomask")


def case_id(geom, n):
    return "x".join(map(str, geom)) + f"-n{n}"


@functools.lru_cache(maxsize=1)
def _inputs(geom, n):
    return Case(F32, geom, n, 0.0, False)


@functools.lru_cache(maxsize=4)
def launch(geom, n, mode):
    """one launch of sf_conv_dgrad on the seeded inputs of the case -> (kernel name, din on the CPU, guard band intact?)"""
    c = _inputs(geom, n)
    Cin, H, W, Cout, K, S = geom
    d = make_desc(F32, geom, 0.0, 1)
    din = Guarded((n, H, W, Cin))
    din.t.fill_(float("nan"))
    lib.conv_dgrad(c.dy_dev, c.wk, c.x_dev if mode == "mask" else None, din.t, n, d)
    torch.cuda.synchronize()
    return lib.conv_kernel_name(DGRAD, n, d), din.t.cpu(), din.intact()


def digest(din):
    return hashlib.sha256(din.contiguous().numpy().tobytes()).hexdigest()


PARAMS = [(g, n, m) for g, n in CASES for m in MODES]
IDS = [f"{case_id(g, n)}-{m}" for g, n, m in PARAMS]


@pytest.mark.parametrize("geom,n,mode", PARAMS, ids=IDS)
def test_against_float64(geom, n, mode):
    Cin, H, W, Cout, K, S = geom
    name, din, intact = launch(geom, n, mode)
    assert name.startswith(("k_dgrad_quadrow_z<128, 128", "k_dgrad_quadrow<128, 128")), name
    assert intact, "the data gradient wrote outside din"
    assert bool(torch.isfinite(din).all()), "an element of din was not written (the NaN fill is still there)"
    c = _inputs(geom, n)
    _, _, gx, gmag = c.grads
    if mode == "mask":
        m = (c.x > 0).permute(0, 2, 3, 1)
        gx, gmag = gx * m, gmag * m
    got = din.double()
    rel = _maxnorm(got, gx, 3e-5, mode)
    ratio = _elementwise(got, gx, gmag, K * K * Cout, mode)
    print(f"dgrad classes {case_id(geom, n)} {name} {mode}: max|err|/max|ref| {rel:.3g} max(err/bound) {ratio:.3g}")


GPARAMS = [(g, n, m) for g, n in GOLDEN_CASES for m in MODES]


@pytest.mark.parametrize("geom,n,mode", GPARAMS, ids=[f"{case_id(g, n)}-{m}" for g, n, m in GPARAMS])
def test_bytes_equal_the_zero_multiplying_kernel(geom, n, mode):
    with open(GOLDEN) as f:
        golden = json.load(f)["sha256"]
    _, din, _ = launch(geom, n, mode)
    assert digest(din) == golden[f"{case_id(geom, n)}-{mode}"]
