"""The action-head kernels that came after tests/golden/rl_heads_parent.npz was written (k_masked_ppo_loss_md / _mh /
_wide, k_masked_vtrace_ratio / _wide, k_consistency_loss / _wide): bit equality of every output with
tests/golden/rl_heads_parent2.npz, written by commit PARENT2 from the same host-drawn inputs
(tools/gen_golden_rl_heads_parent.py --second).  The file is built with -ffp-contract=off, so a rewrite
that keeps the operation order keeps the bits; a swapped pointer, a stride taken from the wrong argument or a mask row
read through the wrong mapping shows here at the first case that reaches it.

Sizes follow the rule of test_gpu_rl_heads_parent_bits.py: at most 256 rows (one block) on the lane-per-row kernels, 7 rows
on the wave-per-row ones, so the double atomics do not depend on block order."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_rl_heads_parent",
                                               os.path.join(ROOT, "tools", "gen_golden_rl_heads_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = os.path.join(ROOT, "tests", "golden", "rl_heads_parent2.npz")


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert str(g["parent"]) == gen.PARENT2
    return g


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}") if a.dtype.kind == "f" else a


def check_bits(golden, name, out):
    want = {k.split("/", 1)[1] for k in golden.files if k.startswith(name + "/")}
    assert want == set(out), (name, sorted(want), sorted(out))
    for k, v in out.items():
        g = golden[f"{name}/{k}"]
        assert g.dtype == v.dtype and g.shape == v.shape, (name, k, g.dtype, v.dtype, g.shape, v.shape)
        diff = bits(g) != bits(v)
        assert not diff.any(), (f"{name}/{k}: {int(diff.sum())} of {diff.size} elements differ in bits from the parent "
                                f"commit's, first at {np.argwhere(diff)[0].tolist()}")


@pytest.mark.parametrize("case", gen.MASKED_LOSS_CASES, ids=lambda c: c[0])
def test_masked_ppo_loss_bits(lib, golden, case):
    out = gen.run_loss_case(lib, case)
    # the case holds what it is there for: both hard clamps of the ratio, an invalid row, all-masked member rows
    assert out["ratio"][0] == 20.0 and out["ratio"][1] == np.float32(0.05)
    assert (out["grads"] == 0).all(1).any(), "no invalid row in the minibatch"
    assert out["all_masked_rows"] > 0, "no valid row with an all-masked member in the minibatch"
    assert np.isfinite(out["grads"]).all() and np.isfinite(out["sums"]).all()
    check_bits(golden, case[0], out)


@pytest.mark.parametrize("case", gen.MASKED_VTRACE_CASES, ids=lambda c: c[0])
def test_masked_vtrace_bits(lib, golden, case):
    out = gen.run_vtrace_case(lib, case)
    assert np.isfinite(out["vs"]).all() and np.isfinite(out["adv"]).all()
    check_bits(golden, case[0], out)


@pytest.mark.parametrize("case", gen.CONSISTENCY_CASES, ids=lambda c: c[0])
def test_consistency_loss_bits(lib, golden, case):
    out = gen.run_consistency_case(lib, case)
    n = case[2]
    g = out["grads"]
    assert (g[:n] == gen.SENT).all(), "the target rows' gradient was written"
    assert (g[n:] == 0).all(1).any(), "no invalid row in the minibatch"
    assert np.isfinite(g).all() and np.isfinite(out["sums"]).all() and out["sums"][0] > 0
    check_bits(golden, case[0], out)
