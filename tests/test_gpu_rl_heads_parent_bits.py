"""The action-head kernels of csrc/sf_rl.hip (k_ppo_loss<MAXA>, k_ppo_loss_md / _mh / _wide, k_vtrace_ratio<MAXA> / _wide
with k_vtrace, and the four samplers, lane-per-row and wave-per-row) after their repeated arithmetic was folded into
shared device helpers: bit equality of every output with tests/golden/rl_heads_parent.npz, written by
the commit before that change from the same host-drawn inputs (tools/gen_golden_rl_heads_parent.py).  The file is built
with -ffp-contract=off, so a helper that keeps the operation order keeps the bits; a moved operand or a changed clamp,
tie rule or Philox counter shows here at the first case that reaches it.

Cases are sized so that the loss's double atomics do not depend on block order: at most 256 rows (one block) on the
lane-per-row kernels, 7 rows (two blocks, 0 + a + b) on the wave-per-row ones."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "rl_heads_parent.npz")


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert str(g["parent"]) == gen.PARENT
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


@pytest.mark.parametrize("case", gen.LOSS_CASES, ids=lambda c: c[0])
def test_ppo_loss_bits(lib, golden, case):
    out = gen.run_loss_case(lib, case)
    # the case holds what it is there for: a raw ratio beyond the hard clamp on both sides, invalid rows
    assert out["ratio"][0] == 20.0 and out["ratio"][1] == np.float32(0.05)
    assert (out["grads"] == 0).all(1).any(), "no invalid row in the minibatch"
    check_bits(golden, case[0], out)


@pytest.mark.parametrize("case", gen.VTRACE_CASES, ids=lambda c: c[0])
def test_vtrace_bits(lib, golden, case):
    check_bits(golden, case[0], gen.run_vtrace_case(lib, case))


@pytest.mark.parametrize("deterministic", [False, True], ids=["draw", "det"])
@pytest.mark.parametrize("case", gen.SAMPLER_CASES, ids=lambda c: c[0])
def test_sampler_bits(lib, golden, case, deterministic):
    out = gen.run_sampler_case(lib, case, deterministic)
    assert out["logits_ok"] == 1, "the recorded logits are not the input's, or another step was written"
    check_bits(golden, f"{case[0]}_{'det' if deterministic else 'draw'}", out)
