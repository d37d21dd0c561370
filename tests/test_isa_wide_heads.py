"""Register and scratch budgets of the wave-per-row kernels for action spaces wider than 128 (csrc/sf_rl.hip), checked on
the hipcc listing (no GPU).  They stream rows from memory and want the occupancy: no scratch, and at most 128 registers
(vector + accumulation), i.e. four waves per SIMD out of the 512-register file."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

WIDE_KERNELS = ("k_sample_write_wide", "k_ppo_loss_wide", "k_vtrace_ratio_wide")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not (os.path.isfile(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "sf_rl.s"
    # the flags of sample_factory_amd/build.py for this source
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sample_factory_amd", "csrc"), "-S",
           "--cuda-device-only", os.path.join(ROOT, "sample_factory_amd", "csrc", "sf_rl.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {k["name"]: k for k in mod.kernel_stats(out.read_text())}


@pytest.mark.parametrize("kernel", WIDE_KERNELS)
def test_wide_kernel_has_no_scratch_and_keeps_four_waves_per_simd(listing, kernel):
    found = [k for name, k in listing.items() if kernel in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels of that name in the listing"
    k = found[0]
    assert k["scratch"] == 0, f"{kernel}: {k['scratch']} scratch instructions"
    used = k["vgpr"] + k["agpr"]
    assert used <= 128, f"{kernel}: {used} registers > 128"
