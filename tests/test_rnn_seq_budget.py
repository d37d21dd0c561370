"""Static budgets of the width-1024 sequence kernels (csrc/sf_rnn_wideseq.h), checked on the hipcc listing (no GPU): one
kernel per instantiation the launcher can pick, 160 KB of LDS with one work-group per CU, 512 registers per lane at one wave
per SIMD, no scratch, and a hottest block that is the MFMA loop.  A change that spills or outgrows LDS shows up here before
it reaches a GPU box (a persistent kernel that cannot be co-resident would wait for work-groups that never start)."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# scratch instructions the listing of this tree has (hipcc -O3 -ffp-contract=off on csrc/sf_rnn.hip, the flags of
# sample_factory_amd/build.py): 0 for every forward instantiation and 0 for the LDS-form backward ones (8 hidden units per
# work-group: 102 - 209 VGPRs + 4 AGPRs)
SCRATCH = {"fwd": 0, "bwd": 0}
# mangled-name fragment -> (pass, static LDS bytes the source asks for: W_hh slice + 4 staging tiles + the flag word)
KERNELS = {f"k_wideseq_{d}ILi{kind}ELi{nsub}EE": (d, lds)
           for d, per_kind in (("fwd", {0: 32 * 1028 + 4 * 128 + 4, 1: 32 * 1028 + 4 * 128 + 4}),
                               ("bwd", {0: 8 * 3076 + 4 * 384 + 4, 1: 8 * 4100 + 4 * 512 + 4}))
           for kind, lds in ((k, 4 * v) for k, v in per_kind.items()) for nsub in (1, 2, 4)}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not (os.path.isfile(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "sf_rnn.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "sample_factory_amd", "csrc"), "-S", "--cuda-device-only",
           os.path.join(ROOT, "sample_factory_amd", "csrc", "sf_rnn.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {k["name"]: k for k in mod.kernel_stats(out.read_text())}


def test_every_instantiation_the_launcher_picks_exists_once(listing):
    wide = [n for n in listing if "k_wideseq_" in n]
    assert len(wide) == len(KERNELS) == 12, wide
    for fragment in KERNELS:
        assert sum(fragment in n for n in wide) == 1, fragment


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_wide_kernel_stays_inside_its_budget(listing, fragment):
    direction, lds = KERNELS[fragment]
    k = next(v for n, v in listing.items() if fragment in n)
    used = k["vgpr"] + k["agpr"]
    print(f"{fragment}: {k['vgpr']} VGPR + {k['agpr']} AGPR, {k['scratch']} scratch, {k['lds']} B LDS, hot block {k['hot']}")
    assert used <= 512, f"{fragment}: {used} registers per lane (one wave per SIMD has 512)"
    assert k["scratch"] <= SCRATCH[direction], f"{fragment}: {k['scratch']} scratch instructions (spills in the step loop)"
    assert (k["lds"] or 0) <= 160 * 1024, f"{fragment}: {k['lds']} bytes of static LDS > 160 KB"
    assert k["lds"] == lds, f"{fragment}: {k['lds']} bytes of static LDS, the source asks for {lds}"
    assert 2 * k["lds"] > 160 * 1024 or used > 256, "one work-group per CU is what keeps the grid co-resident"
    hot = k["hot"]
    assert hot["mfma"] >= 32 and hot["mfma"] > hot["valu"], f"{fragment}: the hottest block is not the MFMA loop: {hot}"
