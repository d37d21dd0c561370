"""Scratch budget of the kernels that carry a head list of up to SF_MAX_ACTION_HEADS = 64 members (csrc/sf_rl.hip), checked
on the hipcc listing (no GPU).  k_ppo_loss_mh is new: it must not keep per-member state in a lane (seven float[64] arrays
would be 448 registers, i.e. scratch).  The others only received the longer list as a kernel argument, which the compiler
must go on reading from the argument segment and not copy to scratch to index it.  Nothing but the compiler's metadata
is looked at; the register counts are recorded in DESIGN.md §3.10."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

NEW_KERNELS = ("k_ppo_loss_mh",)
LONGER_LIST = ("k_ppo_loss_md", "k_sample_write_tuple", "k_vtrace_ratioILi8E", "k_vtrace_ratioILi32E",
               "k_vtrace_ratioILi128E", "k_loss_scalars")


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


@pytest.mark.parametrize("kernel", NEW_KERNELS + LONGER_LIST)
def test_head_list_kernel_has_no_scratch(listing, kernel):
    found = [k for name, k in listing.items() if kernel in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels of that name in the listing"
    k = found[0]
    assert k["scratch"] == 0, f"{kernel}: {k['scratch']} scratch instructions"
    print(f"{kernel}: {k['vgpr']} VGPR, {k['agpr']} AGPR, {k['lds']} bytes of LDS")


def test_long_list_loss_kernel_keeps_the_occupancy_of_the_eight_member_one(listing):
    """no per-member arrays: fewer registers than k_ppo_loss_md, which keeps seven float[8]"""
    mh = next(k for name, k in listing.items() if "k_ppo_loss_mh" in name)
    md = next(k for name, k in listing.items() if "k_ppo_loss_md" in name)
    assert mh["vgpr"] + mh["agpr"] <= md["vgpr"] + md["agpr"], (mh, md)
