"""The u8 normalising loader of the register-staged conv kernels (MODE_U8_NORM = 5 of csrc/sf_nn.hip), checked on the hipcc
listing without a GPU: every forward / weight-gradient instantiation exists, has no scratch and fits as many waves per SIMD
as the f32-frame sibling (MODE_F32F_NORM = 4) of the same tile, both read from the same listing."""
import re

import pytest

from tests.test_isa_budget import listing  # noqa: F401  (the module-scoped fixture: one hipcc -S run of sf_nn.hip)

FWD_TILES = ("Li256ELi32ELi4ELi1E", "Li128ELi32ELi4ELi1E", "Li128ELi64ELi2ELi2E", "Li64ELi64ELi2ELi2E")
WGRAD_TILES = ("Li32ELi4ELi1E", "Li64ELi2ELi2E")


def _one(listing, kernel, tile, mode):  # noqa: F811
    pat = re.compile(r"^_Z\d+%sI%sLi%dEE" % (kernel, tile, mode))
    found = [k for name, k in listing.items() if pat.match(name)]
    assert len(found) == 1, f"{kernel}<{tile}, {mode}>: {len(found)} instantiations in the listing"
    return found[0]


def _waves(k):
    used = k["vgpr"] + k["agpr"]
    return 512 // ((used + 7) // 8 * 8)  # waves per SIMD that share 512 registers, allocation granule 8


@pytest.mark.parametrize("kernel,tile", [("k_conv_fwd", t) for t in FWD_TILES] + [("k_conv_wgrad", t) for t in WGRAD_TILES])
def test_u8_norm_instantiation_matches_its_f32_sibling(listing, kernel, tile):  # noqa: F811
    u8, f32 = _one(listing, kernel, tile, 5), _one(listing, kernel, tile, 4)
    assert u8["scratch"] == 0, f"{kernel}<{tile}, 5>: {u8['scratch']} scratch instructions (spills)"
    assert u8["hot"]["mfma"] >= 16, "the hottest block is the MFMA loop"
    assert _waves(u8) >= _waves(f32), (f"{kernel}<{tile}>: {u8['vgpr']} + {u8['agpr']} registers -> {_waves(u8)} waves per "
                                       f"SIMD, the f32 mode has {f32['vgpr']} + {f32['agpr']} -> {_waves(f32)}")
    assert (u8["lds"] or 0) == (f32["lds"] or 0)
