"""Register, scratch, LDS and occupancy budget of the label-refinement kernels (csrc/refine.hip), single context and tile contexts, read
from the compiler as in test_segdesc_resources.py: every one of them compiles for gfx950 without scratch and without spilled registers,
both refine kernels -- two entry points of one body -- stay within 8 KB of LDS and five wavefronts per SIMD, and every other kernel
reaches eight."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

REFINE = ("k_rf_refine", "k_rf_tile_refine")
KERNELS = ("k_rf_init", "k_rf_unused_flags", "k_rf_unused_list", "k_rf_mark", "k_rf_refine")
TILE_KERNELS = ("k_rf_band_flags", "k_rf_band_compact", "k_rf_tile_labels", "k_rf_tile_init", "k_rf_tile_mark", "k_rf_tile_refine")
_compiled = {}


def _checked(names, tmp_path):
    """the compiler's figures of refine.hip (compiled once); scratch, spills and the occupancy floor of the kernels `names`"""
    if not _compiled:
        _compiled.update(_usage("refine.hip", tmp_path))
    k = _compiled
    ours = {n: v for n, v in k.items() if any(s in n for s in names)}
    assert sorted(n for n in names if any(n in m for m in ours)) == sorted(names), sorted(k)
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
        assert u["Occupancy"] >= (5 if any(s in name for s in REFINE) else 8), (name, u)   # (waves per SIMD)
    return k


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refine_kernels_have_no_scratch_and_no_spills(tmp_path):
    _checked(KERNELS, tmp_path)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_refine_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _checked(TILE_KERNELS, tmp_path)
    lds = {n: u["LDS Size"] for n, u in k.items() if any(s in n for s in REFINE)}
    print(lds)
    assert len(lds) == 2 and all(v <= 8192 for v in lds.values()), lds
