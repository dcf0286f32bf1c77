"""Register, scratch and LDS budget of the kernels that the tiled label refinement adds to csrc/refine.hip, read from the compiler as in
test_refine_resources.py: every one of them compiles for gfx950 without scratch and without spilled registers, and the tile variant of
the refine kernel stays within the 8 KB of LDS of the single-context one."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_rf_band_flags", "k_rf_band_compact", "k_rf_tile_labels", "k_rf_tile_init", "k_rf_tile_fill_flags",
           "k_rf_tile_mark", "k_rf_tile_refine")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_refine_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("refine.hip", tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in KERNELS)}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
    lds = {n: u["LDS Size"] for n, u in k.items() if "k_rf_refine" in n or "k_rf_tile_refine" in n}
    print(lds)
    assert len(lds) == 2 and all(v <= 8192 for v in lds.values()), lds
