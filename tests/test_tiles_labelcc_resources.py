"""Register and scratch budget of the tile-context kernels of the connected parts of a point labelling (csrc/labelcc_tiles.hip), read
from the compiler as in test_labelcc_resources.py: every k_lt_* kernel compiles for gfx950 without scratch and without spilled
registers, and each is one instantiation under its name."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_lt_band_flags", "k_lt_band_records", "k_lt_part_codes", "k_lt_find", "k_lt_unused_flags", "k_lt_unused_list", "k_lt_link_short",
           "k_lt_link_long", "k_lt_apply")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_label_component_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("labelcc_tiles.hip", tmp_path)
    ours = {n: v for n, v in k.items() if "k_lt_" in n}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    assert len(ours) == len(KERNELS), sorted(ours)
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
