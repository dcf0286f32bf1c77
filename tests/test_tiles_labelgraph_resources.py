"""Register and scratch budget of the tile-context kernels of the label graph (csrc/labelgraph_tiles.hip), read from the compiler as in
test_tiles_labelcc_resources.py: every k_lgt_* kernel compiles for gfx950 without scratch and without spilled registers, and each is one
instantiation under its name (the row kernel: its count and its write instantiation)."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_lgt_merge_keys", "k_lgt_split_keys", "k_lgt_unused_flags", "k_lgt_unused_list", "k_lgt_rowsILb0", "k_lgt_rowsILb1")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_label_graph_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("labelgraph_tiles.hip", tmp_path)
    ours = {n: v for n, v in k.items() if "k_lgt_" in n}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    assert len(ours) == len(KERNELS), sorted(ours)
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
