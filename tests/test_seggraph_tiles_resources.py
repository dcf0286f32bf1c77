"""Register and scratch budget of the kernels the tiled segment graph adds to csrc/seggraph.hip (the halo-label lookup, the tile label
kernel, the row walk over owned rows in both of its passes), read from the compiler as in test_seggraph_resources.py: no scratch and no
spilled registers on gfx950.  The single-engine row walks must still be there under their own names."""
import os

import pytest

from test_seggraph_resources import HIPCC, _usage

# (k_sg_rows<WRITE, TILE>: ILb0ELb1E = the count pass over owned rows, ILb1ELb1E = the write pass)
KERNELS = ("k_sg_halo_find", "k_sg_tile_labels", "k_sg_rowsILb0ELb1E", "k_sg_rowsILb1ELb1E")
SINGLE = ("k_sg_rowsILb0ELb0E", "k_sg_rowsILb1ELb0E")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_graph_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("seggraph.hip", tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in KERNELS)}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    for name, u in ours.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
    assert all(any(s in n for n in k) for s in SINGLE), sorted(k)
