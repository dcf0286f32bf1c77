"""Register and scratch budget of what the tiled label comparison adds to csrc/segcompare.hip, read from the compiler as in
test_segcompare_resources.py: k_cmp_scan_own (step 1 over a rank's own points, with the largest label), k_cmp_cells_scan,
k_cmp_cells_keys and k_cmp_cells_sums (the merge of a cell list) compile for gfx950 without scratch and without spilled registers, and no
other kernel was added."""
import os

import pytest

from test_segbox_resources import _check
from test_segcompare_resources import KERNELS
from test_segdesc_resources import HIPCC, _usage

ADDED = ("k_cmp_scan_own", "k_cmp_cells_scan", "k_cmp_cells_keys", "k_cmp_cells_sums")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cell_merge_kernels_have_no_scratch_and_no_spills(tmp_path):
    ours = _check("segcompare.hip", ADDED, tmp_path)
    for name, u in ours.items():
        print(name, u)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_exactly_the_listed_kernels_were_added(tmp_path):
    usage = _usage("segcompare.hip", tmp_path)
    ours = sorted(n for n in usage if "k_cmp_" in n)
    # k_cmp_heads is a template with two instantiations (64-bit point and cell keys, 32-bit id keys)
    assert len(ours) == len(KERNELS) + 1 + len(ADDED), ours
    for name in ADDED:
        assert len([n for n in ours if f"{len(name)}{name}" in n]) == 1, (name, ours)
