"""Register and scratch budget of the label-comparison kernels (csrc/segcompare.hip), read from the compiler as in
test_segbox_resources.py: every one of them compiles for gfx950 without scratch and without spilled registers."""
import os

import pytest

from test_segbox_resources import _check
from test_segdesc_resources import HIPCC

KERNELS = ("k_cmp_scan", "k_cmp_keys", "k_cmp_heads", "k_cmp_cell_starts", "k_cmp_cell_counts", "k_cmp_row_starts", "k_cmp_seg_rows",
           "k_cmp_ref_keys", "k_cmp_ref_starts", "k_cmp_ref_rows", "k_cmp_seg_iou")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_label_comparison_kernels_have_no_scratch_and_no_spills(tmp_path):
    ours = _check("segcompare.hip", KERNELS, tmp_path)
    for name, u in ours.items():
        print(name, u)
