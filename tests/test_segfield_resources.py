"""Register and scratch budget of the segment-attribute kernels (csrc/segfield.hip), read from the compiler as in test_segbox_resources.py:
every one of them compiles for gfx950 without scratch and without spilled registers."""
import os

import pytest

from test_segbox_resources import _check
from test_segdesc_resources import HIPCC

KERNELS = ("k_sf_anchor", "k_sf_chunks", "k_sf_final", "k_sf_hist", "k_sf_majority")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_segment_field_kernels_have_no_scratch_and_no_spills(tmp_path):
    ours = _check("segfield.hip", KERNELS, tmp_path)
    for name, u in ours.items():
        print(name, u)
