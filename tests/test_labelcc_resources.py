"""Register and scratch budget of the kernels of the connected parts of a point labelling (csrc/labelcc.hip), read from the compiler as
in test_pointfield_resources.py: every k_lc_* kernel compiles for gfx950 without scratch and without spilled registers."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_lc_heads", "k_lc_vertices", "k_lc_vfirst", "k_lc_unused_flags", "k_lc_unused_list", "k_lc_link_short", "k_lc_link_long",
           "k_lc_compress", "k_lc_roots", "k_lc_parts", "k_lc_label_first", "k_lc_largest_fold", "k_lc_largest", "k_lc_scatter")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_label_component_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("labelcc.hip", tmp_path)
    ours = {n: v for n, v in k.items() if "k_lc_" in n}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    assert len(ours) == len(KERNELS), sorted(ours)
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
