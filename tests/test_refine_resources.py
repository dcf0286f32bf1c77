"""Register and scratch budget of the label-refinement kernels (csrc/refine.hip), read from the compiler as in test_segdesc_resources.py:
every one of them compiles for gfx950 without scratch and without spilled registers."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_rf_init", "k_rf_unused_flags", "k_rf_unused_list", "k_rf_mark", "k_rf_refine")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refine_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("refine.hip", tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in KERNELS)}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
