"""Register and scratch budget of the absorb kernels (csrc/labelabsorb.hip), read from the compiler's resource remarks as in
test_labelgraph_resources.py: every one of them compiles for gfx950 without scratch and without spilled registers."""
import os

import pytest

from test_labelgraph_resources import HIPCC, _usage

KERNELS = ("k_la_candidates", "k_la_records", "k_la_runs", "k_la_targets", "k_la_apply", "k_la_finish")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_label_absorb_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("labelabsorb.hip", tmp_path)
    ours = {n: v for n, v in k.items() if "k_la_" in n}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    assert len(ours) == len(KERNELS), sorted(ours)   # every kernel of the file is named above
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
