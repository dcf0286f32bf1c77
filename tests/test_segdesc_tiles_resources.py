"""Register and scratch budget of the kernels the tiled descriptors add to csrc/segdesc.hip (own-point anchor, own-point chunks, moment
records, the algebra over folded moments), read from the compiler as in test_segdesc_resources.py: no scratch and no spilled registers
on gfx950."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_sd_own_anchor", "k_sd_chunks_own", "k_sd_own_records", "k_sd_algebra")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_descriptor_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("segdesc.hip", tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in KERNELS)}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    for name, u in ours.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
