"""Register and scratch budget of the oriented-box kernels (csrc/segbox.hip), read from the compiler as in test_segdesc_resources.py: every
one of them compiles for gfx950 without scratch and without spilled registers -- and the descriptor kernels (csrc/segdesc.hip), whose
sd_prepare the box pass shares through vgs_context.hpp, still do."""
import os

import pytest

from test_segdesc_resources import HIPCC, KERNELS as SD_KERNELS, _usage

KERNELS = ("k_sb_frames", "k_sb_chunks", "k_sb_final")


def _check(src, names, tmp_path):
    k = _usage(src, tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in names)}
    assert sorted(n for n in names if any(n in m for m in ours)) == sorted(names), sorted(k)
    for name, u in ours.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
    return ours


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_segment_box_kernels_have_no_scratch_and_no_spills(tmp_path):
    ours = _check("segbox.hip", KERNELS, tmp_path)
    for name, u in ours.items():
        print(name, u)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_segment_descriptor_kernels_still_have_no_scratch_and_no_spills(tmp_path):
    _check("segdesc.hip", SD_KERNELS, tmp_path)
