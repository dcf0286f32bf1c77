"""Register and scratch budget of the point-labelling kernels (csrc/pointseg.hip), read from the compiler as in test_segdesc_resources.py:
every one of them compiles for gfx950 without scratch and without spilled registers, and the kernels that run a body of
csrc/segpass.hpp reach the occupancy of the node-pass kernel that runs the same body (k_sd_chunks, k_sd_final, k_sb_chunks, k_sb_final),
read from the same compiler in the same run -- sharing the bodies must not cost either side a register budget."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_ps_keys", "k_ps_segments", "k_ps_chunks", "k_ps_final", "k_ps_box_chunks", "k_ps_box_final")
# new kernel -> (source file, kernel) whose body it shares
TWINS = {"k_ps_chunks": ("segdesc.hip", "k_sd_chunksP"), "k_ps_final": ("segdesc.hip", "k_sd_final"),
         "k_ps_box_chunks": ("segbox.hip", "k_sb_chunksP"), "k_ps_box_final": ("segbox.hip", "k_sb_final")}


def _one(kernels, name):
    hit = [v for n, v in kernels.items() if name in n]
    assert len(hit) == 1, (name, sorted(kernels))
    return hit[0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_point_labelling_kernels_have_no_scratch_no_spills_and_their_twins_occupancy(tmp_path):
    k = _usage("pointseg.hip", tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in KERNELS)}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
    other = {src: _usage(src, tmp_path) for src in sorted({s for s, _ in TWINS.values()})}
    for new, (src, twin) in TWINS.items():
        a, b = _one(k, new), _one(other[src], twin)
        assert a["Occupancy"] >= b["Occupancy"], (new, a, twin, b)
    for name in ("k_ps_keys", "k_ps_segments"):   # the two passes over keys: nothing that could limit them
        assert _one(k, name)["Occupancy"] >= _one(other["segdesc.hip"], "k_sd_keys")["Occupancy"], name
