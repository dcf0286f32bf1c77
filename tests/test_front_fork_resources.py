"""Resource budget of the features stage's kernels, read from the compiler (hipcc cross-compiles gfx950 without a GPU).  k_features lost
its used-flag store to k_used_flags and runs on a side stream beside the adjacency kernels: both instantiations must keep what they had
before that change -- registers, LDS (three tiles of 2048 floats) and wavefronts per SIMD -- and k_used_flags, a pass over the voxel
table, needs no scratch."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

# the compiler's report for k_features<256> / k_features<64> with the used-flag store still inside (the parent of the front fork)
PARENT = {
    "_Z10k_featuresILi256EEv": dict(vgprs=72, occupancy=6),
    "_Z10k_featuresILi64EEv": dict(vgprs=72, occupancy=2),   # (LDS: one 64-thread workgroup holds the same three tiles)
}
LDS_BYTES = 3 * 2048 * 4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_features_kernels_keep_their_budget_and_used_flags_has_no_scratch(tmp_path):
    k = _usage("features.hip", tmp_path)
    for prefix, want in PARENT.items():
        hit = {n: v for n, v in k.items() if n.startswith(prefix)}
        assert len(hit) == 1, sorted(k)
        (name, u), = hit.items()
        assert u["VGPRs"] <= want["vgprs"], (name, u)
        assert u["Occupancy"] >= want["occupancy"], (name, u)
        assert u["LDS Size"] == LDS_BYTES, (name, u)
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0, (name, u)
    flags = {n: v for n, v in k.items() if n.startswith("_Z12k_used_flags")}
    assert len(flags) == 1, sorted(k)
    (name, u), = flags.items()
    assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["LDS Size"] == 0, (name, u)
