"""Resource budget of the merge front, read from the compiler (hipcc cross-compiles gfx950 without a GPU).  k_cross and k_union_mutual
wait on chains of dependent loads, so their throughput is loads in flight over latency: both must keep eight wavefronts per SIMD without
scratch, and the per-row lists in LDS must stay small enough that 32 single-wavefront workgroups share a compute unit."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_merge_front_keeps_eight_wavefronts_without_scratch(tmp_path):
    k = _usage("merge.hip", tmp_path)
    front = {n: v for n, v in k.items() if n.startswith("_Z7k_cross") or n.startswith("_Z14k_union_mutual")}
    assert len(front) == 2, sorted(k)
    for name, u in front.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["Occupancy"] >= 8, (name, u)
        assert u["LDS Size"] <= 2048, (name, u)
