"""Register and scratch budget of the tile-context kernels of the point-labelling pass (csrc/pointseg.hip: k_ps_shared, k_ps_own_chunks,
k_ps_pairs, k_ps_own_records), read from the compiler as in test_segdesc_resources.py: every one of them compiles for gfx950 without
scratch and without spilled registers, and the chunk and fold kernels keep the occupancy of their twins k_ps_chunks and k_ps_final, with
which they share one templated body each.  The twins' own figures are held to what they were before the bodies became templates
(k_ps_chunks: 56 VGPRs, 8 waves per SIMD; k_ps_final: 66 VGPRs, 7 waves per SIMD), so sharing the body has cost neither side."""
import os

import pytest

from test_pointseg_resources import _one
from test_segdesc_resources import HIPCC, _usage

NEW = ("k_ps_shared", "k_ps_own_chunks", "k_ps_pairs", "k_ps_own_records")
TWINS = {"k_ps_own_chunks": "k_ps_chunksP", "k_ps_own_records": "k_ps_final"}
BEFORE = {"k_ps_chunksP": 8, "k_ps_final": 7}   # waves per SIMD of the twins before this pass had tile kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_kernels_have_no_scratch_no_spills_and_their_twins_occupancy(tmp_path):
    k = _usage("pointseg.hip", tmp_path)
    for name in NEW:
        u = _one(k, name)
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
    for new, twin in TWINS.items():
        a, b = _one(k, new), _one(k, twin)
        assert a["Occupancy"] >= b["Occupancy"] >= BEFORE[twin], (new, a, twin, b)
    for name in ("k_ps_shared", "k_ps_pairs"):   # one load, one compare, one store per thread: nothing that could limit them
        assert _one(k, name)["Occupancy"] >= _one(k, "k_ps_keys")["Occupancy"], name
