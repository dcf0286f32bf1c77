"""Register and scratch budget of the tile-context kernels of the attribute pass of a point labelling (csrc/pointfield.hip:
k_pf_own_chunks, k_pf_own_hist), read from the compiler as in test_segdesc_resources.py: both compile for gfx950 without scratch and
without spilled registers and keep the occupancy of their twins k_pf_chunks and k_pf_hist, with which they share one templated body each
(pf_chunk_body<OWN> over sf_chunk_sums<OWN>, sf_hist_chunk<OWN>), read from the same compile.  The twins' own figures are held to what
they were before the bodies took the template parameter (k_pf_chunks: 53 VGPRs, k_pf_hist: 10 VGPRs, 8 waves per SIMD each), and so is
k_pf_anchor, which gained the own range's start as an argument: sharing has cost neither side."""
import os

import pytest

from test_pointfield_resources import _clean, _one
from test_segdesc_resources import HIPCC, _usage

NEW = ("k_pf_own_chunks", "k_pf_own_hist")
TWINS = {"k_pf_own_chunks": "k_pf_chunks", "k_pf_own_hist": "k_pf_hist"}
BEFORE = {"k_pf_chunks": 8, "k_pf_hist": 8, "k_pf_anchor": 8}   # waves per SIMD before this pass had tile kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tile_kernels_have_no_scratch_no_spills_and_their_twins_occupancy(tmp_path):
    k = _usage("pointfield.hip", tmp_path)
    for name in NEW:
        u = _one(k, name)
        print(name, u)
        _clean(name, u)
    for new, twin in TWINS.items():
        a, b = _one(k, new), _one(k, twin)
        assert a["Occupancy"] >= b["Occupancy"] >= BEFORE[twin], (new, a, twin, b)
    u = _one(k, "k_pf_anchor")
    _clean("k_pf_anchor", u)
    assert u["Occupancy"] >= BEFORE["k_pf_anchor"], u
