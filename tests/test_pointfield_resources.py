"""Register and scratch budget of the attribute kernels of a point labelling (csrc/pointfield.hip), read from the compiler as in
test_pointseg_resources.py: every one of them compiles for gfx950 without scratch and without spilled registers, and the two chunk
kernels, which run the bodies of csrc/segpass.hpp that k_sf_chunks and k_sf_hist run, reach those kernels' occupancy, read from the same
compiler in the same run -- sharing the bodies must not cost either side a register budget.  The kernel set of csrc/segfield.hip, whose
bodies moved into the shared header, is still free of scratch and spills."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

KERNELS = ("k_pf_anchor", "k_pf_chunks", "k_pf_hist")
TWINS = {"k_pf_chunks": "k_sf_chunksP", "k_pf_hist": "k_sf_histP"}   # (the P of the mangled name's first parameter: not k_sf_chunks_own)
SEGFIELD = ("k_sf_anchor", "k_sf_chunks", "k_sf_chunks_own", "k_sf_final", "k_sf_own_records", "k_sf_hist", "k_sf_hist_own", "k_sf_majority")


def _one(kernels, name):
    hit = [v for n, v in kernels.items() if name in n]
    assert len(hit) == 1, (name, sorted(kernels))
    return hit[0]


def _clean(name, u):
    assert u["ScratchSize"] == 0, (name, u)
    assert u["VGPRs Spill"] == 0, (name, u)
    assert u["SGPRs Spill"] == 0, (name, u)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_point_field_kernels_have_no_scratch_no_spills_and_their_twins_occupancy(tmp_path):
    k = _usage("pointfield.hip", tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in KERNELS)}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    assert len(ours) == len(KERNELS), sorted(ours)
    for name, u in ours.items():
        print(name, u)
        _clean(name, u)
    sf = _usage("segfield.hip", tmp_path)
    theirs = {n: v for n, v in sf.items() if "k_sf_" in n}
    assert len(theirs) >= len(SEGFIELD) and all(any(s in n for n in theirs) for s in SEGFIELD), sorted(sf)
    for name, u in theirs.items():
        print(name, u)
        _clean(name, u)
    for new, twin in TWINS.items():
        a, b = _one(k, new), _one(sf, twin)
        assert a["Occupancy"] >= b["Occupancy"], (new, a, twin, b)
