"""Register and scratch budget of what the tiled attribute statistics add to csrc/segfield.hip, read from the compiler as in
test_segdesc_resources.py:
  * the added kernels -- k_sf_chunks_own and k_sf_hist_own, the own-point forms of the two chunk kernels; k_sf_anchor_own, the values of
    every label's first own point; k_sf_own_records, the fold of k_sf_final that leaves the sums as they are -- have no scratch and no
    spilled registers on gfx950, and no other kernel was added;
  * k_sf_anchor, k_sf_chunks, k_sf_final, k_sf_hist and k_sf_majority keep the VGPR and SGPR counts they had before the chunk bodies became
    templates over OWN -- the single-context instantiations compile to what they compiled to at commit 96c6094, where these figures were
    read.  (k_sf_final is also the finish of the tiled table, over one partial per entry: its tail is not a function of its own, because
    the compiler then gives the kernel another register allocation, 30 VGPRs.)
  * csrc/segdesc.hip only gained a host function around the launch of k_sd_own_anchor: its kernels keep their counts too."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

ADDED = ("k_sf_anchor_own", "k_sf_chunks_own", "k_sf_hist_own", "k_sf_own_records")
# (VGPRs, TotalSGPRs) at commit 96c6094 "Per-segment statistics of caller-supplied point attributes on the device"
PARENT = {
    "segfield.hip": {"k_sf_anchor": (12, 23), "k_sf_chunks": (53, 46), "k_sf_final": (32, 26), "k_sf_hist": (10, 37), "k_sf_majority": (12, 20)},
    "segdesc.hip": {"k_sd_keys": (8, 15), "k_sd_runlen": (8, 18), "k_sd_segments": (10, 20), "k_sd_chunks": (55, 34), "k_sd_chunks_own": (59, 38),
                    "k_sd_own_anchor": (16, 30), "k_sd_final": (70, 42), "k_sd_own_records": (80, 30), "k_sd_algebra": (64, 34)},
}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return {src: _usage(src, tmp_path_factory.mktemp(src.split(".")[0])) for src in PARENT}


def _kernel(usage, name):
    """the usage record of kernel `name`: its mangled name holds the length-prefixed identifier, so k_sf_chunks does not match ..._own"""
    hits = [u for n, u in usage.items() if f"{len(name)}{name}" in n]
    assert len(hits) == 1, (name, sorted(usage))
    return hits[0]


def test_exactly_the_listed_kernels_were_added(usage):
    ours = sorted(n for n in usage["segfield.hip"] if "k_sf_" in n)
    assert len(ours) == len(PARENT["segfield.hip"]) + len(ADDED), ours
    for name in ADDED:
        _kernel(usage["segfield.hip"], name)
    assert len([n for n in usage["segdesc.hip"] if "k_sd_" in n]) == len(PARENT["segdesc.hip"])


@pytest.mark.parametrize("name", ADDED)
def test_added_kernels_have_no_scratch_and_no_spills(usage, name):
    u = _kernel(usage["segfield.hip"], name)
    print(name, u)
    assert u["ScratchSize"] == 0, (name, u)
    assert u["VGPRs Spill"] == 0, (name, u)
    assert u["SGPRs Spill"] == 0, (name, u)


@pytest.mark.parametrize("src,name", [(s, n) for s in sorted(PARENT) for n in sorted(PARENT[s])])
def test_existing_kernels_keep_their_registers(usage, src, name):
    u = _kernel(usage[src], name)
    assert (u["VGPRs"], u["TotalSGPRs"]) == PARENT[src][name], (name, u)
    assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
