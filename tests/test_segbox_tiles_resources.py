"""Register and scratch budget of what the tiled boxes add to csrc/segbox.hip, read from the compiler as in test_segdesc_resources.py:
  * k_sb_chunks_own, the own-point form of the chunk kernel (the only kernel added), has no scratch and no spilled registers on gfx950;
  * k_sb_frames, k_sb_chunks and k_sb_final keep the VGPR and SGPR counts they had before the chunk body became a template over OWN --
    the single-engine instantiation compiles to what it compiled to at commit 739d73c, where these figures were read."""
import os

import pytest

from test_segdesc_resources import HIPCC, _usage

ADDED = ("k_sb_chunks_own",)
# (VGPRs, TotalSGPRs) of segbox.hip at commit 739d73c "Oriented bounding boxes of the kept segments, computed on the device"
PARENT = {"k_sb_frames": (24, 14), "k_sb_chunks": (36, 49), "k_sb_final": (60, 26)}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _usage("segbox.hip", tmp_path_factory.mktemp("segbox"))


def _kernel(usage, name):
    """the usage record of kernel `name`: its mangled name holds the length-prefixed identifier, so k_sb_chunks does not match ..._own"""
    hits = [u for n, u in usage.items() if f"{len(name)}{name}" in n]
    assert len(hits) == 1, (name, sorted(usage))
    return hits[0]


def test_no_kernel_beyond_the_own_point_chunks_was_added(usage):
    ours = sorted(n for n in usage if "k_sb_" in n)
    assert len(ours) == len(PARENT) + len(ADDED), ours


@pytest.mark.parametrize("name", ADDED)
def test_added_kernels_have_no_scratch_and_no_spills(usage, name):
    u = _kernel(usage, name)
    print(name, u)
    assert u["ScratchSize"] == 0, (name, u)
    assert u["VGPRs Spill"] == 0, (name, u)
    assert u["SGPRs Spill"] == 0, (name, u)


@pytest.mark.parametrize("name", sorted(PARENT))
def test_single_engine_kernels_keep_their_registers(usage, name):
    u = _kernel(usage, name)
    assert (u["VGPRs"], u["TotalSGPRs"]) == PARENT[name], (name, u)
    assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
