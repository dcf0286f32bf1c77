"""The kernels that turn the sorted keys into the voxel table (csrc/voxelize.hip), read from the compiler as in test_kernel_resources.py:
the two passes over the keys and the one-workgroup scan between them compile for gfx950, in both key widths, without scratch and without
spilled registers -- and the chain they replace (head flags, a device-wide scan of them, single-thread launches that moved one number
each) is gone from the code object."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# (mangled names: I<j|m>E = the uint32_t / uint64_t instantiation)
KERNELS = ("k_run_countsIjE", "k_run_countsImE", "k_tile_offsets", "k_voxel_runsIjE", "k_voxel_runsImE")
GONE = ("k_heads", "k_voxel_table", "k_count_valid", "k_copy_last", "k_set_u32")


def _usage(src, tmp_path):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "-c", os.path.join(CSRC, src), "-o", str(tmp_path / "dev.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_voxel_run_kernels_have_no_scratch_and_their_predecessors_are_gone(tmp_path):
    k = _usage("voxelize.hip", tmp_path)
    ours = {n: v for n, v in k.items() if any(s in n for s in KERNELS)}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    assert len(ours) == len(KERNELS), sorted(ours)
    for name, u in ours.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
    # the code object itself: its symbol table names the new kernels and nothing of the old chain
    with open(tmp_path / "dev.o", "rb") as f:
        obj = f.read()
    for name in KERNELS:
        assert name.encode() in obj, name
    for old in GONE:
        assert old.encode() not in obj, old
        assert not any(old in n for n in k), old
