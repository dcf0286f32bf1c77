"""Register and scratch budget of the label-graph kernels (csrc/labelgraph.hip), read from the compiler as in test_seggraph_resources.py:
every one of them compiles for gfx950 without scratch and without spilled registers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_lg_iota", "k_lg_node_runs", "k_lg_unused_flags", "k_lg_unused_list", "k_lg_rowsILb0", "k_lg_rowsILb1", "k_lg_gather_keys",
           "k_lg_heads", "k_lg_starts", "k_lg_nchunk", "k_lg_chunks", "k_lg_final")


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
def test_label_graph_kernels_have_no_scratch_and_no_spills(tmp_path):
    k = _usage("labelgraph.hip", tmp_path)
    ours = {n: v for n, v in k.items() if "k_lg_" in n}
    assert sorted(n for n in KERNELS if any(n in m for m in ours)) == sorted(KERNELS), sorted(k)
    assert len(ours) == len(KERNELS), sorted(ours)   # every kernel of the file is named above
    for name, u in ours.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
        assert u["SGPRs Spill"] == 0, (name, u)
