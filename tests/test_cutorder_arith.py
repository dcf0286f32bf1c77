"""The integer arithmetic of csrc/cutorder.hip on the host (csrc/cutorder_arith.h, the same functions the kernel and the driver call):
the pair index p -> (i, j) of k_co_eval -- a double sqrt settled by two loops -- must be the p-th pair in row-major order over i < j for
every p of every k in 2 .. 300 and of the cap, and for the first and last p of every row at k in {2047, 2048, 2049, 4224, 8191, 8192};
the chunk partition must give consecutive chunks that cover every voxel once, stay within the budget unless they hold one voxel, carry
the running sums of k (k - 1) / 2 as offsets (0 for k = 0 and k = 1), and give a voxel above the budget a chunk of its own -- budgets
1, 10 and 2^29, random k.  (No scene of a few seconds reaches 2^29 pairs: the second chunk exists on the host only.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_index_and_chunk_partition(tmp_path):
    exe = tmp_path / "cutorder_check"
    src = os.path.join(ROOT, "tests", "cpp", "cutorder_check.cpp")
    inc = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "bad=0" in out, out
