"""Host-only part of the absorb step's front end: the usage errors of vgs_run's --absorbed-labels / --absorb-islands /
--absorb-min-points / --absorb-rounds / --absorb-drop (argument parsing only, no device), in the manner of
test_label_components_cli_cpu.py.  Each exits 2 and names the flag that is missing; complete sets pass the parser (the run then ends on the
task file, which does not exist)."""
import os
import subprocess

import pytest

from test_label_components_cli_cpu import CSRC, HIPCC, ROOT, RUN


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_absorb_flags_without_their_companions_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    task, out, csv = str(tmp_path / "none.txt"), str(tmp_path / "o.i32"), str(tmp_path / "o.csv")
    cls = ["--class-field", "cls", "--classes", "4"]
    isl, mnp = ["--absorb-islands", "50"], ["--absorb-min-points", "20"]
    cases = [(["--absorbed-labels", out] + isl, b"--absorbed-labels", b"neither"),                      # no source
             (["--absorbed-labels", out, "--refine"] + cls + isl, b"--absorbed-labels", b"both"),       # two sources
             (["--absorbed-labels", out, "--refine", "--classes", "4"] + isl, b"--absorbed-labels", b"both"),
             (["--absorbed-labels", out, "--class-field", "cls"] + isl, b"--absorbed-labels", b"--classes"),
             (["--absorbed-labels", out, "--classes", "4"] + isl, b"--absorbed-labels", b"--class-field"),
             (["--absorbed-labels", out, "--refine"], b"--absorbed-labels", b"--absorb-islands"),        # no threshold
             (["--absorbed-labels", out, "--refine", "--absorb-rounds", "3", "--absorb-drop"], b"--absorbed-labels", b"--absorb-min-points"),
             (["--absorbed-labels", out] + cls, b"--absorbed-labels", b"--absorb-islands"),
             (["--refine"] + isl, b"--absorb-islands", b"--absorbed-labels"),                            # the options without the file
             (["--refine"] + mnp, b"--absorb-min-points", b"--absorbed-labels"),
             (["--refine", "--absorb-rounds", "2"], b"--absorb-rounds", b"--absorbed-labels"),
             (["--refine", "--absorb-drop"], b"--absorb-drop", b"--absorbed-labels"),
             (["--absorbed-labels", out, "--refine", "--absorb-islands", "-1"], b"--absorb-islands -1", b"not negative"),
             (["--absorbed-labels", out, "--refine", "--absorb-min-points", "x"], b"--absorb-min-points x", b"not negative"),
             (["--absorbed-labels", out, "--refine", "--absorb-rounds", "65"] + isl, b"--absorb-rounds 65", b"0 .. 64"),
             (["--refine", "--absorbed-labels"], b"--absorbed-labels", b"unknown argument"),
             (["--absorbed-labels", out, "--refine", "--absorb-islands"], b"--absorb-islands", b"unknown argument"),
             # the class flags without any consumer still name the voxel-label flag, and now this one
             (["--class-field", "cls"], b"--absorbed-labels", b"--segment-classes")]
    for args, flag, word in cases:
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and flag in r.stderr and word in r.stderr, (args, r.returncode, r.stderr)
    assert not os.path.exists(out)
    # complete sets pass the parser: the run stops at the task file
    for args in (["--refine", "--absorbed-labels", out] + isl, ["--refine", "--absorbed-labels", out] + mnp,
                 ["--refine", "--absorbed-labels", out, "--absorb-rounds", "0", "--absorb-drop"] + isl + mnp,
                 ["--absorbed-labels", out] + cls + isl, ["--absorbed-labels", out, "--absorb-rounds", "64"] + cls + mnp,
                 ["--absorbed-labels", out, "--class-components", csv, "--class-graph", csv] + cls + isl,
                 ["--refine", "--refined-components", csv, "--refined-graph", csv, "--absorbed-labels", out] + isl):
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and b"not a task file" in r.stderr, (args, r.returncode, r.stderr)
    # a PLY input cannot carry the class field: refused before the cloud is loaded (the file does not exist)
    stock = os.path.join(ROOT, "tests", "golden", "task_vgs_stock.txt")
    r = subprocess.run([RUN, stock, "--in", str(tmp_path / "none.ply"), "--absorbed-labels", out] + cls + isl, capture_output=True)
    assert r.returncode == 2 and b"PCD input" in r.stderr and b"--absorbed-labels" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out)
    r = subprocess.run([RUN], capture_output=True)   # the usage text names the new flags
    assert r.returncode == 2 and all(w in r.stderr for w in (b"--absorbed-labels", b"--absorb-islands", b"--absorb-min-points", b"--absorb-rounds",
                                                             b"--absorb-drop"))
