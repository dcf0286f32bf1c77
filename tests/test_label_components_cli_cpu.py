"""Host-only part of the label components' front end: the usage errors of vgs_run's --refined-components / --class-components /
--component-ids (argument parsing only, no device).  Each exits 2 and names the flag that is missing; complete sets pass the parser (the
run then ends on the task file, which does not exist).  The cases of test_point_label_fields_cli_cpu.py keep holding beside them."""
import os
import subprocess

import pytest

from test_segdesc_resources import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
RUN = os.path.join(ROOT, "examples", "vgs_run")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_component_flags_without_their_companions_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    task, out, ids = str(tmp_path / "none.txt"), str(tmp_path / "o.csv"), str(tmp_path / "o.i32")
    cls = ["--class-field", "cls", "--classes", "4"]
    cases = [(["--refined-components", out], b"--refined-components", b"needs --refine"),
             (["--class-components", out, "--classes", "4"], b"--class-components", b"--class-field"),
             (["--class-components", out, "--class-field", "cls"], b"--class-components", b"--classes"),
             (["--class-components", out, "--class-field", "cls", "--classes", "0"], b"--classes", b"1 .. 1024"),
             (["--class-components"], b"--class-components", b"unknown argument"),
             (["--refine", "--refined-components"], b"--refined-components", b"unknown argument"),
             (["--component-ids", ids], b"--component-ids", b"neither"),
             (["--refine", "--component-ids", ids], b"--component-ids", b"neither"),
             (["--refine", "--refined-components", out, "--class-components", out] + cls + ["--component-ids", ids], b"--component-ids", b"both"),
             (["--refine", "--refined-components", out, "--component-ids"], b"--component-ids", b"unknown argument"),
             # the class flags without any consumer still name the voxel-label flag, and now this one
             (["--refine", "--refined-components", out] + cls, b"--class-field", b"--segment-classes"),
             (["--class-field", "cls"], b"--class-components", b"--segment-classes")]
    for args, flag, word in cases:
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and flag in r.stderr and word in r.stderr, (args, r.returncode, r.stderr)
    assert not os.path.exists(out) and not os.path.exists(ids)
    # complete sets pass the parser: the run stops at the task file
    for args in (["--refine", "--refined-components", out], ["--refine", "--refined-components", out, "--component-ids", ids],
                 ["--class-components", out] + cls, ["--class-components", out, "--component-ids", ids] + cls,
                 ["--refine", "--refined-components", out, "--class-components", out] + cls):
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and b"not a task file" in r.stderr, (args, r.returncode, r.stderr)
    # a PLY input cannot carry the class field: refused before the cloud is loaded (the file does not exist)
    stock = os.path.join(ROOT, "tests", "golden", "task_vgs_stock.txt")
    r = subprocess.run([RUN, stock, "--in", str(tmp_path / "none.ply"), "--class-components", out] + cls, capture_output=True)
    assert r.returncode == 2 and b"PCD input" in r.stderr and b"--class-components" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out)
    r = subprocess.run([RUN], capture_output=True)   # the usage text names the new flags
    assert r.returncode == 2 and all(w in r.stderr for w in (b"--refined-components", b"--class-components", b"--component-ids"))
