"""Host-only part of the refined attribute tables' front end: the usage errors of vgs_run's --refined-segment-fields /
--refined-segment-classes (argument parsing only, no device).  Each exits 2 and names the flag that is missing; --fields / --class-field /
--classes given with a refined file alone pass the parser (the run then ends on the task file, which does not exist).  The cases of
test_segment_fields_cli_cpu.py keep holding beside them."""
import os
import subprocess

import pytest

from test_segdesc_resources import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
RUN = os.path.join(ROOT, "examples", "vgs_run")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refined_attribute_flags_without_their_companions_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    task, out = str(tmp_path / "none.txt"), str(tmp_path / "o.csv")
    cases = [(["--refined-segment-fields", out, "--fields", "intensity"], b"--refined-segment-fields", b"need --refine"),
             (["--refined-segment-classes", out, "--class-field", "cls", "--classes", "4"], b"--refined-segment-classes", b"need --refine"),
             (["--segment-fields", out, "--refined-segment-fields", out, "--fields", "intensity"], b"--refined-segment-fields", b"need --refine"),
             (["--refine", "--refined-segment-fields", out], b"--refined-segment-fields", b"--fields"),
             (["--refine", "--refined-segment-fields", out, "--fields", ","], b"--refined-segment-fields", b"--fields"),
             (["--refine", "--refined-segment-classes", out, "--classes", "4"], b"--refined-segment-classes", b"--class-field"),
             (["--refine", "--refined-segment-classes", out, "--class-field", "cls"], b"--refined-segment-classes", b"--classes"),
             (["--refine", "--refined-segment-classes", out, "--class-field", "cls", "--classes", "0"], b"--classes", b"1 .. 1024"),
             (["--refine", "--refined-segment-classes", out, "--class-field", "cls", "--classes", "1025"], b"--classes", b"1 .. 1024"),
             (["--refine", "--refined-segment-fields", out, "--fields", ",".join(f"f{i}" for i in range(65))], b"--fields", b"at most 64"),
             (["--refine", "--refined-segment-fields"], b"--refined-segment-fields", b"unknown argument"),
             # the old rule: the attribute flags without any consumer still name the voxel-label flag
             (["--refine", "--fields", "intensity"], b"--fields", b"--segment-fields"),
             (["--refine", "--class-field", "cls"], b"--class-field", b"--segment-classes"),
             (["--refine", "--classes", "4"], b"--classes", b"--segment-classes")]
    for args, flag, word in cases:
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and flag in r.stderr and word in r.stderr, (args, r.returncode, r.stderr)
    assert not os.path.exists(out)
    # given only with a refined file the three flags are accepted: the parser passes and the run stops at the task file
    for args in (["--refine", "--refined-segment-fields", out, "--fields", "intensity,z"],
                 ["--refine", "--refined-segment-classes", out, "--class-field", "cls", "--classes", "4"]):
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and b"not a task file" in r.stderr, (args, r.returncode, r.stderr)
    # a PLY input cannot carry the fields: refused before the cloud is loaded (the file does not exist)
    stock = os.path.join(ROOT, "tests", "golden", "task_vgs_stock.txt")
    for args, flag in ((["--refined-segment-fields", out, "--fields", "intensity"], b"--refined-segment-fields"),
                       (["--refined-segment-classes", out, "--class-field", "cls", "--classes", "4"], b"--refined-segment-classes")):
        r = subprocess.run([RUN, stock, "--in", str(tmp_path / "none.ply"), "--refine"] + args, capture_output=True)
        assert r.returncode == 2 and b"PCD input" in r.stderr and flag in r.stderr, (args, r.returncode, r.stderr)
    assert not os.path.exists(out)
    r = subprocess.run([RUN], capture_output=True)   # the usage text names the new flags
    assert r.returncode == 2 and b"--refined-segment-fields" in r.stderr and b"--refined-segment-classes" in r.stderr
