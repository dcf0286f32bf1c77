"""Host-only part of the tiled front end's attribute options (examples/vgs_tiles_run --segment-fields / --segment-classes): the usage
errors -- a missing companion option, a value out of range, an attribute file whose size does not match the rank's points -- end with
status 2 before anything touches a device or a collective, the way test_segment_fields_cli_cpu.py covers vgs_run."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")


def _run(args):
    return subprocess.run([EXE, "--emulate", "2x1"] + args, capture_output=True, timeout=60)


def test_attribute_flags_without_their_companions_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix, out = str(tmp_path / "none"), str(tmp_path / "o.csv")
    cases = [(["--segment-fields", out], b"--field-channels"), (["--field-channels", "3"], b"--segment-fields"),
             (["--segment-fields", out, "--field-channels", "0"], b"1 .. 64"), (["--segment-fields", out, "--field-channels", "65"], b"1 .. 64"),
             (["--segment-classes", out], b"--classes"), (["--classes", "4"], b"--segment-classes"),
             (["--segment-classes", out, "--classes", "0"], b"1 .. 1024"), (["--segment-classes", out, "--classes", "1025"], b"1 .. 1024")]
    for args, word in cases:
        r = _run(args + [prefix])
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
    assert not os.path.exists(out)


def test_attribute_files_that_do_not_match_the_points_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix, out = str(tmp_path / "t"), str(tmp_path / "o.csv")
    n = [40, 25]
    for r in range(2):
        np.zeros((n[r], 3), np.float32).tofile(f"{prefix}.{r}.f32")
        np.zeros((n[r], 2), np.float32).tofile(f"{prefix}.{r}.fields.f32")
        np.zeros(n[r], np.int32).tofile(f"{prefix}.{r}.classes.i32")
    # rank 1's files are one row short / one row long; rank 0's are right
    np.zeros((n[1] - 1, 2), np.float32).tofile(f"{prefix}.1.fields.f32")
    r = _run(["--segment-fields", out, "--field-channels", "2", prefix])
    assert r.returncode == 2 and b".1.fields.f32" in r.stderr and b"25 points" in r.stderr, (r.returncode, r.stderr)
    r = _run(["--segment-fields", out, "--field-channels", "3", prefix])            # the right rows, the wrong channel count: rank 0 already
    assert r.returncode == 2 and b".0.fields.f32" in r.stderr, (r.returncode, r.stderr)
    np.zeros(n[1] + 1, np.int32).tofile(f"{prefix}.1.classes.i32")
    r = _run(["--segment-classes", out, "--classes", "4", prefix])
    assert r.returncode == 2 and b".1.classes.i32" in r.stderr, (r.returncode, r.stderr)
    os.remove(f"{prefix}.0.classes.i32")                                            # a missing file is a mismatch as well
    r = _run(["--segment-classes", out, "--classes", "4", prefix])
    assert r.returncode == 2 and b".0.classes.i32" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out) and not os.path.exists(f"{prefix}.0.labels.i32")
