"""Host-only part of the tiled front end's scoring options (examples/vgs_tiles_run --segment-matches / --truth-matches): the usage errors
-- --truth-matches without --segment-matches, a truth file that is missing, one whose size does not match the rank's points -- end with
status 2 and the file and the point count named, before anything touches a device or a collective and without an output file, the way
test_tiles_segfields_cli_cpu.py covers the attribute options."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")


def _run(args):
    return subprocess.run([EXE, "--emulate", "2x1"] + args, capture_output=True, timeout=60)


def test_truth_matches_needs_segment_matches(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix, out = str(tmp_path / "none"), str(tmp_path / "truth.csv")
    r = _run(["--truth-matches", out, prefix])
    assert r.returncode == 2 and b"--segment-matches" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out)


def test_truth_files_that_do_not_match_the_points_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix, seg, tru = str(tmp_path / "t"), str(tmp_path / "seg.csv"), str(tmp_path / "truth.csv")
    n = [40, 25]
    for r in range(2):
        np.zeros((n[r], 3), np.float32).tofile(f"{prefix}.{r}.f32")
        np.zeros(n[r], np.int32).tofile(f"{prefix}.{r}.truth.i32")
    args = ["--segment-matches", seg, "--truth-matches", tru, prefix]
    # rank 1's file is one id short, then one id long; rank 0's is right
    for m in (n[1] - 1, n[1] + 1):
        np.zeros(m, np.int32).tofile(f"{prefix}.1.truth.i32")
        r = _run(args)
        assert r.returncode == 2 and b".1.truth.i32" in r.stderr and b"25 points" in r.stderr, (m, r.returncode, r.stderr)
    # a missing file: named with the points it should cover
    np.zeros(n[1], np.int32).tofile(f"{prefix}.1.truth.i32")
    os.remove(f"{prefix}.0.truth.i32")
    r = _run(args)
    assert r.returncode == 2 and b".0.truth.i32" in r.stderr and b"40 points" in r.stderr, (r.returncode, r.stderr)
    r = _run(["--segment-matches", seg, prefix])                                  # ... without --truth-matches as well
    assert r.returncode == 2 and b".0.truth.i32" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(seg) and not os.path.exists(tru) and not os.path.exists(f"{prefix}.0.labels.i32")
