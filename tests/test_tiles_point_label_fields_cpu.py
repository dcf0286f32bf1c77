"""CPU test of the tiled front end's attribute tables of the refined labels (examples/vgs_tiles_run.cpp): --refined-segment-fields and
--refined-segment-classes without --refine are usage errors -- exit status 2, "need --refine" and the usage text, before any file is
written and before any GPU call; and the companion options keep their rules."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")


def _run(tmp_path, opts):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    return subprocess.run([EXE, "--emulate", "2x1", *opts, str(tmp_path / "t")], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("opts", [["--refined-segment-fields", "a.csv", "--field-channels", "5"], ["--refined-segment-classes", "b.csv", "--classes", "16"],
                                  ["--refined-segment-fields", "a.csv", "--field-channels", "5", "--refined-segment-classes", "b.csv", "--classes", "16"]])
def test_refined_attribute_options_need_refine(tmp_path, opts):
    p = _run(tmp_path, opts)
    assert p.returncode == 2 and "need --refine" in p.stderr and "usage:" in p.stderr, (p.returncode, p.stderr)
    assert "--refined-segment-fields" in p.stderr and "--refined-segment-classes" in p.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("opts,word", [(["--refine", "--refined-segment-fields", "a.csv"], "--refined-segment-fields needs --field-channels"),
                                       (["--refine", "--refined-segment-classes", "b.csv"], "--refined-segment-classes needs --classes"),
                                       (["--field-channels", "5"], "--field-channels needs --segment-fields"),
                                       (["--classes", "16"], "--classes needs --segment-classes"),
                                       (["--refine", "--refined-segment-fields", "a.csv", "--field-channels", "65"], "--field-channels must be in 1 .. 64"),
                                       (["--refine", "--refined-segment-classes", "b.csv", "--classes", "1025"], "--classes must be in 1 .. 1024")])
def test_companion_options(tmp_path, opts, word):
    p = _run(tmp_path, opts)
    assert p.returncode == 2 and word in p.stderr, (p.returncode, p.stderr)
    assert not os.listdir(tmp_path)


def test_missing_attribute_files_are_a_usage_error(tmp_path):
    """--field-channels is satisfied by the refined option alone, and the rank's attribute file is then looked for before any collective"""
    import numpy as np
    np.zeros((10, 3), np.float32).tofile(str(tmp_path / "t.0.f32"))
    np.zeros((10, 3), np.float32).tofile(str(tmp_path / "t.1.f32"))
    before = sorted(os.listdir(tmp_path))
    p = _run(tmp_path, ["--refine", "--refined-segment-fields", str(tmp_path / "a.csv"), "--field-channels", "5"])
    assert p.returncode == 2 and "fields.f32" in p.stderr, (p.returncode, p.stderr)
    assert sorted(os.listdir(tmp_path)) == before
