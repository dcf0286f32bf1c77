"""Host-only part of the tiled front end's refinement options (examples/vgs_tiles_run --refine [--patch-radius r] [--switch-ratio s]
[--no-fill]): --patch-radius, --switch-ratio and --no-fill without --refine, and values out of range -- a negative, non-finite or
malformed radius, a ratio outside [0, 1] -- end with status 2 and a message that names the option, before anything touches a device or a
collective and without an output file, the way test_tiles_segment_matches_cli_cpu.py covers the scoring options."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")


def _run(args):
    return subprocess.run([EXE, "--emulate", "2x1"] + args, capture_output=True, timeout=60)


def _points(tmp_path):
    prefix = str(tmp_path / "t")
    for r in range(2):
        np.zeros((30, 3), np.float32).tofile(f"{prefix}.{r}.f32")
    return prefix


def _no_output(prefix):
    return not any(os.path.exists(f"{prefix}.{r}.{s}") for r in range(2) for s in ("labels.i32", "refined.i32"))


@pytest.mark.parametrize("opts", [["--patch-radius", "0.1"], ["--switch-ratio", "0.5"], ["--no-fill"], ["--no-fill", "--patch-radius", "0.1"]],
                         ids=["patch-radius", "switch-ratio", "no-fill", "two"])
def test_refine_options_need_refine(tmp_path, opts):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = _points(tmp_path)
    r = _run(opts + [prefix])
    assert r.returncode == 2 and b"need --refine" in r.stderr, (r.returncode, r.stderr)
    assert _no_output(prefix)


@pytest.mark.parametrize("opt,value", [("--patch-radius", "-0.1"), ("--patch-radius", "inf"), ("--patch-radius", "nan"), ("--patch-radius", "0.1x"),
                                       ("--patch-radius", ""), ("--switch-ratio", "-0.01"), ("--switch-ratio", "1.01"), ("--switch-ratio", "nan"),
                                       ("--switch-ratio", "half")])
def test_refine_values_out_of_range_are_usage_errors(tmp_path, opt, value):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = _points(tmp_path)
    r = _run(["--refine", opt, value, prefix])
    assert r.returncode == 2 and opt.encode() in r.stderr, (r.returncode, r.stderr)
    assert (b"not negative" if opt == "--patch-radius" else b"[0, 1]") in r.stderr, r.stderr
    assert _no_output(prefix)
