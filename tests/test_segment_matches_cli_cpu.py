"""Host-only parts of the label-comparison front end: the usage errors of vgs_run's --segment-matches / --truth-field / --truth-matches
(argument parsing only, no device), and read_pcd_field_int32 of include/point_clouds_io.hpp through a small stand-alone program, over
files written by pcd.write_pcd in all three DATA layouts: a U 4 field with values above 2^24 (which a float cannot hold), an I 4 field with
negative values, a U 1 field and a float field of whole numbers; and the values it must refuse instead of rounding."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
RUN = os.path.join(ROOT, "examples", "vgs_run")
MODES = ["ascii", "binary", "binary_compressed"]

PROGRAM = r"""
#include <cstdio>
#include "point_clouds_io.hpp"
// usage: prog <file.pcd> <field>: the values of read_pcd_field_int32, one per line; status 3 and the message on a reader error
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<int32_t> out;
  std::string err;
  if (vgs_io::read_pcd_field_int32(argv[1], argv[2], out, err) != 0) { std::fprintf(stderr, "%s\n", err.c_str()); return 3; }
  std::printf("%zu\n", out.size());
  for (int32_t v : out) std::printf("%d\n", (int)v);
  return 0;
}
"""


def test_match_flags_without_their_companions_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    task, out = str(tmp_path / "none.txt"), str(tmp_path / "o.csv")
    cases = [(["--segment-matches", out], b"--truth-field"),
             (["--segment-matches", out, "--truth-matches", out], b"--truth-field"),
             (["--truth-field", "instance"], b"--segment-matches"),
             (["--truth-matches", out], b"--segment-matches"),
             (["--truth-field", "instance", "--truth-matches", out], b"--segment-matches"),
             (["--segment-matches"], b"unknown argument"), (["--truth-field"], b"unknown argument")]
    for args, word in cases:
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
    # a PLY input cannot carry the field: refused before the cloud is loaded (the file does not exist)
    r = subprocess.run([RUN, os.path.join(ROOT, "tests", "golden", "task_vgs_stock.txt"), "--in", str(tmp_path / "none.ply"), "--segment-matches", out,
                        "--truth-field", "instance"], capture_output=True)
    assert r.returncode == 2 and b"PCD input" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out)
    r = subprocess.run([RUN], capture_output=True)
    assert r.returncode == 2 and b"--segment-matches" in r.stderr and b"--truth-field" in r.stderr


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcd_int_field")
    (d / "prog.cpp").write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(d / "prog.cpp"), "-o", str(d / "prog")])
    return str(d / "prog")


def _read(reader, path, field):
    r = subprocess.run([reader, str(path), field], capture_output=True, text=True)
    if r.returncode != 0:
        return r.returncode, r.stderr
    lines = r.stdout.split()
    assert int(lines[0]) == len(lines) - 1
    return 0, np.array(lines[1:], dtype=np.int64)


@pytest.mark.parametrize("mode", MODES)
def test_read_pcd_field_int32_is_exact(vgs, reader, tmp_path, mode):
    rng = np.random.default_rng(5)
    n = 500
    xyz = rng.normal(0, 5, (n, 3)).astype(np.float32)
    inst = rng.integers(0, 2**31, n).astype(np.uint32)
    inst[:4] = (2**24 + 1, 2**31 - 1, 0, 16777217 + 2)           # odd values above 2^24: float32 would round every one of them
    assert (inst.astype(np.float32).astype(np.int64) != inst.astype(np.int64)).sum() > n // 2
    signed = rng.integers(-2**31, 2**31, n).astype(np.int32)
    signed[:3] = (-1, -2**31, 2**31 - 1)
    small = rng.integers(0, 256, n).astype(np.uint8)
    whole = rng.integers(-1000, 1000, n).astype(np.float32)
    path = tmp_path / "in.pcd"
    vgs.pcd.write_pcd(path, xyz, mode=mode, extra={"instance": inst, "signed": signed, "small": small, "whole": whole},
                      field_order=["small", "x", "instance", "y", "whole", "z", "signed"])
    for name, want in (("instance", inst), ("signed", signed), ("small", small), ("whole", whole)):
        rc, got = _read(reader, path, name)
        assert rc == 0, got
        assert np.array_equal(got, want.astype(np.int64)), name
    rc, msg = _read(reader, path, "truth")
    assert rc == 3 and "truth" in msg


@pytest.mark.parametrize("mode", MODES)
def test_read_pcd_field_int32_refuses_what_it_cannot_hold(vgs, reader, tmp_path, mode):
    n = 40
    xyz = np.zeros((n, 3), np.float32)
    big = np.arange(n, dtype=np.uint32)
    big[17] = 2**31                                               # one past INT32_MAX
    frac = np.arange(n, dtype=np.float32)
    frac[23] = 7.5
    nan = np.arange(n, dtype=np.float32)
    nan[5] = np.nan
    huge = np.arange(n, dtype=np.float32)
    huge[9] = 3e9
    path = tmp_path / "bad.pcd"
    vgs.pcd.write_pcd(path, xyz, mode=mode, extra={"big": big, "frac": frac, "nan": nan, "huge": huge})
    for name, at in (("big", 17), ("frac", 23), ("nan", 5), ("huge", 9)):
        rc, msg = _read(reader, path, name)
        assert rc == 3 and f"point {at} " in msg and f"'{name}'" in msg and "int32" in msg, (name, rc, msg)
    rc, got = _read(reader, path, "x")
    assert rc == 0 and not got.any()
