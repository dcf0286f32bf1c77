"""Host-only parts of the segment-attribute front end: the usage errors of vgs_run's --segment-fields / --segment-classes (argument
parsing only, no device), and read_pcd_fields of include/point_clouds_io.hpp through a small stand-alone program, over files written by
pcd.write_pcd in all three DATA layouts with a float field, a U 1 field and a U 2 field."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
RUN = os.path.join(ROOT, "examples", "vgs_run")

PROGRAM = r"""
#include <cstdio>
#include "point_clouds_io.hpp"
// usage: prog <file.pcd> <field> [<field> ...]: the rows of read_pcd_fields as %.9g, then the points of read_pcd_xyz; status 3 and the
// message on a reader error
int main(int argc, char** argv) {
  std::vector<std::string> names;
  for (int a = 2; a < argc; ++a) names.push_back(argv[a]);
  std::vector<float> out;
  std::string err;
  if (vgs_io::read_pcd_fields(argv[1], names, out, err) != 0) { std::fprintf(stderr, "%s\n", err.c_str()); return 3; }
  const size_t C = names.size(), n = C ? out.size() / C : 0;
  std::printf("%zu %zu\n", n, C);
  for (size_t i = 0; i < n; ++i) {
    for (size_t c = 0; c < C; ++c) std::printf(c ? " %.9g" : "%.9g", (double)out[i * C + c]);
    std::printf("\n");
  }
  std::vector<pcl::PointXYZ> pts;
  uint32_t w = 0, h = 0;
  if (vgs_io::read_pcd_xyz(argv[1], pts, &w, &h, err) != 0) { std::fprintf(stderr, "%s\n", err.c_str()); return 3; }
  for (const auto& p : pts) std::printf("%.9g %.9g %.9g\n", (double)p.x, (double)p.y, (double)p.z);
  return 0;
}
"""


def test_segment_flags_without_their_companions_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    task, out = str(tmp_path / "none.txt"), str(tmp_path / "o.csv")
    cases = [(["--segment-fields", out], b"--fields"),
             (["--segment-classes", out, "--classes", "4"], b"--class-field"),
             (["--segment-classes", out, "--class-field", "cls"], b"--classes"),
             (["--segment-classes", out, "--class-field", "cls", "--classes", "0"], b"1 .. 1024"),
             (["--segment-classes", out, "--class-field", "cls", "--classes", "1025"], b"1 .. 1024"),
             (["--fields", "intensity"], b"--segment-fields"), (["--class-field", "cls"], b"--segment-classes"),
             (["--classes", "4"], b"--segment-classes")]
    for args, word in cases:
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
    # a PLY input cannot carry the fields: refused before the cloud is loaded (the file does not exist)
    r = subprocess.run([RUN, os.path.join(ROOT, "tests", "golden", "task_vgs_stock.txt"), "--in", str(tmp_path / "none.ply"), "--segment-fields", out,
                        "--fields", "intensity"], capture_output=True)
    assert r.returncode == 2 and b"PCD input" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out)


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcd_fields")
    (d / "prog.cpp").write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(d / "prog.cpp"), "-o", str(d / "prog")])
    return str(d / "prog")


@pytest.mark.parametrize("mode", ["ascii", "binary", "binary_compressed"])
def test_read_pcd_fields(vgs, reader, tmp_path, mode):
    rng = np.random.default_rng(3)
    n = 700
    xyz = rng.normal(0, 5, (n, 3)).astype(np.float32)
    inten = rng.uniform(0, 1, n).astype(np.float32)
    cls = rng.integers(0, 256, n).astype(np.uint8)
    ring = rng.integers(0, 65536, n).astype(np.uint16)
    ring[:2] = (0, 65535)
    path = tmp_path / "in.pcd"
    vgs.pcd.write_pcd(path, xyz, mode=mode, extra={"intensity": inten, "cls": cls, "ring": ring}, field_order=["cls", "x", "ring", "y", "intensity", "z"])
    r = subprocess.run([reader, str(path), "ring", "intensity", "cls"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].split() == [str(n), "3"] and len(lines) == 1 + 2 * n
    got = np.array([ln.split() for ln in lines[1:1 + n]], dtype=np.float64).astype(np.float32)
    assert np.array_equal(got, np.stack([ring.astype(np.float32), inten, cls.astype(np.float32)], axis=1))
    pts = np.array([ln.split() for ln in lines[1 + n:]], dtype=np.float64).astype(np.float32)
    assert np.array_equal(pts, xyz)                       # read_pcd_xyz goes through the same decoder
    r = subprocess.run([reader, str(path), "intensity", "reflectance"], capture_output=True, text=True)
    assert r.returncode == 3 and "reflectance" in r.stderr and "intensity" not in r.stderr.replace(str(path), "")
