"""Host-only parts of the refined-table front end: the usage errors of vgs_run's --refined-segments / --refined-segment-boxes /
--refined-matches / --refined-truth-matches (argument parsing only, no device), and the CSV writers of examples/segments_csv.hpp, which
the new files share with the voxel-label tables, over a hand-made table through a small stand-alone program: every double written as
%.17g and every float as %.9g reads back to the bit -- an empty label's infinite box, signed zeros, denormals and 2^53 + 1 neighbours
included."""
import os
import subprocess

import numpy as np
import pytest

from test_segdesc_resources import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
RUN = os.path.join(ROOT, "examples", "vgs_run")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "segments_csv.hpp"
// usage: prog <dir>: a hand-made table of three rows through the four writers, and the same numbers as raw bytes in <dir>/raw.bin
// (per row: 29 doubles of the segments file, then 22 of the boxes file, then 6 of each match file)
static const double D[] = {0.1, -1.0 / 3.0, 4.9406564584124654e-324, 1.7976931348623157e308, -0.0, 9007199254740993.0, 2.2250738585072014e-308,
                           6.02214076e23, -299792.458, 1e-17, 0.30000000000000004, 123456789.12345679};
static const float F[] = {0.1f, -1.0f / 3.0f, 1.4e-45f, 3.4028235e38f, -0.0f, 16777217.0f, 1.17549435e-38f, 2.5f, -7.125f, 1e-9f};
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  std::vector<pcl::ClusterDescriptor> desc(3);
  std::vector<pcl::ClusterBox> boxes(3);
  pcl::ClusterLabelComparison m;
  std::vector<double> raw;
  int d = 0, f = 0;
  auto nd = [&]() { const double v = D[d % 12]; ++d; return v * (double)(1 + d % 5); };
  auto nf = [&]() { const float v = F[f % 10]; ++f; return v * (float)(1 + f % 3); };
  for (int i = 0; i < 3; ++i) {
    pcl::ClusterDescriptor& s = desc[i];
    s.n_points = i == 1 ? 0 : 4000000000LL + i; s.n_nodes = i == 1 ? 0 : 2147483647 - i;
    for (int a = 0; a < 6; ++a) s.bbox[a] = i == 1 ? (a < 3 ? HUGE_VALF : -HUGE_VALF) : nf();
    for (int a = 0; a < 3; ++a) { s.centroid[a] = i == 1 ? 0.0 : nd(); s.evals[a] = i == 1 ? 0.0 : nd(); }
    for (int a = 0; a < 9; ++a) s.evecs[a] = i == 1 ? (a % 4 == 0 ? 1.0 : 0.0) : nd();
    for (int a = 0; a < 8; ++a) s.eigen8[a] = i == 1 ? 0.0f : nf();
    raw.push_back(i); raw.push_back((double)s.n_points); raw.push_back(s.n_nodes);
    for (int a = 0; a < 6; ++a) raw.push_back(s.bbox[a]);
    for (int a = 0; a < 3; ++a) raw.push_back(s.centroid[a]);
    for (int a = 0; a < 3; ++a) raw.push_back(s.evals[a]);
    for (int r = 0; r < 3; ++r) raw.push_back(s.evecs[3 * r]);
    for (int r = 0; r < 3; ++r) raw.push_back(s.evecs[3 * r + 2]);
    for (int a = 0; a < 8; ++a) raw.push_back(s.eigen8[a]);
    pcl::ClusterBox& b = boxes[i];
    raw.push_back(i);
    for (int a = 0; a < 3; ++a) raw.push_back(b.center[a] = nd());
    for (int a = 0; a < 3; ++a) raw.push_back(b.half[a] = i == 1 ? 0.0 : nd());
    for (int a = 0; a < 9; ++a) raw.push_back(b.frame[a] = nd());
    for (int a = 0; a < 3; ++a) raw.push_back(b.lo[a] = i == 1 ? -0.0 : nd());
    for (int a = 0; a < 3; ++a) raw.push_back(b.hi[a] = i == 1 ? 0.0 : nd());
    m.seg_annotated.push_back(3000000000LL * i); m.seg_refs.push_back(7 - i); m.seg_best_ref.push_back(i == 1 ? -1 : 2147483647);
    m.seg_best_n.push_back(2999999999LL * i); m.seg_best_iou.push_back(i == 1 ? 0.0 : nd());
    raw.push_back(i); raw.push_back((double)m.seg_annotated[i]); raw.push_back(m.seg_refs[i]); raw.push_back(m.seg_best_ref[i]);
    raw.push_back((double)m.seg_best_n[i]); raw.push_back(m.seg_best_iou[i]);
    m.ref_id.push_back(i * 1000000000); m.ref_points.push_back(5000000000LL + i); m.ref_dropped.push_back(i);
    m.ref_best_seg.push_back(i - 1); m.ref_best_n.push_back(4999999999LL * i); m.ref_best_iou.push_back(nd());
    raw.push_back(m.ref_id[i]); raw.push_back((double)m.ref_points[i]); raw.push_back((double)m.ref_dropped[i]); raw.push_back(m.ref_best_seg[i]);
    raw.push_back((double)m.ref_best_n[i]); raw.push_back(m.ref_best_iou[i]);
  }
  if (writeSegmentsCsv(dir + "/segments.csv", desc) || writeBoxesCsv(dir + "/boxes.csv", boxes) || writeSegmentMatchesCsv(dir + "/matches.csv", m) ||
      writeTruthMatchesCsv(dir + "/truth.csv", m)) return 3;
  FILE* o = std::fopen((dir + "/raw.bin").c_str(), "wb");
  if (!o || std::fwrite(raw.data(), sizeof(double), raw.size(), o) != raw.size() || std::fclose(o) != 0) return 4;
  return 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refined_flags_without_their_companions_are_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    task, out = str(tmp_path / "none.txt"), str(tmp_path / "o.csv")
    cases = [(["--refined-segments", out], b"need --refine"),
             (["--refined-segment-boxes", out], b"need --refine"),
             (["--refined-segment-boxes", out, "--box-frame", "upright"], b"need --refine"),
             (["--refined-matches", out, "--truth-field", "instance"], b"need --refine"),
             (["--refined-matches", out, "--truth-field", "instance", "--refined-truth-matches", out], b"need --refine"),
             (["--refined-truth-matches", out], b"need --refine"),
             (["--segments", out, "--refined-segments", out], b"need --refine"),
             (["--refine", "--refined-matches", out], b"--truth-field"),
             (["--refine", "--refined-matches", out, "--refined-truth-matches", out], b"--truth-field"),
             (["--refine", "--refined-truth-matches", out], b"--refined-matches"),
             (["--refine", "--refined-truth-matches", out, "--truth-field", "instance"], b"--refined-matches"),
             (["--refine", "--truth-field", "instance"], b"--segment-matches"),
             (["--refine", "--refined-matches", out, "--truth-field", "instance", "--truth-matches", out], b"--segment-matches"),
             (["--refine", "--refined-segments"], b"unknown argument"), (["--refined-matches"], b"unknown argument")]
    for args, word in cases:
        r = subprocess.run([RUN, task] + args, capture_output=True)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
    assert not os.path.exists(out)
    # a PLY input cannot carry the truth field: refused before the cloud is loaded (the file does not exist)
    r = subprocess.run([RUN, os.path.join(ROOT, "tests", "golden", "task_vgs_stock.txt"), "--in", str(tmp_path / "none.ply"), "--refine",
                        "--refined-matches", out, "--truth-field", "instance"], capture_output=True)
    assert r.returncode == 2 and b"PCD input" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([RUN], capture_output=True)   # the usage text names the new flags
    assert r.returncode == 2
    for flag in (b"--refined-segments", b"--refined-segment-boxes", b"--refined-matches", b"--refined-truth-matches"):
        assert flag in r.stderr, flag


def test_csv_writers_round_trip_a_hand_made_table(tmp_path):
    (tmp_path / "prog.cpp").write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "examples"),
                           str(tmp_path / "prog.cpp"), "-o", str(tmp_path / "prog")])
    subprocess.check_call([str(tmp_path / "prog"), str(tmp_path)])
    raw = np.fromfile(tmp_path / "raw.bin", dtype=np.float64).reshape(3, 29 + 22 + 6 + 6)
    parts = {"segments": (raw[:, :29], 29), "boxes": (raw[:, 29:51], 22), "matches": (raw[:, 51:57], 6), "truth": (raw[:, 57:63], 6)}
    for name, (want, width) in parts.items():
        with open(tmp_path / (name + ".csv")) as f:
            assert len(f.readline().strip().split(",")) == width, name
        got = np.loadtxt(tmp_path / (name + ".csv"), delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
        assert got.shape == want.shape, name
        if name == "segments":   # the float columns read back as the floats that were written, the rest as the doubles
            fcols = list(range(3, 9)) + list(range(21, 29))
            assert got[:, fcols].astype(np.float32).tobytes() == want[:, fcols].astype(np.float32).tobytes()
            dcols = [c for c in range(29) if c not in fcols]
            assert got[:, dcols].tobytes() == want[:, dcols].tobytes()
        else:
            assert got.tobytes() == want.tobytes(), name
    seg = raw[:, :29]
    assert (seg[1, 3:6] == np.inf).all() and (seg[1, 6:9] == -np.inf).all()        # the empty label's box went through
    assert np.signbit(raw[1, 29 + 16:29 + 19]).all() and not np.signbit(raw[1, 29 + 19:29 + 22]).any()   # and so did -0.0
