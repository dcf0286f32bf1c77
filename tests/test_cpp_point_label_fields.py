"""getLabelFieldStats / getLabelClassHistogram of include/vgs_segmentation.hpp, on both classes, through a small program built against the
header and the library: the rows of a labelling that splits every cluster inside its voxels (K given) and of refineClusterLabels()' result
(K left to the clusters' range) equal Engine.label_field_stats / label_class_histogram by bytes for the same cloud, parameters and inputs,
n_skipped included; and VoxelBasedSegmentation returns empty tables before drawColorMapofPointsinClusters."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vgs-svgs-segmentation_amd")
CH, N_CLASSES = 3, 6

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "vgs_segmentation.hpp"
// usage: prog <method 2|3> <dir>: reads <dir>/xyz.bin (n x 3 float), field.bin (n x CH float, rows PAD floats apart), cls.bin (n int32);
// segments with the stock parameters; writes <dir>/out.bin: for the labelling 3 * cluster + (i mod 3) (K = 3 * clusters + 1) and for the
// refined labels (K left to its default) the two tables row by row, and <dir>/meta.txt: clusters, the two n_skipped pairs, rows before drawing
static const int CH = %d, PAD = %d, NC = %d;
template <typename T> static std::vector<T> load(const std::string& p) {
  FILE* f = std::fopen(p.c_str(), "rb");
  if (!f) std::exit(5);
  std::fseek(f, 0, SEEK_END);
  const long b = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)b / sizeof(T));
  if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(5);
  std::fclose(f);
  return v;
}
template <typename T> static void put(FILE* o, const T* p, size_t n) { if (std::fwrite(p, sizeof(T), n, o) != n) std::exit(6); }
static void dump(FILE* o, const std::vector<pcl::ClusterFieldStats>& s, const std::vector<pcl::ClusterClassHistogram>& h) {
  for (const auto& r : s) {
    put(o, r.n_valid.data(), r.n_valid.size()); put(o, r.anchor.data(), r.anchor.size()); put(o, r.mean.data(), r.mean.size());
    put(o, r.var.data(), r.var.size()); put(o, r.vmin.data(), r.vmin.size()); put(o, r.vmax.data(), r.vmax.size());
  }
  for (const auto& r : h) {
    put(o, r.hist.data(), r.hist.size()); put(o, &r.n_outside, 1); put(o, &r.majority, 1); put(o, &r.majority_count, 1);
  }
}
template <typename S> static int tables(S& s, const std::string& dir, const std::vector<float>& field, const std::vector<int32_t>& cls, int64_t n,
                                        size_t before) {
  const int64_t kept = (int64_t)s.getClusterIdx().size();
  std::vector<int32_t> own = s.drawColorMapofPointsinClusters(), split((size_t)n);
  for (int64_t i = 0; i < n; ++i) split[i] = own[i] < 0 ? -1 : 3 * own[i] + (int32_t)(i %% 3);
  FILE* o = std::fopen((dir + "/out.bin").c_str(), "wb");
  if (!o) return 6;
  int64_t sk[4] = {-1, -1, -1, -1};
  const int64_t K = 3 * kept + 1;
  dump(o, s.getLabelFieldStats(split.data(), field.data(), n, CH, 4 * PAD, K, &sk[0]), s.getLabelClassHistogram(split.data(), cls.data(), n, NC, K, &sk[1]));
  const std::vector<int32_t> fine = s.refineClusterLabels();
  dump(o, s.getLabelFieldStats(fine.data(), field.data(), n, CH, 4 * PAD, -1, &sk[2]), s.getLabelClassHistogram(fine.data(), cls.data(), n, NC, -1, &sk[3]));
  if (std::fclose(o) != 0) return 6;
  FILE* m = std::fopen((dir + "/meta.txt").c_str(), "w");
  if (!m) return 6;
  std::fprintf(m, "%%lld %%lld %%lld %%lld %%lld %%zu\n", (long long)kept, (long long)sk[0], (long long)sk[1], (long long)sk[2], (long long)sk[3], before);
  return std::fclose(m) == 0 ? 0 : 6;
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int method = std::atoi(argv[1]);
  const std::string dir = argv[2];
  const std::vector<float> xyz = load<float>(dir + "/xyz.bin"), field = load<float>(dir + "/field.bin");
  const std::vector<int32_t> cls = load<int32_t>(dir + "/cls.bin");
  const int64_t n = (int64_t)cls.size();
  PCXYZPtr cloud(new PCXYZ);
  cloud->points.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) { cloud->points[i].x = xyz[3 * i]; cloud->points[i].y = xyz[3 * i + 1]; cloud->points[i].z = xyz[3 * i + 2]; }
  double b[6];
  try {
    if (method == 2) {
      pcl::VoxelBasedSegmentation<pcl::PointXYZ> s(0.15f);
      s.setInputCloud(cloud); s.getCloudPointNum(cloud); s.addPointsFromInputCloud();
      s.setVoxelSize(0.15f, 10, 3, 3);
      s.getBoundingBox(b[0], b[1], b[2], b[3], b[4], b[5]); s.setBoundingBox(b[0], b[1], b[2], b[3], b[4], b[5]);
      s.setVoxelCenters(); s.calcualteVoxelCloudAttributes(cloud); s.findAllVoxelAdjacency(0.5f);
      s.segmentVoxelCloudWithGraphModel(0.3f, 0.2f, 0.2f, 0.2f, 0.2f, 0.2f, 2.0f);
      std::vector<int32_t> zero((size_t)n, 0);   // before drawColorMapofPointsinClusters: empty tables, like getLabelDescriptors
      const size_t before = s.getLabelFieldStats(zero.data(), field.data(), n, CH, 4 * PAD).size() +
                            s.getLabelClassHistogram(zero.data(), cls.data(), n, NC).size();
      s.drawColorMapofPointsinClusters();
      return tables(s, dir, field, cls, n, before);
    }
    pcl::SuperVoxelBasedSegmentation<pcl::PointXYZ> s(0.05f);
    s.setInputCloud(cloud); s.getCloudPointNum(cloud); s.addPointsFromInputCloud();
    s.setVoxelSize(0.05f, 0); s.setSupervoxelSize(0.25f, 3, 0, 3); s.setGraphSize(0.5f, 0.5f);
    s.getBoundingBox(b[0], b[1], b[2], b[3], b[4], b[5]); s.setBoundingBox(b[0], b[1], b[2], b[3], b[4], b[5]);
    s.setSupervoxelCentersCentroids(); s.getVoxelNum();
    s.segmentSupervoxelCloudWithGraphModel(0.0f, 0.25f, 0.75f, 0.5f, 0.2f, 0.2f, 0.2f, 0.2f, 0.75f, 1.0f);
    return tables(s, dir, field, cls, n, 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %%s\n", e.what());
    return 1;
  }
}
"""


def _rows(raw, at, K, spec):
    """K records of (dtype, count) fields from the byte string raw at offset at -> ({index: array (K, count)}, the offset behind them)"""
    dt = np.dtype([(f"f{i}", d, (c,)) for i, (d, c) in enumerate(spec)])
    a = np.frombuffer(raw, dtype=dt, count=K, offset=at)
    return [np.ascontiguousarray(a[f"f{i}"]) for i in range(len(spec))], at + K * dt.itemsize


def _tables(raw, at, K):
    st, at = _rows(raw, at, K, [(np.int64, CH), (np.float64, CH), (np.float64, CH), (np.float64, CH), (np.float32, CH), (np.float32, CH)])
    hi, at = _rows(raw, at, K, [(np.int64, N_CLASSES), (np.int64, 1), (np.int32, 1), (np.int64, 1)])
    return st, [hi[0]] + [h[:, 0] for h in hi[1:]], at


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("cpp_point_label_fields")
    (d / "prog.cpp").write_text(PROGRAM % (CH, CH + 2, N_CLASSES))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(d / "prog.cpp"), "-o", str(d / "prog"),
                           "-L", PKG, "-lvgs_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return str(d / "prog")


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_label_attribute_getters_match_engine(gpu, prog, tmp_path, method):
    xyz = gpu.scenes.town_scene(60_000)
    N = xyz.shape[0]
    rng = np.random.default_rng(41)
    wide = np.full((N, CH + 2), np.float32(np.nan))
    wide[:, :CH] = rng.normal(50.0, 9.0, (N, CH)).astype(np.float32)
    wide[rng.choice(N, 80, replace=False), 1] = np.inf
    field = wide[:, :CH]
    cls = rng.integers(-1, N_CLASSES + 1, N).astype(np.int32)
    xyz.tofile(tmp_path / "xyz.bin"); wide.tofile(tmp_path / "field.bin"); cls.tofile(tmp_path / "cls.bin")
    subprocess.check_call([prog, str(method), str(tmp_path)])
    if method == 2:   # the call sequence of the program, parameter by parameter
        s = gpu.VoxelBasedSegmentation(0.15)
        s.setInputCloud(xyz); s.getCloudPointNum(xyz); s.addPointsFromInputCloud()
        s.setVoxelSize(0.15, 10, 3, 3)
        s.setVoxelCenters(); s.calcualteVoxelCloudAttributes(xyz); s.findAllVoxelAdjacency(0.5)
        s.segmentVoxelCloudWithGraphModel(0.3, 0.2, 0.2, 0.2, 0.2, 0.2, 2.0)
    else:
        s = gpu.SuperVoxelBasedSegmentation(0.05)
        s.setInputCloud(xyz); s.getCloudPointNum(xyz); s.addPointsFromInputCloud()
        s.setVoxelSize(0.05, 0); s.setSupervoxelSize(0.25, 3, 0, 3); s.setGraphSize(0.5, 0.5)
        s.segmentSupervoxelCloudWithGraphModel(0.0, 0.25, 0.75, 0.5, 0.2, 0.2, 0.2, 0.2, 0.75, 1.0)
    own = s.drawColorMapofPointsinClusters()
    eng = s.engine
    kept = eng.counts()["kept"]
    meta = [int(v) for v in open(tmp_path / "meta.txt").read().split()]
    assert meta[0] == kept > 0 and meta[5] == 0
    split = np.where(own >= 0, 3 * own + np.arange(N) % 3, -1).astype(np.int32)
    fine = s.refineClusterLabels()
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for labels, K, sk in ((split, 3 * kept + 1, meta[1:3]), (fine, None, meta[3:5])):
        st, hi = eng.label_field_stats(labels, field, K=K), eng.label_class_histogram(labels, cls, N_CLASSES, K=K)
        assert sk == [st["n_skipped"], hi["n_skipped"]]
        rows = st["mean"].shape[0]
        assert rows == (kept if K is None else K)
        got_st, got_hi, at = _tables(raw, at, rows)
        for (name, _), g in zip(gpu.Engine.FIELD_STAT_FIELDS, got_st):
            assert g.tobytes() == st[name].tobytes(), name
        for (name, _, _), g in zip(gpu.Engine.CLASS_HIST_FIELDS, got_hi):
            assert g.tobytes() == hi[name].tobytes(), name
    assert at == len(raw)
    assert not np.array_equal(fine, own)
