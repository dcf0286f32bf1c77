// examples/vgs_tiles_run.cpp -- the native tiled driver (include/vgs_tiles.h) from the command line: one rank per tile.
//
//   RCCL, one process per GPU (started by any launcher that sets RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT --
//   torchrun's variables): rank 0 creates the ncclUniqueId and hands it to the others over a TCP socket on MASTER_PORT + 1,
//   every rank calls ncclCommInitRank and passes the communicator to vgs_tiles_create:
//       vgs_tiles_run --rccl 4x2 --pitch 50 --voxel 0.1 <prefix>
//   Emulation on one GPU (tests): the ranks are threads of this process and meet in shared memory:
//       vgs_tiles_run --emulate 2x2 --pitch 6.1 --voxel 0.1 <prefix>
//   Rank r reads its points from <prefix>.<r>.f32 (packed float32 xyz) and writes one int32 label per point to
//   <prefix>.<r>.labels.i32.  Prints "<world> <kept segments> <points of rank 0> <boundary records of rank 0>".
//   --segments <file.csv>: every rank takes part in vgs_tiles_get_segment_descriptors (a collective) and rank 0 writes the table of the
//   global segments in the CSV format of vgs_run --segments (examples/segments_csv.hpp).
//   --segment-graph <file.csv>: every rank takes part in vgs_tiles_get_segment_graph (a collective) and rank 0 writes the adjacency graph
//   of the global segments in the CSV format of vgs_run --segment-graph.
//   --segment-boxes <file.csv> [--box-frame principal|upright]: every rank takes part in vgs_tiles_get_segment_boxes (a collective; it
//   takes the descriptor table first) and rank 0 writes the oriented boxes of the global segments in the CSV format of vgs_run
//   --segment-boxes.
//   --segment-fields <file.csv> --field-channels <C>: rank r reads <prefix>.<r>.fields.f32 (packed float32, C values per point, in the order
//   of its points), every rank takes part in vgs_tiles_segment_field_stats (a collective; no attribute leaves its rank) and rank 0 writes
//   the table in the CSV format of vgs_run --segment-fields, the channels named f0 .. f{C-1}.
//   --segment-classes <file.csv> --classes <C>: rank r reads <prefix>.<r>.classes.i32 (one int32 per point), every rank takes part in
//   vgs_tiles_segment_class_histogram and rank 0 writes the table in the CSV format of vgs_run --segment-classes.
//   --segment-matches <file.csv> [--truth-matches <file.csv>]: rank r reads <prefix>.<r>.truth.i32 (one int32 reference id per point,
//   negative = not annotated), every rank takes part in vgs_tiles_compare_labels (a collective; no label and no id leaves its rank, only
//   contingency cells) and rank 0 writes the per-segment matches, and with --truth-matches the per-id matches, in the CSV formats of
//   vgs_run --segment-matches / --truth-matches.
//   --refine [--patch-radius <r>] [--switch-ratio <s>] [--no-fill]: every rank takes part in vgs_tiles_refine_point_labels (a collective;
//   no label of a point leaves its rank) and writes the refined label of each of its points to <prefix>.<r>.refined.i32, next to
//   .labels.i32.  --patch-radius (finite, not negative; default the voxel size), --switch-ratio in [0, 1] (default 0.25) and --no-fill need
//   --refine.  A second output line holds the counts "refine <working nodes> <examined> <changed> <filled> <beyond the strip>": summed
//   over the ranks with --emulate, one line per rank (its own share, behind "rank <r>") with --rccl.
//   --refined-segments <file.csv>, --refined-segment-boxes <file.csv>, --refined-matches <file.csv> [--refined-truth-matches <file.csv>]:
//   the same tables for the REFINED labels (they need --refine): every rank hands its refined labels to
//   vgs_tiles_point_label_descriptors, vgs_tiles_point_label_boxes (in the --box-frame) and vgs_tiles_compare_point_labels (against
//   <prefix>.<r>.truth.i32) -- collectives; no label leaves its rank -- and rank 0 writes the files, with the columns of vgs_run's
//   --refined-segments, --refined-segment-boxes, --refined-matches and --refined-truth-matches.
//   --refined-segment-fields <file.csv> --field-channels <C>, --refined-segment-classes <file.csv> --classes <C>: the attribute tables of the
//   REFINED labels (they need --refine), from the same <prefix>.<r>.fields.f32 / <prefix>.<r>.classes.i32: every rank hands its refined
//   labels and its rows to vgs_tiles_point_label_field_stats / vgs_tiles_point_label_class_histogram (collectives; nothing of a point
//   leaves its rank) and rank 0 writes the files, with the columns of vgs_run's --refined-segment-fields / --refined-segment-classes.
//   --field-channels and --classes serve the node option and the refined one alike.
//   --refined-components <file.csv> (needs --refine), --class-components <file.csv> --classes <C> (over <prefix>.<r>.classes.i32): the
//   connected parts of the refined labels, or of the classes, over all ranks -- every rank hands its labels to
//   vgs_tiles_point_label_components (two collectives; no label leaves its rank) and rank 0 writes one row per part with the columns of
//   vgs_run's --refined-components / --class-components, the shared-grid code of the part's first node (first_code) in place of the node.
//   --component-ids: every rank also writes the part of each of its points to <prefix>.<r>.parts.i32; it serves exactly one of the two.
//   --refined-graph <file.csv> (needs --refine), --class-graph <file.csv> --classes <C> (over <prefix>.<r>.classes.i32): the adjacency
//   graph of the refined labels, or of the classes, over all ranks -- every rank hands its labels to vgs_tiles_point_label_graph (two
//   collectives; no label leaves its rank) and rank 0 writes one row per edge with the columns and the writer of vgs_run's
//   --refined-graph / --class-graph.  A path that cannot be opened for writing is a usage error too.
//   All of them can be combined.  A missing companion option, a value out of range (1 .. 64 channels, 1 .. 1024 classes) and an attribute
//   or truth file that is missing or whose size does not match the rank's points are usage errors: exit status 2, before any collective.
#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <unistd.h>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "segments_csv.hpp"
#include "vgs_tiles.h"

static bool read_f32(const std::string& path, std::vector<float>& out) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out.resize((size_t)bytes / 4);
  const size_t got = std::fread(out.data(), 4, out.size(), f);
  std::fclose(f);
  return got == out.size();
}

static bool read_i32(const std::string& path, std::vector<int32_t>& out) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out.resize((size_t)bytes / 4);
  const size_t got = std::fread(out.data(), 4, out.size(), f);
  std::fclose(f);
  return got == out.size();
}

// size of a file in bytes, -1 if it cannot be examined
static long long file_bytes(const std::string& path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0 ? (long long)st.st_size : -1;
}

static bool write_i32(const std::string& path, const std::vector<int32_t>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t put = std::fwrite(v.data(), 4, v.size(), f);
  std::fclose(f);
  return put == v.size();
}

struct Job {
  vgs_params p; int tx, ty; double pitch; std::string prefix, segments, graph, boxes; int box_frame = VGS_BOX_PRINCIPAL;
  std::string fields, classes;        // --segment-fields / --segment-classes
  int field_channels = 0, n_classes = 0;
  std::string matches, truth_matches;   // --segment-matches / --truth-matches
  std::string r_segments, r_boxes, r_matches, r_truth_matches;   // --refined-segments / --refined-segment-boxes / --refined-matches / --refined-truth-matches
  std::string r_fields, r_classes;    // --refined-segment-fields / --refined-segment-classes
  std::string r_parts, c_parts;       // --refined-components / --class-components
  bool part_ids = false;              // --component-ids
  std::string r_lgraph, c_lgraph;     // --refined-graph / --class-graph
  bool refine = false, refine_fill = true;   // --refine, --no-fill
  float patch_radius = -1.0f, switch_ratio = -1.0f;   // --patch-radius / --switch-ratio (negative: the context's default)
};

static std::string rank_file(const Job& J, int rank, const char* suffix) { return J.prefix + "." + std::to_string(rank) + suffix; }

// The attribute files of one rank against its points, by size alone: 0 fine, 2 a usage error (message printed).  A points file that cannot
// be examined is left to run_rank.
static int check_attribute_files(const Job& J, int rank) {
  const long long pts = file_bytes(rank_file(J, rank, ".f32"));
  if (pts < 0) return 0;
  const long long n = pts / 12;
  if (!J.fields.empty() || !J.r_fields.empty()) {
    const std::string path = rank_file(J, rank, ".fields.f32");
    const long long b = file_bytes(path);
    if (b != n * 4 * (long long)J.field_channels) {
      std::fprintf(stderr, "%s: %lld bytes, but %lld points x %d channels x 4 = %lld\n", path.c_str(), b, n, J.field_channels, n * 4 * (long long)J.field_channels);
      return 2;
    }
  }
  if (!J.classes.empty() || !J.r_classes.empty() || !J.c_parts.empty() || !J.c_lgraph.empty()) {
    const std::string path = rank_file(J, rank, ".classes.i32");
    const long long b = file_bytes(path);
    if (b != n * 4) { std::fprintf(stderr, "%s: %lld bytes, but %lld points x 4 = %lld\n", path.c_str(), b, n, n * 4); return 2; }
  }
  if (!J.matches.empty() || !J.r_matches.empty()) {
    const std::string path = rank_file(J, rank, ".truth.i32");
    const long long b = file_bytes(path);
    if (b < 0) { std::fprintf(stderr, "%s: cannot be read; --segment-matches / --refined-matches need one int32 for each of the %lld points of rank %d\n", path.c_str(), n, rank); return 2; }
    if (b != n * 4) { std::fprintf(stderr, "%s: %lld bytes, but %lld points x 4 = %lld\n", path.c_str(), b, n, n * 4); return 2; }
  }
  return 0;
}

// The graph files of --refined-graph / --class-graph, which rank 0 writes at the very end: 0 fine, 2 a path that cannot be opened for
// writing (message printed).  The last of the refusals; a file the probe itself created is removed again.
static int check_graph_paths(const Job& J) {
  for (const std::string* path : {&J.r_lgraph, &J.c_lgraph}) {
    if (path->empty()) continue;
    const bool was_there = file_bytes(*path) >= 0;
    FILE* f = std::fopen(path->c_str(), "ab");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", path->c_str()); return 2; }
    std::fclose(f);
    if (!was_there) std::remove(path->c_str());
  }
  return 0;
}

// the tables as the CSV writers of segments_csv.hpp take them
struct DescArrays {
  std::vector<int64_t> np; std::vector<int32_t> nn; std::vector<float> bb, e8; std::vector<double> ce, cv, ev, vv;
  explicit DescArrays(size_t k) : np(k + 1), nn(k + 1), bb(6 * k + 1), e8(8 * k + 1), ce(3 * k + 1), cv(6 * k + 1), ev(3 * k + 1), vv(9 * k + 1) {}
};
static int write_descriptors(const std::string& path, size_t k, const DescArrays& A) {
  std::vector<pcl::ClusterDescriptor> desc(k);
  for (size_t i = 0; i < k; ++i) {
    pcl::ClusterDescriptor& d = desc[i];
    d.n_points = A.np[i]; d.n_nodes = A.nn[i];
    for (int a = 0; a < 6; ++a) { d.bbox[a] = A.bb[6 * i + a]; d.cov[a] = A.cv[6 * i + a]; }
    for (int a = 0; a < 3; ++a) { d.centroid[a] = A.ce[3 * i + a]; d.evals[a] = A.ev[3 * i + a]; }
    for (int a = 0; a < 9; ++a) d.evecs[a] = A.vv[9 * i + a];
    for (int a = 0; a < 8; ++a) d.eigen8[a] = A.e8[8 * i + a];
  }
  return writeSegmentsCsv(path, desc);
}
struct BoxArrays {
  std::vector<double> ce, ha, fr, lo, hi;
  explicit BoxArrays(size_t k) : ce(3 * k + 1), ha(3 * k + 1), fr(9 * k + 1), lo(3 * k + 1), hi(3 * k + 1) {}
};
static int write_boxes(const std::string& path, size_t k, const BoxArrays& A) {
  std::vector<pcl::ClusterBox> boxes(k);
  for (size_t i = 0; i < k; ++i) {
    pcl::ClusterBox& b = boxes[i];
    for (int a = 0; a < 3; ++a) { b.center[a] = A.ce[3 * i + a]; b.half[a] = A.ha[3 * i + a]; b.lo[a] = A.lo[3 * i + a]; b.hi[a] = A.hi[3 * i + a]; }
    for (int a = 0; a < 9; ++a) b.frame[a] = A.fr[9 * i + a];
  }
  return writeBoxesCsv(path, boxes);
}
// a field table of k rows x C channels (the channels named f0 .. f{C-1}) and a class table of k rows x nc classes
struct FieldArrays {
  std::vector<int64_t> nv; std::vector<double> an, me, va; std::vector<float> mn, mx;
  explicit FieldArrays(size_t kc) : nv(kc + 1), an(kc + 1), me(kc + 1), va(kc + 1), mn(kc + 1), mx(kc + 1) {}
};
static int write_field_stats(const std::string& path, size_t k, size_t C, const FieldArrays& A) {
  std::vector<std::string> names;
  for (size_t ch = 0; ch < C; ++ch) names.push_back("f" + std::to_string(ch));
  std::vector<pcl::ClusterFieldStats> stats(k);
  for (size_t i = 0; i < k; ++i) {
    pcl::ClusterFieldStats& f = stats[i];
    f.n_valid.assign(A.nv.begin() + i * C, A.nv.begin() + (i + 1) * C); f.anchor.assign(A.an.begin() + i * C, A.an.begin() + (i + 1) * C);
    f.mean.assign(A.me.begin() + i * C, A.me.begin() + (i + 1) * C); f.var.assign(A.va.begin() + i * C, A.va.begin() + (i + 1) * C);
    f.vmin.assign(A.mn.begin() + i * C, A.mn.begin() + (i + 1) * C); f.vmax.assign(A.mx.begin() + i * C, A.mx.begin() + (i + 1) * C);
  }
  return writeFieldStatsCsv(path, names, stats);
}
struct ClassArrays {
  std::vector<int64_t> hi, no, mc; std::vector<int32_t> ma;
  ClassArrays(size_t k, size_t nc) : hi(k * nc + 1), no(k + 1), mc(k + 1), ma(k + 1) {}
};
static int write_class_hist(const std::string& path, size_t k, size_t nc, const ClassArrays& A) {
  std::vector<pcl::ClusterClassHistogram> hist(k);
  for (size_t i = 0; i < k; ++i) {
    pcl::ClusterClassHistogram& h = hist[i];
    h.hist.assign(A.hi.begin() + i * nc, A.hi.begin() + (i + 1) * nc);
    h.n_outside = A.no[i]; h.majority = A.ma[i]; h.majority_count = A.mc[i];
  }
  return writeClassHistCsv(path, (int)nc, hist);
}
// the tables of the driver's last comparison (nc cells, G ids, K segment rows; m.summary is filled) into the match files; "" on success
static std::string write_matches(vgs_tiles* t, int64_t nc, int64_t G, int64_t K, pcl::ClusterLabelComparison& m, const std::string& seg_path,
                                 const std::string& truth_path) {
  m.cell_seg.resize((size_t)nc); m.cell_ref.resize((size_t)nc); m.cell_n.resize((size_t)nc);
  m.ref_id.resize((size_t)G); m.ref_points.resize((size_t)G); m.ref_dropped.resize((size_t)G); m.ref_best_seg.resize((size_t)G);
  m.ref_best_n.resize((size_t)G); m.ref_best_iou.resize((size_t)G);
  m.seg_annotated.resize((size_t)K); m.seg_refs.resize((size_t)K); m.seg_best_ref.resize((size_t)K); m.seg_best_n.resize((size_t)K);
  m.seg_best_iou.resize((size_t)K);
  if (vgs_tiles_get_label_comparison(t, m.cell_seg.data(), m.cell_ref.data(), m.cell_n.data(), m.ref_id.data(), m.ref_points.data(), m.ref_dropped.data(),
                                     m.ref_best_seg.data(), m.ref_best_n.data(), m.ref_best_iou.data(), m.seg_annotated.data(), m.seg_refs.data(),
                                     m.seg_best_ref.data(), m.seg_best_n.data(), m.seg_best_iou.data()) != VGS_OK)
    return std::string("rank 0: ") + vgs_tiles_last_error_string(t);
  if (writeSegmentMatchesCsv(seg_path, m) != 0) return "cannot write " + seg_path;
  if (!truth_path.empty() && writeTruthMatchesCsv(truth_path, m) != 0) return "cannot write " + truth_path;
  return "";
}

// The connected parts of a labelling of this rank's points with K labels: two collectives of every rank, the same table on each; rank 0
// writes the CSV, every rank its part ids when asked.  "" on success.
static std::string write_components(vgs_tiles* t, const Job& J, int rank, const std::vector<int32_t>& lab, int64_t n, int64_t K, const std::string& path) {
  int64_t C = 0, skipped = 0;
  if (vgs_tiles_point_label_components(t, lab.data(), n, K, &C, &skipped) != VGS_OK) return std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
  const size_t c = (size_t)C, k = (size_t)K;
  std::vector<int32_t> ids((size_t)n + 1), pl(c + 1), pn(c + 1), ll(k + 1);
  std::vector<int64_t> pp(c + 1), lf(k + 2);
  std::vector<uint64_t> pc(c + 1);
  if (vgs_tiles_get_point_label_components(t, ids.data(), pl.data(), pp.data(), pn.data(), pc.data(), lf.data(), ll.data()) != VGS_OK)
    return std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
  pl.resize(c); pp.resize(c); pn.resize(c); pc.resize(c); ll.resize(k); ids.resize((size_t)n);
  if (rank == 0 && writeTileComponentsCsv(path, pl, pp, pn, pc, ll) != 0) return "cannot write " + path;
  if (J.part_ids && !write_i32(rank_file(J, rank, ".parts.i32"), ids)) return "cannot write the part ids";
  return "";
}

// The adjacency graph of a labelling of this rank's points with K labels: two collectives of every rank, the same table on each; rank 0
// writes the CSV.  "" on success.
static std::string write_label_graph(vgs_tiles* t, int rank, const std::vector<int32_t>& lab, int64_t n, int64_t K, const std::string& path) {
  pcl::LabelGraph g;
  int64_t E = 0;
  if (vgs_tiles_point_label_graph(t, lab.data(), n, K, &E, &g.n_skipped) != VGS_OK) return std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
  if (rank != 0) return "";
  const size_t e1 = (size_t)E;
  std::vector<int32_t> ab(2 * e1 + 2), nd(2 * e1 + 2);
  std::vector<int64_t> ns(e1 + 1), np(e1 + 1), nf(e1 + 1);
  std::vector<double> ws(e1 + 1);
  std::vector<float> mn(e1 + 1), mx(e1 + 1);
  if (vgs_tiles_get_point_label_graph(t, ab.data(), ns.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data()) != VGS_OK)
    return std::string("rank 0: ") + vgs_tiles_last_error_string(t);
  g.edges.resize(e1);
  for (size_t i = 0; i < e1; ++i) {
    pcl::LabelEdge& e = g.edges[i];
    e.a = ab[2 * i]; e.b = ab[2 * i + 1]; e.n_shared = ns[i]; e.n_pairs = np[i]; e.n_finite = nf[i]; e.nodes_a = nd[2 * i]; e.nodes_b = nd[2 * i + 1];
    e.w_sum = ws[i]; e.w_min = mn[i]; e.w_max = mx[i];
  }
  return writeLabelGraphCsv(path, g) != 0 ? "cannot write " + path : "";
}

// one rank: load, run, save; returns 0 on success
static int run_rank(const Job& J, int comm_kind, void* comm, int rank, int world, int64_t* kept, int64_t* n_pts, int64_t* n_rec, int64_t* refine_counts /* 5 */, std::string* err) {
  std::vector<float> xyz;
  if (!read_f32(J.prefix + "." + std::to_string(rank) + ".f32", xyz)) { *err = "cannot read the points of rank " + std::to_string(rank); return 1; }
  std::vector<float> field;
  std::vector<int32_t> cls;
  if ((!J.fields.empty() || !J.r_fields.empty()) && !read_f32(rank_file(J, rank, ".fields.f32"), field)) { *err = "cannot read the fields of rank " + std::to_string(rank); return 1; }
  if ((!J.classes.empty() || !J.r_classes.empty() || !J.c_parts.empty() || !J.c_lgraph.empty()) && !read_i32(rank_file(J, rank, ".classes.i32"), cls)) { *err = "cannot read the classes of rank " + std::to_string(rank); return 1; }
  std::vector<int32_t> truth;
  if ((!J.matches.empty() || !J.r_matches.empty()) && !read_i32(rank_file(J, rank, ".truth.i32"), truth)) { *err = "cannot read the truth ids of rank " + std::to_string(rank); return 1; }
  vgs_tiles* t = nullptr;
  vgs_status s = vgs_tiles_create(&J.p, comm_kind, comm, rank, world, J.tx, J.ty, J.pitch, 0.0, 0.0, &t);
  if (s != VGS_OK) { *err = std::string("vgs_tiles_create: ") + vgs_last_error_string(nullptr); return 1; }
  const int64_t n = (int64_t)(xyz.size() / 3);
  std::vector<int32_t> labels((size_t)n + 1);
  int rc = 0;
  if ((s = vgs_tiles_set_points(t, xyz.data(), n, 12)) != VGS_OK || (s = vgs_tiles_run(t)) != VGS_OK ||
      (s = vgs_tiles_get_point_labels(t, labels.data(), kept)) != VGS_OK) {
    *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
    rc = 1;
  }
  if (rc == 0 && !J.segments.empty()) {
    // the descriptors of the global segments: a collective of every rank, the same table on each; rank 0 writes it
    const size_t k = (size_t)*kept;
    DescArrays A(k);
    int64_t K = 0;
    if (vgs_tiles_get_segment_descriptors(t, &K, A.np.data(), A.nn.data(), A.bb.data(), A.ce.data(), A.cv.data(), A.ev.data(), A.vv.data(), A.e8.data()) != VGS_OK) {
      *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
      rc = 1;
    } else if (rank == 0 && write_descriptors(J.segments, k, A) != 0) { *err = "cannot write " + J.segments; rc = 1; }
  }
  if (rc == 0 && !J.graph.empty()) {
    // the adjacency graph of the global segments: the first call is a collective of every rank and leaves the table cached
    int64_t E = 0;
    std::vector<pcl::ClusterEdge> edges;
    vgs_status sg = vgs_tiles_get_segment_graph(t, &E, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (sg == VGS_OK && rank == 0 && E > 0) {
      const size_t e1 = (size_t)E;
      std::vector<int32_t> ab(2 * e1), nd(2 * e1);
      std::vector<int64_t> np(e1), nf(e1);
      std::vector<double> ws(e1);
      std::vector<float> mn(e1), mx(e1);
      sg = vgs_tiles_get_segment_graph(t, &E, ab.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data());
      edges.resize(e1);
      for (size_t i = 0; i < e1; ++i) {
        pcl::ClusterEdge& e = edges[i];
        e.a = ab[2 * i]; e.b = ab[2 * i + 1]; e.n_pairs = np[i]; e.n_finite = nf[i]; e.nodes_a = nd[2 * i]; e.nodes_b = nd[2 * i + 1];
        e.w_sum = ws[i]; e.w_min = mn[i]; e.w_max = mx[i];
      }
    }
    if (sg != VGS_OK) { *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t); rc = 1; }
    else if (rank == 0 && writeGraphCsv(J.graph, edges) != 0) { *err = "cannot write " + J.graph; rc = 1; }
  }
  if (rc == 0 && !J.boxes.empty()) {
    // the oriented boxes of the global segments: a collective of every rank, the same table on each; rank 0 writes it
    const size_t k = (size_t)*kept;
    BoxArrays A(k);
    int64_t K = 0;
    if (vgs_tiles_get_segment_boxes(t, J.box_frame, &K, A.ce.data(), A.ha.data(), A.fr.data(), A.lo.data(), A.hi.data()) != VGS_OK) {
      *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
      rc = 1;
    } else if (rank == 0 && write_boxes(J.boxes, k, A) != 0) { *err = "cannot write " + J.boxes; rc = 1; }
  }
  if (rc == 0 && !J.fields.empty()) {
    // the statistics of this rank's attribute rows over the global segments: a collective of every rank, the same table on each
    const size_t k = (size_t)*kept, C = (size_t)J.field_channels;
    FieldArrays A(k * C);
    int64_t K = 0;
    if (vgs_tiles_segment_field_stats(t, field.data(), n, J.field_channels, 4 * (int64_t)J.field_channels, &K, A.nv.data(), A.an.data(), A.me.data(), A.va.data(),
                                      A.mn.data(), A.mx.data()) != VGS_OK) {
      *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
      rc = 1;
    } else if (rank == 0 && write_field_stats(J.fields, k, C, A) != 0) { *err = "cannot write " + J.fields; rc = 1; }
  }
  if (rc == 0 && !J.classes.empty()) {
    const size_t k = (size_t)*kept, nc = (size_t)J.n_classes;
    ClassArrays A(k, nc);
    int64_t K = 0;
    if (vgs_tiles_segment_class_histogram(t, cls.data(), n, J.n_classes, &K, A.hi.data(), A.no.data(), A.ma.data(), A.mc.data()) != VGS_OK) {
      *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
      rc = 1;
    } else if (rank == 0 && write_class_hist(J.classes, k, nc, A) != 0) { *err = "cannot write " + J.classes; rc = 1; }
  }
  if (rc == 0 && !J.matches.empty()) {
    // the score against this rank's reference ids over the global segments: a collective of every rank, the same tables on each
    int64_t K = 0, nc = 0, G = 0;
    pcl::ClusterLabelComparison m;
    if (vgs_tiles_compare_labels(t, truth.data(), n, &K, &nc, &G, m.summary) != VGS_OK) {
      *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
      rc = 1;
    } else if (rank == 0) {
      const std::string e = write_matches(t, nc, G, K, m, J.matches, J.truth_matches);
      if (!e.empty()) { *err = e; rc = 1; }
    }
  }
  if (rc == 0 && J.refine) {
    // the refined labels of this rank's points: a collective of every rank; each rank writes its own file
    vgs_refine_params rp;
    vgs_refine_params_default(vgs_tiles_context(t), &rp);
    if (J.patch_radius >= 0.0f) rp.patch_radius = J.patch_radius;
    if (J.switch_ratio >= 0.0f) rp.switch_ratio = J.switch_ratio;
    rp.fill = J.refine_fill ? 1 : 0;
    std::vector<int32_t> fine((size_t)n + 1);
    if (vgs_tiles_refine_point_labels(t, &rp, refine_counts) != VGS_OK || vgs_tiles_get_refined_labels(t, fine.data()) != VGS_OK) {
      *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
      rc = 1;
    } else {
      fine.resize((size_t)n);
      if (!write_i32(rank_file(J, rank, ".refined.i32"), fine)) { *err = "cannot write the refined labels"; rc = 1; }
    }
    // the tables of the refined labelling, K = kept rows: collectives of every rank, the same tables on each; rank 0 writes them
    const size_t k = (size_t)*kept;
    if (rc == 0 && !J.r_segments.empty()) {
      DescArrays A(k);
      int64_t skipped = 0;
      if (vgs_tiles_point_label_descriptors(t, fine.data(), n, *kept, &skipped, A.np.data(), A.nn.data(), A.bb.data(), A.ce.data(), A.cv.data(), A.ev.data(),
                                            A.vv.data(), A.e8.data()) != VGS_OK) {
        *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
        rc = 1;
      } else if (rank == 0 && write_descriptors(J.r_segments, k, A) != 0) { *err = "cannot write " + J.r_segments; rc = 1; }
    }
    if (rc == 0 && !J.r_boxes.empty()) {
      BoxArrays A(k);
      if (vgs_tiles_point_label_boxes(t, fine.data(), n, *kept, J.box_frame, A.ce.data(), A.ha.data(), A.fr.data(), A.lo.data(), A.hi.data()) != VGS_OK) {
        *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
        rc = 1;
      } else if (rank == 0 && write_boxes(J.r_boxes, k, A) != 0) { *err = "cannot write " + J.r_boxes; rc = 1; }
    }
    if (rc == 0 && !J.r_matches.empty()) {
      int64_t nc = 0, G = 0;
      pcl::ClusterLabelComparison m;
      if (vgs_tiles_compare_point_labels(t, fine.data(), *kept, truth.data(), n, &nc, &G, m.summary) != VGS_OK) {
        *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
        rc = 1;
      } else if (rank == 0) {
        const std::string e = write_matches(t, nc, G, *kept, m, J.r_matches, J.r_truth_matches);
        if (!e.empty()) { *err = e; rc = 1; }
      }
    }
    if (rc == 0 && !J.r_fields.empty()) {
      const size_t C = (size_t)J.field_channels;
      FieldArrays A(k * C);
      int64_t skipped = 0;
      if (vgs_tiles_point_label_field_stats(t, fine.data(), *kept, field.data(), n, J.field_channels, 4 * (int64_t)J.field_channels, &skipped, A.nv.data(),
                                            A.an.data(), A.me.data(), A.va.data(), A.mn.data(), A.mx.data()) != VGS_OK) {
        *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
        rc = 1;
      } else if (rank == 0 && write_field_stats(J.r_fields, k, C, A) != 0) { *err = "cannot write " + J.r_fields; rc = 1; }
    }
    if (rc == 0 && !J.r_classes.empty()) {
      const size_t nc = (size_t)J.n_classes;
      ClassArrays A(k, nc);
      int64_t skipped = 0;
      if (vgs_tiles_point_label_class_histogram(t, fine.data(), *kept, cls.data(), n, J.n_classes, &skipped, A.hi.data(), A.no.data(), A.ma.data(),
                                                A.mc.data()) != VGS_OK) {
        *err = std::string("rank ") + std::to_string(rank) + ": " + vgs_tiles_last_error_string(t);
        rc = 1;
      } else if (rank == 0 && write_class_hist(J.r_classes, k, nc, A) != 0) { *err = "cannot write " + J.r_classes; rc = 1; }
    }
    if (rc == 0 && !J.r_parts.empty()) {
      fine.resize((size_t)n + 1);
      const std::string e = write_components(t, J, rank, fine, n, *kept, J.r_parts);
      if (!e.empty()) { *err = e; rc = 1; }
    }
    if (rc == 0 && !J.r_lgraph.empty()) {
      fine.resize((size_t)n + 1);
      const std::string e = write_label_graph(t, rank, fine, n, *kept, J.r_lgraph);
      if (!e.empty()) { *err = e; rc = 1; }
    }
  }
  if (rc == 0 && !J.c_parts.empty()) {
    cls.resize((size_t)n + 1);
    const std::string e = write_components(t, J, rank, cls, n, J.n_classes, J.c_parts);
    if (!e.empty()) { *err = e; rc = 1; }
  }
  if (rc == 0 && !J.c_lgraph.empty()) {
    cls.resize((size_t)n + 1);
    const std::string e = write_label_graph(t, rank, cls, n, J.n_classes, J.c_lgraph);
    if (!e.empty()) { *err = e; rc = 1; }
  }
  if (rc == 0) {
    labels.resize((size_t)n);
    if (!write_i32(J.prefix + "." + std::to_string(rank) + ".labels.i32", labels)) { *err = "cannot write the labels"; rc = 1; }
    *n_pts = n;
    vgs_tiles_get_info(t, nullptr, nullptr, n_rec);
  }
  vgs_tiles_destroy(t);
  return rc;
}

// ncclUniqueId from rank 0 to everyone over TCP (the launcher gives MASTER_ADDR / MASTER_PORT; port + 1 is used here)
static bool exchange_id(ncclUniqueId* id, int rank, int world, const char* addr, int port) {
  if (world == 1) return true;
  if (rank == 0) {
    const int srv = socket(AF_INET, SOCK_STREAM, 0);
    int one = 1;
    setsockopt(srv, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    sockaddr_in a{};
    a.sin_family = AF_INET; a.sin_addr.s_addr = htonl(INADDR_ANY); a.sin_port = htons((uint16_t)port);
    if (bind(srv, (sockaddr*)&a, sizeof(a)) != 0 || listen(srv, world) != 0) { close(srv); return false; }
    for (int k = 1; k < world; ++k) {
      const int fd = accept(srv, nullptr, nullptr);
      if (fd < 0) { close(srv); return false; }
      const bool ok = write(fd, id, sizeof(*id)) == (ssize_t)sizeof(*id);
      close(fd);
      if (!ok) { close(srv); return false; }
    }
    close(srv);
    return true;
  }
  sockaddr_in a{};
  a.sin_family = AF_INET; a.sin_port = htons((uint16_t)port);
  if (inet_pton(AF_INET, addr, &a.sin_addr) != 1) return false;
  for (int attempt = 0; attempt < 600; ++attempt) {   // rank 0 may not be listening yet
    const int fd = socket(AF_INET, SOCK_STREAM, 0);
    if (connect(fd, (sockaddr*)&a, sizeof(a)) == 0) {
      size_t got = 0;
      while (got < sizeof(*id)) { const ssize_t r = read(fd, (char*)id + got, sizeof(*id) - got); if (r <= 0) break; got += (size_t)r; }
      close(fd);
      return got == sizeof(*id);
    }
    close(fd);
    usleep(100000);
  }
  return false;
}

static void print_usage(const char* exe) {
  std::fprintf(stderr, "usage: %s (--rccl|--emulate) <tx>x<ty> [--pitch m] [--voxel m] [--graph m] [--segments file.csv] [--segment-graph file.csv] [--segment-boxes file.csv [--box-frame principal|upright]] [--segment-fields file.csv --field-channels C] [--segment-classes file.csv --classes C] [--segment-matches file.csv [--truth-matches file.csv]] [--refine [--patch-radius r] [--switch-ratio s] [--no-fill] [--refined-segments file.csv] [--refined-segment-boxes file.csv] [--refined-matches file.csv [--refined-truth-matches file.csv]] [--refined-segment-fields file.csv --field-channels C] [--refined-segment-classes file.csv --classes C] [--refined-components file.csv] [--refined-graph file.csv]] [--class-components file.csv --classes C] [--component-ids] [--class-graph file.csv --classes C] <prefix>\n", exe);
}

int main(int argc, char** argv) {
  Job J;
  vgs_params_default_vgs(&J.p);
  J.p.voxel_size = 0.1f;
  J.tx = 1; J.ty = 1; J.pitch = 0.0;
  int mode = -1;   // 0 rccl, 1 emulate
  bool have_channels = false, have_classes = false, refine_opts = false;
  for (int a = 1; a < argc; ++a) {
    if ((!std::strcmp(argv[a], "--rccl") || !std::strcmp(argv[a], "--emulate")) && a + 1 < argc) {
      mode = !std::strcmp(argv[a], "--emulate") ? 1 : 0;
      if (std::sscanf(argv[++a], "%dx%d", &J.tx, &J.ty) != 2) { std::fprintf(stderr, "layout must be <tiles_x>x<tiles_y>\n"); return 2; }
    } else if (!std::strcmp(argv[a], "--pitch") && a + 1 < argc) J.pitch = std::atof(argv[++a]);
    else if (!std::strcmp(argv[a], "--voxel") && a + 1 < argc) J.p.voxel_size = (float)std::atof(argv[++a]);
    else if (!std::strcmp(argv[a], "--graph") && a + 1 < argc) J.p.graph_size = (float)std::atof(argv[++a]);
    else if (!std::strcmp(argv[a], "--segments") && a + 1 < argc) J.segments = argv[++a];
    else if (!std::strcmp(argv[a], "--segment-graph") && a + 1 < argc) J.graph = argv[++a];
    else if (!std::strcmp(argv[a], "--segment-boxes") && a + 1 < argc) J.boxes = argv[++a];
    else if (!std::strcmp(argv[a], "--box-frame") && a + 1 < argc) {
      ++a;
      if (!std::strcmp(argv[a], "principal")) J.box_frame = VGS_BOX_PRINCIPAL;
      else if (!std::strcmp(argv[a], "upright")) J.box_frame = VGS_BOX_UPRIGHT;
      else { std::fprintf(stderr, "--box-frame must be principal or upright\n"); return 2; }
    }
    else if (!std::strcmp(argv[a], "--segment-fields") && a + 1 < argc) J.fields = argv[++a];
    else if (!std::strcmp(argv[a], "--field-channels") && a + 1 < argc) { J.field_channels = std::atoi(argv[++a]); have_channels = true; }
    else if (!std::strcmp(argv[a], "--segment-classes") && a + 1 < argc) J.classes = argv[++a];
    else if (!std::strcmp(argv[a], "--classes") && a + 1 < argc) { J.n_classes = std::atoi(argv[++a]); have_classes = true; }
    else if (!std::strcmp(argv[a], "--segment-matches") && a + 1 < argc) J.matches = argv[++a];
    else if (!std::strcmp(argv[a], "--truth-matches") && a + 1 < argc) J.truth_matches = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segments") && a + 1 < argc) J.r_segments = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segment-boxes") && a + 1 < argc) J.r_boxes = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-matches") && a + 1 < argc) J.r_matches = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-truth-matches") && a + 1 < argc) J.r_truth_matches = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segment-fields") && a + 1 < argc) J.r_fields = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segment-classes") && a + 1 < argc) J.r_classes = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-components") && a + 1 < argc) J.r_parts = argv[++a];
    else if (!std::strcmp(argv[a], "--class-components") && a + 1 < argc) J.c_parts = argv[++a];
    else if (!std::strcmp(argv[a], "--component-ids")) J.part_ids = true;
    else if (!std::strcmp(argv[a], "--refined-graph") && a + 1 < argc) J.r_lgraph = argv[++a];
    else if (!std::strcmp(argv[a], "--class-graph") && a + 1 < argc) J.c_lgraph = argv[++a];
    else if (!std::strcmp(argv[a], "--refine")) J.refine = true;
    else if (!std::strcmp(argv[a], "--no-fill")) { J.refine_fill = false; refine_opts = true; }
    else if ((!std::strcmp(argv[a], "--patch-radius") || !std::strcmp(argv[a], "--switch-ratio")) && a + 1 < argc) {
      const bool radius = argv[a][2] == 'p';
      char* end = nullptr;
      const float v = std::strtof(argv[++a], &end);
      if (end == argv[a] || *end != 0 || !std::isfinite(v) || v < 0.0f || (!radius && v > 1.0f)) {
        std::fprintf(stderr, "%s %s: %s\n", argv[a - 1], argv[a], radius ? "a finite number, not negative" : "a number in [0, 1]");
        return 2;
      }
      (radius ? J.patch_radius : J.switch_ratio) = v;
      refine_opts = true;
    }
    else if (argv[a][0] != '-') J.prefix = argv[a];
    else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
  }
  if (mode < 0 || J.prefix.empty()) { print_usage(argv[0]); return 2; }
  if (!J.fields.empty() && !have_channels) { std::fprintf(stderr, "--segment-fields needs --field-channels <C>\n"); return 2; }
  if (!J.r_fields.empty() && !have_channels) { std::fprintf(stderr, "--refined-segment-fields needs --field-channels <C>\n"); return 2; }
  if (J.fields.empty() && J.r_fields.empty() && have_channels) { std::fprintf(stderr, "--field-channels needs --segment-fields <file.csv>\n"); return 2; }
  if (have_channels && (J.field_channels < 1 || J.field_channels > 64)) { std::fprintf(stderr, "--field-channels must be in 1 .. 64\n"); return 2; }
  if (!J.classes.empty() && !have_classes) { std::fprintf(stderr, "--segment-classes needs --classes <C>\n"); return 2; }
  if (!J.r_classes.empty() && !have_classes) { std::fprintf(stderr, "--refined-segment-classes needs --classes <C>\n"); return 2; }
  if (!J.c_parts.empty() && !have_classes) { std::fprintf(stderr, "--class-components needs --classes <C>\n"); print_usage(argv[0]); return 2; }
  if (!J.c_lgraph.empty() && !have_classes) { std::fprintf(stderr, "--class-graph needs --classes <C>\n"); print_usage(argv[0]); return 2; }
  if (J.classes.empty() && J.r_classes.empty() && J.c_parts.empty() && J.c_lgraph.empty() && have_classes) { std::fprintf(stderr, "--classes needs --segment-classes <file.csv>\n"); return 2; }
  if (have_classes && (J.n_classes < 1 || J.n_classes > 1024)) { std::fprintf(stderr, "--classes must be in 1 .. 1024\n"); print_usage(argv[0]); return 2; }
  if (J.part_ids && J.r_parts.empty() == J.c_parts.empty()) {
    std::fprintf(stderr, J.r_parts.empty() ? "--component-ids needs --refined-components or --class-components\n"
                                           : "--component-ids serves one table: exactly one of --refined-components and --class-components\n");
    print_usage(argv[0]);
    return 2;
  }
  if (J.matches.empty() && !J.truth_matches.empty()) { std::fprintf(stderr, "--truth-matches needs --segment-matches <file.csv>\n"); return 2; }
  if (refine_opts && !J.refine) { std::fprintf(stderr, "--patch-radius / --switch-ratio / --no-fill need --refine\n"); return 2; }
  if (!J.refine && (!J.r_segments.empty() || !J.r_boxes.empty() || !J.r_matches.empty() || !J.r_truth_matches.empty() || !J.r_fields.empty() ||
                    !J.r_classes.empty() || !J.r_parts.empty())) {
    std::fprintf(stderr, "--refined-segments / --refined-segment-boxes / --refined-matches / --refined-truth-matches / --refined-segment-fields / "
                         "--refined-segment-classes / --refined-components need --refine\n");
    print_usage(argv[0]);
    return 2;
  }
  if (J.r_matches.empty() && !J.r_truth_matches.empty()) { std::fprintf(stderr, "--refined-truth-matches needs --refined-matches <file.csv>\n"); return 2; }
  if (!J.r_lgraph.empty() && !J.refine) { std::fprintf(stderr, "--refined-graph needs --refine\n"); print_usage(argv[0]); return 2; }
  const int world = J.tx * J.ty;
  int64_t kept = 0, n_pts = 0, n_rec = 0;
  int64_t rcounts[5] = {0, 0, 0, 0, 0};
  if (mode == 1) {
    for (int r = 0; r < world; ++r) if (check_attribute_files(J, r) != 0) return 2;
    if (check_graph_paths(J) != 0) return 2;
    void* group = nullptr;
    vgs_tiles_local_group_create(world, &group);
    std::vector<std::thread> th;
    std::vector<int> rc((size_t)world, 0);
    std::vector<std::string> errs((size_t)world);
    std::vector<int64_t> k((size_t)world), np((size_t)world), nr((size_t)world), rcn(5 * (size_t)world, 0);
    for (int r = 0; r < world; ++r)
      th.emplace_back([&, r] {
        rc[(size_t)r] = run_rank(J, VGS_TILES_COMM_LOCAL, group, r, world, &k[(size_t)r], &np[(size_t)r], &nr[(size_t)r], &rcn[5 * (size_t)r], &errs[(size_t)r]);
        if (rc[(size_t)r]) vgs_tiles_local_group_abort(group);   // the other ranks must not wait for this one
      });
    for (auto& t : th) t.join();
    vgs_tiles_local_group_destroy(group);
    for (int r = 0; r < world; ++r) if (rc[(size_t)r]) { std::fprintf(stderr, "error: %s\n", errs[(size_t)r].c_str()); return 1; }
    for (int r = 1; r < world; ++r) if (k[(size_t)r] != k[0]) { std::fprintf(stderr, "error: ranks disagree on the number of segments\n"); return 1; }
    kept = k[0]; n_pts = np[0]; n_rec = nr[0];
    for (int r = 0; r < world; ++r) for (int i = 0; i < 5; ++i) rcounts[i] += rcn[5 * (size_t)r + (size_t)i];
  } else {
    const char* e_rank = std::getenv("RANK"); const char* e_world = std::getenv("WORLD_SIZE"); const char* e_local = std::getenv("LOCAL_RANK");
    const char* e_addr = std::getenv("MASTER_ADDR"); const char* e_port = std::getenv("MASTER_PORT");
    const int rank = e_rank ? std::atoi(e_rank) : 0;
    if (check_attribute_files(J, rank) != 0) return 2;
    if (rank == 0 && check_graph_paths(J) != 0) return 2;
    if ((e_world ? std::atoi(e_world) : 1) != world) { std::fprintf(stderr, "WORLD_SIZE does not match the %dx%d layout\n", J.tx, J.ty); return 2; }
    J.p.device = e_local ? std::atoi(e_local) : 0;
    if (hipSetDevice(J.p.device) != hipSuccess) { std::fprintf(stderr, "hipSetDevice(%d) failed\n", J.p.device); return 1; }
    ncclUniqueId id;
    if (rank == 0 && ncclGetUniqueId(&id) != ncclSuccess) { std::fprintf(stderr, "ncclGetUniqueId failed\n"); return 1; }
    if (!exchange_id(&id, rank, world, e_addr ? e_addr : "127.0.0.1", (e_port ? std::atoi(e_port) : 29500) + 1)) { std::fprintf(stderr, "rank %d: cannot exchange the ncclUniqueId\n", rank); return 1; }
    ncclComm_t comm;
    if (ncclCommInitRank(&comm, world, id, rank) != ncclSuccess) { std::fprintf(stderr, "rank %d: ncclCommInitRank failed\n", rank); return 1; }
    std::string err;
    const int rc = run_rank(J, VGS_TILES_COMM_RCCL, (void*)comm, rank, world, &kept, &n_pts, &n_rec, rcounts, &err);
    ncclCommDestroy(comm);
    if (rc) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
    // (every rank its own share: a sum over the ranks would be a collective for a printout)
    if (J.refine && rank != 0) std::printf("rank %d refine %ld %ld %ld %ld %ld\n", rank, (long)rcounts[0], (long)rcounts[1], (long)rcounts[2], (long)rcounts[3], (long)rcounts[4]);
    if (rank != 0) return 0;
  }
  std::printf("%d %ld %ld %ld\n", world, (long)kept, (long)n_pts, (long)n_rec);
  if (J.refine) std::printf("%srefine %ld %ld %ld %ld %ld\n", mode == 1 ? "" : "rank 0 ", (long)rcounts[0], (long)rcounts[1], (long)rcounts[2], (long)rcounts[3], (long)rcounts[4]);
  return 0;
}
