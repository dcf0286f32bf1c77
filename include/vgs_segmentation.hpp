// include/vgs_segmentation.hpp -- host-side C++ mirror of the reference's two class templates over the
// C-ABI of include/vgs.h.  Same class names, member names, argument meaning and call order as
//   pcl::VoxelBasedSegmentation<PointT>       (reference voxel_segmentation.h:57-2305)
//   pcl::SuperVoxelBasedSegmentation<PointT>  (reference supervoxel_segmentation.h:58-2308)
// so that the reference's driver functions segmentationVGS / segmentationSVGS (reference `test`:9-170) compile
// against this header after replacing the PCL cloud types by the two small types below (PCL is not a
// dependency of this engine).  Every member forwards to one or two C entry points; no computation happens here.
//
// What is deliberately NOT mirrored: PCD/PLY IO, viewers, the draw*
// mesh helpers, FPFH and weighted-covariance dead code.  drawColorMapofPointsinClusters is kept because the
// reference makes it obligatory before getClusterIdx (VS:947-1014): here it returns per-point labels.
//
// Error behaviour: the reference's members are void and unchecked; here a failed call throws std::runtime_error
// carrying vgs_last_error_string (bad call order -> VGS_E_STATE instead of reading uninitialised members).
#ifndef VGS_SEGMENTATION_HPP_
#define VGS_SEGMENTATION_HPP_

#include <cstdint>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "vgs.h"

namespace pcl {

struct PointXYZ {  // 16 bytes like pcl::PointXYZ (x, y, z, padding)
  float x, y, z, pad;
  PointXYZ() : x(0), y(0), z(0), pad(1.0f) {}
  PointXYZ(float x_, float y_, float z_) : x(x_), y(y_), z(z_), pad(1.0f) {}
};

struct PointXYZRGB {  // x, y, z, padding, then the colour packed as PCL packs it: 0x00RRGGBB in one 32-bit word
  float x, y, z, pad;
  uint32_t rgba;
  float pad2[3];
  PointXYZRGB() : x(0), y(0), z(0), pad(1.0f), rgba(0), pad2{0, 0, 0} {}
};

template <typename PointT>
struct PointCloud {
  typedef std::shared_ptr<PointCloud<PointT>> Ptr;
  std::vector<PointT> points;
  uint32_t width = 0, height = 1;
  size_t size() const { return points.size(); }
};

}  // namespace pcl

typedef pcl::PointCloud<pcl::PointXYZ>::Ptr PCXYZPtr;
typedef pcl::PointCloud<pcl::PointXYZ> PCXYZ;
typedef pcl::PointCloud<pcl::PointXYZRGB> PCXYZRGB;
typedef pcl::PointCloud<pcl::PointXYZRGB>::Ptr PCXYZRGBPtr;

namespace vgs_color {
// one colour per cluster from a 64-bit LCG (Knuth's MMIX constants), seeded: the reference draws its colours with
// rand() after srand(time(0)) (VS:960, point_clouds_IO.cpp:36), so its files differ from run to run; these do not
struct Palette {
  uint64_t s;
  explicit Palette(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull) {}
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33) & 0x00ffffffu;  // 0x00RRGGBB
  }
};
// cluster by cluster, member by member (VS:963-1009, point_clouds_IO.cpp:39-61); points of no cluster are absent
inline void color_clusters(const PCXYZ& in, const std::vector<std::vector<int>>& clusters, uint64_t seed, PCXYZRGB& out) {
  Palette pal(seed);
  size_t total = 0;
  for (const auto& c : clusters) total += c.size();
  out.points.clear();
  out.points.reserve(total);
  for (const auto& c : clusters) {
    const uint32_t colour = pal.next();
    for (int idx : c) {
      pcl::PointXYZRGB q;
      const pcl::PointXYZ& p = in.points[(size_t)idx];
      q.x = p.x; q.y = p.y; q.z = p.z; q.rgba = colour;
      out.points.push_back(q);
    }
  }
  out.width = (uint32_t)out.points.size(); out.height = 1;
}
}  // namespace vgs_color

namespace pcl {

namespace vgs_detail {
inline void check(vgs_ctx* c, vgs_status s, const char* what) {
  if (s != VGS_OK) throw std::runtime_error(std::string(what) + ": " + vgs_last_error_string(c));
}
struct CtxDeleter { void operator()(vgs_ctx* c) const { vgs_destroy(c); } };
}  // namespace vgs_detail

// Extension (no VS / SS line): the geometric descriptor of one kept cluster, as vgs_get_segment_descriptors (include/vgs.h) defines it
struct ClusterDescriptor {
  int64_t n_points = 0;   // points of the cluster
  int32_t n_nodes = 0;    // voxels (VGS) or supervoxels (SVGS)
  float bbox[6] = {0, 0, 0, 0, 0, 0};   // min x, y, z, max x, y, z
  double centroid[3] = {0, 0, 0};
  double cov[6] = {0, 0, 0, 0, 0, 0};   // population covariance: xx, xy, xz, yy, yz, zz
  double evals[3] = {0, 0, 0};          // ascending
  double evecs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // [r*3+j] = component r of eigenvector j: column 0 the normal, column 2 the major axis
  float eigen8[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // the eight eigen features of the method (as the per-node ones)
};

namespace vgs_detail {
// one row per kept cluster, in label order -- the order of getClusterIdx (cluster k of either order holds the points labelled k)
// labels != nullptr: the rows of that per-point labelling (n labels in 0 .. k-1 or negative) instead, as vgs_point_label_descriptors
// defines them; *n_skipped = its labelled points outside the octree
inline std::vector<ClusterDescriptor> cluster_descriptors(vgs_ctx* c, int64_t k, const int32_t* labels = nullptr, int64_t n = 0,
                                                          int64_t* n_skipped = nullptr) {
  std::vector<ClusterDescriptor> out((size_t)k);
  if (k == 0 && !labels) return out;
  std::vector<int64_t> np((size_t)k + 1);
  std::vector<int32_t> nn((size_t)k + 1);
  std::vector<float> bb((size_t)k * 6 + 1), e8((size_t)k * 8 + 1);
  std::vector<double> ce((size_t)k * 3 + 1), cv((size_t)k * 6 + 1), ev((size_t)k * 3 + 1), vv((size_t)k * 9 + 1);
  if (labels)   // (called for k = 0 too: the state and argument checks are the library's)
    check(c, vgs_point_label_descriptors(c, labels, n, k, n_skipped, np.data(), nn.data(), bb.data(), ce.data(), cv.data(), ev.data(), vv.data(),
                                         e8.data()), "vgs_point_label_descriptors");
  else
    check(c, vgs_get_segment_descriptors(c, np.data(), nn.data(), bb.data(), ce.data(), cv.data(), ev.data(), vv.data(), e8.data()),
          "vgs_get_segment_descriptors");
  for (size_t i = 0; i < (size_t)k; ++i) {
    ClusterDescriptor& d = out[i];
    d.n_points = np[i]; d.n_nodes = nn[i];
    for (int a = 0; a < 6; ++a) { d.bbox[a] = bb[6 * i + a]; d.cov[a] = cv[6 * i + a]; }
    for (int a = 0; a < 3; ++a) { d.centroid[a] = ce[3 * i + a]; d.evals[a] = ev[3 * i + a]; }
    for (int a = 0; a < 9; ++a) d.evecs[a] = vv[9 * i + a];
    for (int a = 0; a < 8; ++a) d.eigen8[a] = e8[8 * i + a];
  }
  return out;
}
}  // namespace vgs_detail

// Extension (no VS / SS line): the oriented bounding box of one kept cluster, as vgs_get_segment_boxes (include/vgs.h) defines it
struct ClusterBox {
  double center[3] = {0, 0, 0};   // centre of the box
  double half[3] = {0, 0, 0};     // half extent along axis j
  double frame[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // [r*3+j] = component r of axis j
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};     // min and max of the projections of (p - centroid) onto axis j
};

namespace vgs_detail {
// one row per kept cluster, in label order -- the order of getClusterIdx
// labels != nullptr: the boxes of that per-point labelling instead, as vgs_point_label_boxes defines them
inline std::vector<ClusterBox> cluster_boxes(vgs_ctx* c, int64_t k, int frame, const int32_t* labels = nullptr, int64_t n = 0) {
  std::vector<ClusterBox> out((size_t)k);
  std::vector<double> ce((size_t)k * 3 + 1), ha((size_t)k * 3 + 1), fr((size_t)k * 9 + 1), lo((size_t)k * 3 + 1), hi((size_t)k * 3 + 1);
  // (called for k = 0 too: the state and frame checks are the library's)
  if (labels)
    check(c, vgs_point_label_boxes(c, labels, n, k, (int32_t)frame, ce.data(), ha.data(), fr.data(), lo.data(), hi.data()), "vgs_point_label_boxes");
  else
    check(c, vgs_get_segment_boxes(c, (int32_t)frame, ce.data(), ha.data(), fr.data(), lo.data(), hi.data()), "vgs_get_segment_boxes");
  for (size_t i = 0; i < (size_t)k; ++i) {
    ClusterBox& b = out[i];
    for (int a = 0; a < 3; ++a) { b.center[a] = ce[3 * i + a]; b.half[a] = ha[3 * i + a]; b.lo[a] = lo[3 * i + a]; b.hi[a] = hi[3 * i + a]; }
    for (int a = 0; a < 9; ++a) b.frame[a] = fr[9 * i + a];
  }
  return out;
}
}  // namespace vgs_detail

// Extension (no VS / SS line): the statistics of a caller's point attribute over one kept cluster, one entry per channel, as
// vgs_segment_field_stats (include/vgs.h) defines them
struct ClusterFieldStats {
  std::vector<int64_t> n_valid;          // finite values of the channel
  std::vector<double> anchor, mean, var; // the shift of the sums; anchor + S1 / n; population variance (NaN without a finite value)
  std::vector<float> vmin, vmax;         // min and max of the finite values (NaN without one)
};
// Extension (no VS / SS line): the class counts of one kept cluster, as vgs_segment_class_histogram (include/vgs.h) defines them
struct ClusterClassHistogram {
  std::vector<int64_t> hist;    // points per class 0 .. n_classes - 1
  int64_t n_outside = 0;        // points whose class is negative or >= n_classes
  int32_t majority = -1;        // the lowest class with the largest count, -1 without one
  int64_t majority_count = 0;
};

namespace vgs_detail {
// one row per kept cluster, in label order -- the order of getClusterIdx; stride in bytes
// labels != nullptr: the rows of that per-point labelling (n labels in 0 .. k-1 or negative) instead, as vgs_point_label_field_stats /
// vgs_point_label_class_histogram define them; *n_skipped = its labelled points outside the octree
inline std::vector<ClusterFieldStats> cluster_field_stats(vgs_ctx* c, int64_t k, const float* field, int64_t n, int32_t channels, int64_t stride,
                                                          const int32_t* labels = nullptr, int64_t* n_skipped = nullptr) {
  const size_t ch = channels > 0 ? (size_t)channels : 0, kc = (size_t)k * ch;
  std::vector<int64_t> nv(kc + 1);
  std::vector<double> an(kc + 1), me(kc + 1), va(kc + 1);
  std::vector<float> mn(kc + 1), mx(kc + 1);
  // (called for k = 0 too: the state and argument checks are the library's)
  if (labels)
    check(c, vgs_point_label_field_stats(c, labels, k, field, n, channels, stride, n_skipped, nv.data(), an.data(), me.data(), va.data(), mn.data(),
                                         mx.data()), "vgs_point_label_field_stats");
  else
    check(c, vgs_segment_field_stats(c, field, n, channels, stride, nv.data(), an.data(), me.data(), va.data(), mn.data(), mx.data()),
          "vgs_segment_field_stats");
  std::vector<ClusterFieldStats> out((size_t)k);
  for (size_t i = 0; i < (size_t)k; ++i) {
    ClusterFieldStats& f = out[i];
    f.n_valid.assign(nv.begin() + i * ch, nv.begin() + (i + 1) * ch);
    f.anchor.assign(an.begin() + i * ch, an.begin() + (i + 1) * ch);
    f.mean.assign(me.begin() + i * ch, me.begin() + (i + 1) * ch);
    f.var.assign(va.begin() + i * ch, va.begin() + (i + 1) * ch);
    f.vmin.assign(mn.begin() + i * ch, mn.begin() + (i + 1) * ch);
    f.vmax.assign(mx.begin() + i * ch, mx.begin() + (i + 1) * ch);
  }
  return out;
}
inline std::vector<ClusterClassHistogram> cluster_class_histogram(vgs_ctx* c, int64_t k, const int32_t* cls, int64_t n, int32_t n_classes,
                                                                  const int32_t* labels = nullptr, int64_t* n_skipped = nullptr) {
  const size_t nc = n_classes > 0 ? (size_t)n_classes : 0;
  std::vector<int64_t> hi((size_t)k * nc + 1), no((size_t)k + 1), mc((size_t)k + 1);
  std::vector<int32_t> ma((size_t)k + 1);
  if (labels)
    check(c, vgs_point_label_class_histogram(c, labels, k, cls, n, n_classes, n_skipped, hi.data(), no.data(), ma.data(), mc.data()),
          "vgs_point_label_class_histogram");
  else
    check(c, vgs_segment_class_histogram(c, cls, n, n_classes, hi.data(), no.data(), ma.data(), mc.data()), "vgs_segment_class_histogram");
  std::vector<ClusterClassHistogram> out((size_t)k);
  for (size_t i = 0; i < (size_t)k; ++i) {
    ClusterClassHistogram& h = out[i];
    h.hist.assign(hi.begin() + i * nc, hi.begin() + (i + 1) * nc);
    h.n_outside = no[i]; h.majority = ma[i]; h.majority_count = mc[i];
  }
  return out;
}
}  // namespace vgs_detail

// Extension (no VS / SS line): the comparison of the clusters with a reference labelling of the same points, as vgs_compare_labels
// (include/vgs.h) defines it: the cells (one per distinct (cluster, id) pair, ascending, cluster -1 = dropped points first), one row per
// distinct reference id, one row per kept cluster (getClusterIdx order), and the summary
struct ClusterLabelComparison {
  std::vector<int32_t> cell_seg, cell_ref;
  std::vector<int64_t> cell_n;
  std::vector<int32_t> ref_id;
  std::vector<int64_t> ref_points, ref_dropped;
  std::vector<int32_t> ref_best_seg;
  std::vector<int64_t> ref_best_n;
  std::vector<double> ref_best_iou;
  std::vector<int64_t> seg_annotated;
  std::vector<int32_t> seg_refs, seg_best_ref;
  std::vector<int64_t> seg_best_n;
  std::vector<double> seg_best_iou;
  int64_t summary[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};
// The scores read off a comparison: clusters matched to an id with IoU > tau (0.5 <= tau < 1), precision = matched / clusters with an
// annotated point, recall = matched / ids, F1, purity, completeness and the adjusted Rand index over the annotated points (the dropped
// points as one class); NaN where a denominator is zero
struct ClusterLabelScores { int64_t matched = 0; double precision = 0, recall = 0, f1 = 0, purity = 0, completeness = 0, ari = 0; };
inline ClusterLabelScores clusterLabelScores(const ClusterLabelComparison& c, double tau = 0.5) {
  if (!(tau >= 0.5 && tau < 1.0)) throw std::runtime_error("clusterLabelScores: tau must lie in [0.5, 1)");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto div = [nan](double a, double b) { return b != 0.0 ? a / b : nan; };
  const int64_t* s = c.summary;
  ClusterLabelScores o;
  for (double v : c.seg_best_iou) o.matched += v > tau ? 1 : 0;
  o.precision = div((double)o.matched, (double)s[5]);
  o.recall = div((double)o.matched, (double)s[3]);
  o.f1 = (o.precision == o.precision && o.recall == o.recall) ? div(2.0 * o.precision * o.recall, o.precision + o.recall) : nan;
  o.purity = div((double)s[6], (double)(s[0] - s[2]));
  o.completeness = div((double)s[7], (double)s[0]);
  const double T = (double)(s[0] % 2 ? s[0] * ((s[0] - 1) / 2) : (s[0] / 2) * (s[0] - 1));
  const double e = div((double)s[9] * (double)s[10], T);
  o.ari = e == e ? div((double)s[8] - e, ((double)s[9] + (double)s[10]) / 2.0 - e) : nan;
  return o;
}

namespace vgs_detail {
inline std::vector<int32_t> refined_labels(vgs_ctx* c, int64_t n, float patch_radius, float switch_ratio, bool fill) {
  vgs_refine_params rp;
  check(c, vgs_refine_params_default(c, &rp), "vgs_refine_params_default");
  if (patch_radius >= 0.0f) rp.patch_radius = patch_radius;
  rp.switch_ratio = switch_ratio;
  rp.fill = fill ? 1 : 0;
  check(c, vgs_refine_point_labels(c, &rp, nullptr), "vgs_refine_point_labels");
  std::vector<int32_t> out((size_t)n);
  if (n > 0) check(c, vgs_get_refined_labels(c, out.data()), "vgs_get_refined_labels");
  return out;
}
// labels != nullptr: that per-point labelling (k rows) is scored instead of the clusters' own, as vgs_compare_point_labels defines it
inline ClusterLabelComparison cluster_label_comparison(vgs_ctx* c, int64_t k, const int32_t* ref, int64_t n, const int32_t* labels = nullptr) {
  ClusterLabelComparison o;
  int64_t n_cells = 0, n_refs = 0;
  if (labels) check(c, vgs_compare_point_labels(c, labels, k, ref, n, &n_cells, &n_refs, o.summary), "vgs_compare_point_labels");
  else check(c, vgs_compare_labels(c, ref, n, &n_cells, &n_refs, o.summary), "vgs_compare_labels");
  const size_t nc = (size_t)n_cells, g = (size_t)n_refs, kk = (size_t)k;
  o.cell_seg.resize(nc); o.cell_ref.resize(nc); o.cell_n.resize(nc);
  o.ref_id.resize(g); o.ref_points.resize(g); o.ref_dropped.resize(g); o.ref_best_seg.resize(g); o.ref_best_n.resize(g); o.ref_best_iou.resize(g);
  o.seg_annotated.resize(kk); o.seg_refs.resize(kk); o.seg_best_ref.resize(kk); o.seg_best_n.resize(kk); o.seg_best_iou.resize(kk);
  check(c, vgs_get_label_comparison(c, o.cell_seg.data(), o.cell_ref.data(), o.cell_n.data(), o.ref_id.data(), o.ref_points.data(),
                                    o.ref_dropped.data(), o.ref_best_seg.data(), o.ref_best_n.data(), o.ref_best_iou.data(),
                                    o.seg_annotated.data(), o.seg_refs.data(), o.seg_best_ref.data(), o.seg_best_n.data(), o.seg_best_iou.data()),
        "vgs_get_label_comparison");
  return o;
}
}  // namespace vgs_detail

// Extension (no VS / SS line): the connected parts of a per-point labelling over the node adjacency, as vgs_point_label_components
// (include/vgs.h) defines them: the part of every point (-1: no label or no node), one row per part in ascending (label, smallest node id
// of the part), and per label its first part (K + 1 entries) and its largest (-1 for a label no point carries)
struct LabelComponents {
  std::vector<int32_t> part_of_point, part_label;
  std::vector<int64_t> part_points;
  std::vector<int32_t> part_nodes, part_first_node;
  std::vector<int64_t> label_first;
  std::vector<int32_t> label_largest;
  int64_t n_skipped = 0;   // labelled points outside the octree
};

namespace vgs_detail {
inline LabelComponents label_components(vgs_ctx* c, int64_t k, const int32_t* labels, int64_t n) {
  LabelComponents o;
  int64_t n_parts = 0;
  check(c, vgs_point_label_components(c, labels, n, k, &n_parts, &o.n_skipped), "vgs_point_label_components");
  const size_t C = (size_t)n_parts, K = (size_t)k;
  o.part_of_point.resize((size_t)n); o.part_label.resize(C); o.part_points.resize(C); o.part_nodes.resize(C); o.part_first_node.resize(C);
  o.label_first.resize(K + 1); o.label_largest.resize(K);
  check(c, vgs_get_point_label_components(c, o.part_of_point.data(), o.part_label.data(), o.part_points.data(), o.part_nodes.data(),
                                          o.part_first_node.data(), o.label_first.data(), o.label_largest.data()), "vgs_get_point_label_components");
  return o;
}
}  // namespace vgs_detail

// Extension (no VS / SS line): one edge of the adjacency graph of the kept clusters, as vgs_get_segment_graph (include/vgs.h) defines it
struct ClusterEdge {
  int32_t a = 0, b = 0;        // cluster indices (getClusterIdx order), a < b
  int64_t n_pairs = 0;         // node pairs {u, v} of a and b inside graph_size of each other
  int64_t n_finite = 0;        // ... whose weight is not NaN
  int32_t nodes_a = 0, nodes_b = 0;   // nodes of a with a neighbour in b, nodes of b with a neighbour in a
  double w_sum = 0;            // sum of the finite local-cut weights of those pairs
  float w_min = 0, w_max = 0;  // their min and max (NaN when n_finite == 0)
};

namespace vgs_detail {
// every edge once, in ascending (a, b) order
inline std::vector<ClusterEdge> cluster_graph(vgs_ctx* c) {
  int64_t E = 0;
  check(c, vgs_get_segment_graph(c, &E, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "vgs_get_segment_graph");
  std::vector<ClusterEdge> out((size_t)E);
  if (E == 0) return out;
  std::vector<int32_t> ab((size_t)E * 2), nd((size_t)E * 2);
  std::vector<int64_t> np((size_t)E), nf((size_t)E);
  std::vector<double> ws((size_t)E);
  std::vector<float> mn((size_t)E), mx((size_t)E);
  check(c, vgs_get_segment_graph(c, &E, ab.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data()), "vgs_get_segment_graph");
  for (size_t i = 0; i < out.size(); ++i) {
    ClusterEdge& e = out[i];
    e.a = ab[2 * i]; e.b = ab[2 * i + 1];
    e.n_pairs = np[i]; e.n_finite = nf[i];
    e.nodes_a = nd[2 * i]; e.nodes_b = nd[2 * i + 1];
    e.w_sum = ws[i]; e.w_min = mn[i]; e.w_max = mx[i];
  }
  return out;
}
}  // namespace vgs_detail

// Extension (no VS / SS line): one edge of the adjacency graph of a per-point labelling, as vgs_point_label_graph (include/vgs.h) defines
// it: ClusterEdge's fields over the CONTACTS of labels a < b (pairs of adjacent nodes, one carrying a and the other b), plus the nodes
// that carry both
struct LabelEdge : ClusterEdge {
  int64_t n_shared = 0;
};
struct LabelGraph {
  std::vector<LabelEdge> edges;   // ascending (a, b)
  int64_t n_skipped = 0;          // labelled points outside the octree
};

// Extension (no VS / SS line): a per-point labelling with its stranded and small connected parts absorbed into the neighbour they touch
// most, as vgs_absorb_point_label_parts (include/vgs.h) defines it, and the eight counts of the call
struct AbsorbedLabels {
  std::vector<int32_t> labels;   // input order; -1 for a dropped point
  int64_t rounds = 0, parts_absorbed = 0, points_relabelled = 0;   // applied rounds; parts and points, summed over them
  int64_t candidates_left = 0, candidate_points_left = 0;          // of the final evaluation
  int64_t points_dropped = 0, n_parts = 0, n_skipped = 0;          // n_parts: of the final evaluation
};

namespace vgs_detail {
inline LabelGraph label_graph(vgs_ctx* c, int64_t k, const int32_t* labels, int64_t n) {
  LabelGraph o;
  int64_t E = 0;
  check(c, vgs_point_label_graph(c, labels, n, k, &E, &o.n_skipped), "vgs_point_label_graph");
  o.edges.resize((size_t)E);
  if (E == 0) return o;
  std::vector<int32_t> ab((size_t)E * 2), nd((size_t)E * 2);
  std::vector<int64_t> ns((size_t)E), np((size_t)E), nf((size_t)E);
  std::vector<double> ws((size_t)E);
  std::vector<float> mn((size_t)E), mx((size_t)E);
  check(c, vgs_get_point_label_graph(c, ab.data(), ns.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data()),
        "vgs_get_point_label_graph");
  for (size_t i = 0; i < o.edges.size(); ++i) {
    LabelEdge& e = o.edges[i];
    e.a = ab[2 * i]; e.b = ab[2 * i + 1];
    e.n_shared = ns[i]; e.n_pairs = np[i]; e.n_finite = nf[i];
    e.nodes_a = nd[2 * i]; e.nodes_b = nd[2 * i + 1];
    e.w_sum = ws[i]; e.w_min = mn[i]; e.w_max = mx[i];
  }
  return o;
}
// the call of vgs_absorb_point_label_parts and its result
inline AbsorbedLabels absorb_label_parts(vgs_ctx* c, int64_t k, const int32_t* labels, int64_t n, int64_t min_points, int64_t island_points,
                                         int32_t max_rounds, bool drop) {
  AbsorbedLabels o;
  vgs_absorb_params ap;
  check(c, vgs_absorb_params_default(&ap), "vgs_absorb_params_default");
  ap.min_points = min_points; ap.island_points = island_points; ap.max_rounds = max_rounds; ap.drop = drop ? 1 : 0;
  int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  check(c, vgs_absorb_point_label_parts(c, labels, n, k, &ap, counts), "vgs_absorb_point_label_parts");
  o.labels.resize((size_t)n);
  check(c, vgs_get_absorbed_point_labels(c, o.labels.data()), "vgs_get_absorbed_point_labels");
  o.rounds = counts[0]; o.parts_absorbed = counts[1]; o.points_relabelled = counts[2]; o.candidates_left = counts[3];
  o.candidate_points_left = counts[4]; o.points_dropped = counts[5]; o.n_parts = counts[6]; o.n_skipped = counts[7];
  return o;
}
// PCL's getSupervoxelAdjacency idiom: both directions of every edge, keyed by cluster index
inline void cluster_adjacency(const std::vector<ClusterEdge>& g, std::multimap<uint32_t, uint32_t>& adjacency) {
  adjacency.clear();
  for (const ClusterEdge& e : g) {
    adjacency.insert(std::make_pair((uint32_t)e.a, (uint32_t)e.b));
    adjacency.insert(std::make_pair((uint32_t)e.b, (uint32_t)e.a));
  }
}
}  // namespace vgs_detail

template <typename PointT>
class VoxelBasedSegmentation {
 public:
  struct Weight_Index { float Weight; int Index; };                                     // VS:64-68
  static bool godown(const Weight_Index& a, const Weight_Index& b) { return a.Weight > b.Weight; }  // VS:70
  static bool riseup(const Weight_Index& a, const Weight_Index& b) { return a.Weight < b.Weight; }  // VS:76

  explicit VoxelBasedSegmentation(double input_resolution) {                              // VS:84
    vgs_params_default_vgs(&p_);
    p_.voxel_size = (float)input_resolution;
    vgs_ctx* c = nullptr;
    vgs_status s = vgs_create(&p_, &c);
    if (s != VGS_OK) throw std::runtime_error(std::string("vgs_create: ") + vgs_last_error_string(nullptr));
    ctx_.reset(c);
  }

  // inherited from pcl::octree::OctreePointCloud in the reference (test:52-56)
  void setInputCloud(const PCXYZPtr& cloud) { cloud_ = cloud; }
  void addPointsFromInputCloud() {
    if (!cloud_) throw std::runtime_error("addPointsFromInputCloud before setInputCloud");
    chk(vgs_set_points(ctx(), &cloud_->points[0].x, (int64_t)cloud_->points.size(), (int32_t)sizeof(PointT)), "vgs_set_points");
    chk(vgs_voxelize(ctx()), "vgs_voxelize");
    adj_off_.clear(); adj_idx_.clear();
  }
  void getBoundingBox(double& min_x, double& min_y, double& min_z, double& max_x, double& max_y, double& max_z) {
    double b[6];
    chk(vgs_get_bbox(ctx(), b), "vgs_get_bbox");
    min_x = b[0]; min_y = b[1]; min_z = b[2]; max_x = b[3]; max_y = b[4]; max_z = b[5];
  }

  int getCloudPointNum(const PCXYZPtr& input_data) { cloud_ = input_data; return (int)input_data->points.size(); }  // VS:94
  int getVoxelNum() { return (int)count(VGS_N_VOXELS); }                 // VS:104
  int getClusterNum() { return (int)count(VGS_N_CLUSTERS); }                              // VS:111
  std::vector<std::vector<int>> getClusterIdx() {                                        // VS:117
    std::vector<std::vector<int>> out;
    if (!drawn_) return out;  // clusters_point_idx_ is filled by drawColorMapofPointsinClusters only (VS:1006)
    const int64_t k = count(VGS_N_KEPT);
    std::vector<int64_t> off((size_t)k + 1);
    // element for element what the reference's clusters_point_idx_ holds: DFS order of the nodes, seed last
    chk(vgs_get_clusters_ordered(ctx(), VGS_ORDER_REFERENCE, off.data(), nullptr), "vgs_get_clusters");
    std::vector<int32_t> idx((size_t)off[k] + 1);
    chk(vgs_get_clusters_ordered(ctx(), VGS_ORDER_REFERENCE, off.data(), idx.data()), "vgs_get_clusters");
    out.resize((size_t)k);
    for (int64_t i = 0; i < k; ++i) out[(size_t)i].assign(idx.begin() + off[i], idx.begin() + off[i + 1]);
    return out;
  }

  // VS:124-131 only STORES its arguments: the octree keeps binning with the constructor's resolution (VS:84), and so does the
  // engine -- voxel_size is not forwarded.  The stored value is what the reference's debug meshes draw their boxes with
  // (VS:561-582) and what getVoxelCenterFromOctreeKey scales the keys by (VS:2106-2108); with a value other than the
  // constructor's the reference's centres no longer lie in their voxels, which the engine does not reproduce: its centres
  // are the octree's own ("setVoxelSize").
  void setVoxelSize(double input_resolution, int points_num_min, int voxels_num_min, int voxels_adj_min) {  // VS:124
    voxel_resolution_ = (float)input_resolution; p_.points_min = points_num_min; p_.voxels_min = voxels_num_min;
    p_.adjacency_min = voxels_adj_min;
    chk(vgs_set_params(ctx(), &p_), "vgs_set_params");
  }
  float getVoxelResolution() const { return voxel_resolution_ > 0.0f ? voxel_resolution_ : p_.voxel_size; }   // (debug meshes)
  void setBoundingBox(double, double, double, double, double, double) {}                 // VS:133 (the engine keeps the octree's box)
  // VS:146.  The voxel table is built by addPointsFromInputCloud with the constructor's resolution and stays as it is.
  void setVoxelCenters() {}   // (the table is built by addPointsFromInputCloud)
  std::vector<PointXYZ> getVoxelCenters() {                                              // VS:191
    const int64_t v = count(VGS_N_VOXELS);
    std::vector<float> c((size_t)v * 3 + 1);
    chk(vgs_get_voxel_centers(ctx(), c.data()), "vgs_get_voxel_centers");
    std::vector<PointXYZ> out((size_t)v);
    for (int64_t i = 0; i < v; ++i) out[(size_t)i] = PointXYZ(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
    return out;
  }
  void calcualteVoxelCloudAttributes(const PCXYZPtr&) { chk(vgs_features(ctx()), "vgs_features"); }  // VS:290 (sic)
  void findAllVoxelAdjacency(float graph_size) {                                         // VS:223
    p_.graph_size = graph_size;
    chk(vgs_set_params(ctx(), &p_), "vgs_set_params");
    chk(vgs_adjacency(ctx()), "vgs_adjacency");
    adj_off_.clear(); adj_idx_.clear();
  }
  std::vector<int> getOneVoxelAdjacency(int voxel_id) {                                  // VS:268
    // the reference keeps voxels_adjacency_idx_ in memory and a caller loops over the voxels: the lists are fetched once per
    // findAllVoxelAdjacency, not once per call
    if (adj_off_.empty()) {
      const int64_t v = count(VGS_N_VOXELS);
      adj_off_.assign((size_t)v + 1, 0);
      chk(vgs_get_lists(ctx(), 0, adj_off_.data(), nullptr), "vgs_get_lists");
      adj_idx_.assign((size_t)adj_off_[v] + 1, 0);
      chk(vgs_get_lists(ctx(), 0, adj_off_.data(), adj_idx_.data()), "vgs_get_lists");
    }
    if (voxel_id < 0 || (size_t)voxel_id + 1 >= adj_off_.size()) throw std::out_of_range("getOneVoxelAdjacency: voxel id");
    return std::vector<int>(adj_idx_.begin() + adj_off_[voxel_id], adj_idx_.begin() + adj_off_[voxel_id + 1]);
  }
  void segmentVoxelCloudWithGraphModel(float cut_thred, float sig_p, float sig_n, float sig_o, float sig_e, float sig_c,
                                       float sig_w) {                                    // VS:372
    p_.cut_thred = cut_thred; p_.sig_p = sig_p; p_.sig_n = sig_n; p_.sig_o = sig_o; p_.sig_e = sig_e; p_.sig_c = sig_c;
    p_.sig_w = sig_w;
    chk(vgs_set_params(ctx(), &p_), "vgs_set_params");
    chk(vgs_segment(ctx()), "vgs_segment");
  }
  // VS:947 "This is obligatory!": fills the per-cluster point lists; here it also returns one label per point
  std::vector<int32_t> drawColorMapofPointsinClusters() {
    std::vector<int32_t> lab((size_t)count(VGS_N_POINTS) + 1);
    chk(vgs_get_point_labels(ctx(), lab.data()), "vgs_get_point_labels");
    lab.pop_back();
    drawn_ = true;
    return lab;
  }
  // the reference's signature (VS:947): the kept clusters as a coloured cloud, one colour each (seeded palette)
  void drawColorMapofPointsinClusters(const PCXYZRGBPtr& colored_cloud, uint64_t seed = 0) {
    drawn_ = true;
    if (colored_cloud && cloud_) vgs_color::color_clusters(*cloud_, getClusterIdx(), seed, *colored_cloud);
  }
  // Extension (no VS line): descriptor i describes getClusterIdx()[i]; empty before drawColorMapofPointsinClusters, like getClusterIdx
  std::vector<ClusterDescriptor> getClusterDescriptors() {
    if (!drawn_) return {};
    return vgs_detail::cluster_descriptors(ctx(), count(VGS_N_KEPT));
  }
  // Extension (no VS line): box i bounds getClusterIdx()[i]; empty before drawColorMapofPointsinClusters, like getClusterDescriptors
  std::vector<ClusterBox> getClusterBoxes(int frame = VGS_BOX_PRINCIPAL) {
    if (!drawn_) return {};
    return vgs_detail::cluster_boxes(ctx(), count(VGS_N_KEPT), frame);
  }
  // Extension (no VS line): the adjacency graph of the kept clusters, indices as getClusterIdx; empty before drawColorMapofPointsinClusters
  std::vector<ClusterEdge> getClusterGraph() {
    if (!drawn_) return {};
    return vgs_detail::cluster_graph(ctx());
  }
  // Extension (no VS line): PCL's getSupervoxelAdjacency idiom over getClusterGraph -- both directions of every edge
  void getClusterAdjacency(std::multimap<uint32_t, uint32_t>& adjacency) { vgs_detail::cluster_adjacency(getClusterGraph(), adjacency); }
  // Extension (no VS line): row i reduces a per-point attribute (n rows of `channels` floats in input order, `stride_bytes` apart) over
  // getClusterIdx()[i]; empty before drawColorMapofPointsinClusters, like getClusterDescriptors
  std::vector<ClusterFieldStats> getClusterFieldStats(const float* field, int64_t n, int32_t channels, int64_t stride_bytes) {
    if (!drawn_) return {};
    return vgs_detail::cluster_field_stats(ctx(), count(VGS_N_KEPT), field, n, channels, stride_bytes);
  }
  // Extension (no VS line): row i counts a per-point class (n int32 in input order) over getClusterIdx()[i]; empty before
  // drawColorMapofPointsinClusters
  std::vector<ClusterClassHistogram> getClusterClassHistogram(const int32_t* classes, int64_t n, int32_t n_classes) {
    if (!drawn_) return {};
    return vgs_detail::cluster_class_histogram(ctx(), count(VGS_N_KEPT), classes, n, n_classes);
  }
  // Extension (no VS line): the clusters against a reference labelling (n int32 in input order, negative = no annotation); row i of the
  // cluster table belongs to getClusterIdx()[i]; empty before drawColorMapofPointsinClusters
  // labels != nullptr: that per-point labelling (n int32, the clusters' label range; refineClusterLabels()' result, say) is scored instead
  ClusterLabelComparison compareClusterLabels(const int32_t* ref, int64_t n, const int32_t* labels = nullptr) {
    if (!drawn_) return {};
    return vgs_detail::cluster_label_comparison(ctx(), count(VGS_N_KEPT), ref, n, labels);
  }
  // Extension (no VS line): the descriptors and boxes of a per-point labelling with the clusters' label range (n int32 in input order,
  // negative = no cluster; vgs_point_label_descriptors / _boxes, include/vgs.h): row i covers the points labelled i; *n_skipped = the
  // labelled points outside the octree.  Empty before drawColorMapofPointsinClusters
  std::vector<ClusterDescriptor> getLabelDescriptors(const int32_t* labels, int64_t n, int64_t* n_skipped = nullptr) {
    if (n_skipped) *n_skipped = 0;
    if (!drawn_) return {};
    return vgs_detail::cluster_descriptors(ctx(), count(VGS_N_KEPT), labels, n, n_skipped);
  }
  std::vector<ClusterBox> getLabelBoxes(const int32_t* labels, int64_t n, int frame = VGS_BOX_PRINCIPAL) {
    if (!drawn_) return {};
    return vgs_detail::cluster_boxes(ctx(), count(VGS_N_KEPT), frame, labels, n);
  }
  // Extension (no VS line): the field statistics and the class histogram of a per-point labelling (n int32 in input order, negative = no
  // row; vgs_point_label_field_stats / vgs_point_label_class_histogram, include/vgs.h): K rows, row i over the points labelled i; K < 0:
  // the clusters' label range; *n_skipped = the labelled points outside the octree.  Empty before drawColorMapofPointsinClusters
  std::vector<ClusterFieldStats> getLabelFieldStats(const int32_t* labels, const float* field, int64_t n, int32_t channels, int64_t stride_bytes,
                                                    int64_t K = -1, int64_t* n_skipped = nullptr) {
    if (n_skipped) *n_skipped = 0;
    if (!drawn_) return {};
    return vgs_detail::cluster_field_stats(ctx(), K < 0 ? count(VGS_N_KEPT) : K, field, n, channels, stride_bytes, labels, n_skipped);
  }
  std::vector<ClusterClassHistogram> getLabelClassHistogram(const int32_t* labels, const int32_t* classes, int64_t n, int32_t n_classes,
                                                            int64_t K = -1, int64_t* n_skipped = nullptr) {
    if (n_skipped) *n_skipped = 0;
    if (!drawn_) return {};
    return vgs_detail::cluster_class_histogram(ctx(), K < 0 ? count(VGS_N_KEPT) : K, classes, n, n_classes, labels, n_skipped);
  }

  // Extension (no VS line): the connected parts of a per-point labelling (n int32 in input order, negative = no label) over the voxel
  // adjacency (vgs_point_label_components, include/vgs.h); K < 0: the clusters' label range.  No part, every point -1, before
  // drawColorMapofPointsinClusters
  LabelComponents getLabelComponents(const int32_t* labels, int64_t n, int64_t K = -1) {
    if (!drawn_) {
      LabelComponents o;
      o.part_of_point.assign((size_t)count(VGS_N_POINTS), -1);
      o.label_first.assign(1, 0);
      return o;
    }
    return vgs_detail::label_components(ctx(), K < 0 ? count(VGS_N_KEPT) : K, labels, n);
  }
  // Extension (no VS line): the adjacency graph of a per-point labelling (vgs_point_label_graph, include/vgs.h), labels and K as
  // getLabelComponents.  No edge before drawColorMapofPointsinClusters
  LabelGraph getLabelGraph(const int32_t* labels, int64_t n, int64_t K = -1) {
    if (!drawn_) return {};
    return vgs_detail::label_graph(ctx(), K < 0 ? count(VGS_N_KEPT) : K, labels, n);
  }
  // Extension (no VS line): the labelling with its parts below min_points points -- below island_points for a part that is not the
  // largest of its label -- absorbed into the neighbour they touch most, for at most max_rounds rounds; drop: what is still too small
  // afterwards gets -1 (vgs_absorb_point_label_parts, include/vgs.h).  labels and K as getLabelComponents.  The labelling itself, no
  // round, before drawColorMapofPointsinClusters
  AbsorbedLabels absorbLabelParts(const int32_t* labels, int64_t n, int64_t min_points, int64_t island_points, int32_t max_rounds = 8,
                                  bool drop = false, int64_t K = -1) {
    if (!drawn_) { AbsorbedLabels o; o.labels.assign(labels, labels + (n > 0 ? n : 0)); return o; }
    return vgs_detail::absorb_label_parts(ctx(), K < 0 ? count(VGS_N_KEPT) : K, labels, n, min_points, island_points, max_rounds, drop);
  }

  // Extension (no VS line): one label per input point, refined at the cluster boundaries (vgs_refine_point_labels, include/vgs.h); label i
  // names getClusterIdx()[i].  patch_radius < 0: the default (the voxel size); every point -1 before drawColorMapofPointsinClusters
  std::vector<int32_t> refineClusterLabels(float patch_radius = -1.0f, float switch_ratio = 0.25f, bool fill = true) {
    if (!drawn_) return std::vector<int32_t>((size_t)count(VGS_N_POINTS), -1);
    return vgs_detail::refined_labels(ctx(), count(VGS_N_POINTS), patch_radius, switch_ratio, fill);
  }

  vgs_ctx* ctx() { return ctx_.get(); }

 private:
  void chk(vgs_status s, const char* what) { vgs_detail::check(ctx_.get(), s, what); }
  int64_t count(int which) {
    int64_t c[VGS_N_COUNTS];
    chk(vgs_get_counts(ctx(), c), "vgs_get_counts");
    return c[which];
  }
  vgs_params p_;
  std::unique_ptr<vgs_ctx, vgs_detail::CtxDeleter> ctx_;
  PCXYZPtr cloud_;
  bool drawn_ = false;
  float voxel_resolution_ = 0.0f;  // setVoxelSize's value (VS:127): stored, never binned with
  std::vector<int64_t> adj_off_;   // getOneVoxelAdjacency's copy of the lists
  std::vector<int32_t> adj_idx_;
};

template <typename PointT>
class SuperVoxelBasedSegmentation {
 public:
  explicit SuperVoxelBasedSegmentation(double input_resolution) {                         // SS:85
    vgs_params_default_svgs(&p_);
    p_.voxel_size = (float)input_resolution;
    vgs_ctx* c = nullptr;
    vgs_status s = vgs_create(&p_, &c);
    if (s != VGS_OK) throw std::runtime_error(std::string("vgs_create: ") + vgs_last_error_string(nullptr));
    ctx_.reset(c);
  }
  void setInputCloud(const PCXYZPtr& cloud) { cloud_ = cloud; }
  void addPointsFromInputCloud() {                                                       // test:142 (own octree: bookkeeping only)
    if (!cloud_) throw std::runtime_error("addPointsFromInputCloud before setInputCloud");
    chk(vgs_set_points(ctx(), &cloud_->points[0].x, (int64_t)cloud_->points.size(), (int32_t)sizeof(PointT)), "vgs_set_points");
  }
  int getCloudPointNum(const PCXYZPtr& input_data) { cloud_ = input_data; return (int)input_data->points.size(); }  // SS:101
  int getVoxelNum() { return (int)count(VGS_N_VOXELS); }                                  // SS:111
  int getSuperVoxelNum() { return (int)count(VGS_N_SUPERVOXELS); }                        // SS:118
  int getClusterNum() { return (int)count(VGS_N_CLUSTERS); }                              // SS:124
  std::vector<std::vector<int>> getClusterIdx() {                                        // SS:130 (no draw call needed, SS:2124)
    const int64_t k = count(VGS_N_KEPT);
    std::vector<int64_t> off((size_t)k + 1);
    // element for element what the reference's clusters_point_idx_ holds: DFS order of the nodes, seed last
    chk(vgs_get_clusters_ordered(ctx(), VGS_ORDER_REFERENCE, off.data(), nullptr), "vgs_get_clusters");
    std::vector<int32_t> idx((size_t)off[k] + 1);
    chk(vgs_get_clusters_ordered(ctx(), VGS_ORDER_REFERENCE, off.data(), idx.data()), "vgs_get_clusters");
    std::vector<std::vector<int>> out((size_t)k);
    for (int64_t i = 0; i < k; ++i) out[(size_t)i].assign(idx.begin() + off[i], idx.begin() + off[i + 1]);
    return out;
  }
  void setVoxelSize(double input_resolution, int points_num_min) {                       // SS:143
    p_.voxel_size = (float)input_resolution; p_.points_min = points_num_min;
    chk(vgs_set_params(ctx(), &p_), "vgs_set_params");
  }
  void setSupervoxelSize(double input_resolution, int voxels_num_min, int, int adjacency_num_min) {  // SS:150
    p_.seed_size = (float)input_resolution; p_.voxels_min = voxels_num_min; p_.adjacency_min = adjacency_num_min;
    chk(vgs_set_params(ctx(), &p_), "vgs_set_params");
  }
  void setGraphSize(double /*small_resolution: consumed nowhere, SS:1438-1475*/, double large_resolution) {  // SS:159
    p_.graph_size = (float)large_resolution;
    chk(vgs_set_params(ctx(), &p_), "vgs_set_params");
  }
  void getBoundingBox(double& min_x, double& min_y, double& min_z, double& max_x, double& max_y, double& max_z) {  // test:145 (inherited from the octree)
    double b[6];
    chk(vgs_voxelize(ctx()), "vgs_voxelize");   // the class's own octree at voxel_resolution_
    chk(vgs_get_bbox(ctx(), b), "vgs_get_bbox");
    min_x = b[0]; min_y = b[1]; min_z = b[2]; max_x = b[3]; max_y = b[4]; max_z = b[5];
  }
  void setBoundingBox(double, double, double, double, double, double) {}                 // SS:166
  void setSupervoxelCentersCentroids() {}                                                // SS:178 (own-octree bookkeeping, unused by the result)
  // the supervoxel labelling pcl::SupervoxelClustering would produce may also be supplied by the caller
  void setSupervoxelLabels(const std::vector<int32_t>& labels, int max_label) {
    chk(svgs_set_supervoxel_labels(ctx(), labels.data(), max_label), "svgs_set_supervoxel_labels");
  }
  void segmentSupervoxelCloudWithGraphModel(float sig_a, float sig_b, float sig_l, float cut_thred, float sig_p, float sig_n,
                                            float sig_o, float sig_e, float sig_c, float sig_w) {  // SS:362
    p_.color_impt = sig_a; p_.spatial_impt = sig_b; p_.normal_impt = sig_l; p_.cut_thred = cut_thred;
    p_.sig_p = sig_p; p_.sig_n = sig_n; p_.sig_o = sig_o; p_.sig_e = sig_e; p_.sig_c = sig_c; p_.sig_w = sig_w;
    chk(vgs_set_params(ctx(), &p_), "vgs_set_params");
    chk(vgs_run(ctx()), "vgs_run");  // createSupervoxels (unless the caller's labelling of THIS cloud is in place), then the graph stages
  }
  std::vector<int32_t> drawColorMapofPointsinClusters() {                                // SS:613
    std::vector<int32_t> lab((size_t)count(VGS_N_POINTS) + 1);
    chk(vgs_get_point_labels(ctx(), lab.data()), "vgs_get_point_labels");
    lab.pop_back();
    return lab;
  }
  void drawColorMapofPointsinClusters(const PCXYZRGBPtr& colored_cloud, uint64_t seed = 0) {  // the reference's signature (SS:613)
    if (colored_cloud && cloud_) vgs_color::color_clusters(*cloud_, getClusterIdx(), seed, *colored_cloud);
  }
  // Extension (no SS line): descriptor i describes getClusterIdx()[i]
  std::vector<ClusterDescriptor> getClusterDescriptors() { return vgs_detail::cluster_descriptors(ctx(), count(VGS_N_KEPT)); }
  // Extension (no SS line): box i bounds getClusterIdx()[i]
  std::vector<ClusterBox> getClusterBoxes(int frame = VGS_BOX_PRINCIPAL) { return vgs_detail::cluster_boxes(ctx(), count(VGS_N_KEPT), frame); }
  // Extension (no SS line): the adjacency graph of the kept clusters, indices as getClusterIdx
  std::vector<ClusterEdge> getClusterGraph() { return vgs_detail::cluster_graph(ctx()); }
  // Extension (no SS line): PCL's getSupervoxelAdjacency idiom over getClusterGraph -- both directions of every edge
  void getClusterAdjacency(std::multimap<uint32_t, uint32_t>& adjacency) { vgs_detail::cluster_adjacency(getClusterGraph(), adjacency); }
  // Extension (no SS line): row i reduces a per-point attribute (n rows of `channels` floats in input order, `stride_bytes` apart) over
  // getClusterIdx()[i]
  std::vector<ClusterFieldStats> getClusterFieldStats(const float* field, int64_t n, int32_t channels, int64_t stride_bytes) {
    return vgs_detail::cluster_field_stats(ctx(), count(VGS_N_KEPT), field, n, channels, stride_bytes);
  }
  // Extension (no SS line): row i counts a per-point class (n int32 in input order) over getClusterIdx()[i]
  std::vector<ClusterClassHistogram> getClusterClassHistogram(const int32_t* classes, int64_t n, int32_t n_classes) {
    return vgs_detail::cluster_class_histogram(ctx(), count(VGS_N_KEPT), classes, n, n_classes);
  }
  // Extension (no SS line): the clusters against a reference labelling (n int32 in input order, negative = no annotation); row i of the
  // cluster table belongs to getClusterIdx()[i]
  // labels != nullptr: that per-point labelling (n int32, the clusters' label range; refineClusterLabels()' result, say) is scored instead
  ClusterLabelComparison compareClusterLabels(const int32_t* ref, int64_t n, const int32_t* labels = nullptr) {
    return vgs_detail::cluster_label_comparison(ctx(), count(VGS_N_KEPT), ref, n, labels);
  }
  // Extension (no SS line): the descriptors and boxes of a per-point labelling with the clusters' label range (n int32 in input order,
  // negative = no cluster; vgs_point_label_descriptors / _boxes, include/vgs.h): row i covers the points labelled i; *n_skipped = the
  // labelled points outside the octree
  std::vector<ClusterDescriptor> getLabelDescriptors(const int32_t* labels, int64_t n, int64_t* n_skipped = nullptr) {
    if (n_skipped) *n_skipped = 0;
    return vgs_detail::cluster_descriptors(ctx(), count(VGS_N_KEPT), labels, n, n_skipped);
  }
  std::vector<ClusterBox> getLabelBoxes(const int32_t* labels, int64_t n, int frame = VGS_BOX_PRINCIPAL) {
    return vgs_detail::cluster_boxes(ctx(), count(VGS_N_KEPT), frame, labels, n);
  }
  // Extension (no SS line): the field statistics and the class histogram of a per-point labelling (n int32 in input order, negative = no
  // row; vgs_point_label_field_stats / vgs_point_label_class_histogram, include/vgs.h): K rows, row i over the points labelled i; K < 0:
  // the clusters' label range; *n_skipped = the labelled points outside the octree
  std::vector<ClusterFieldStats> getLabelFieldStats(const int32_t* labels, const float* field, int64_t n, int32_t channels, int64_t stride_bytes,
                                                    int64_t K = -1, int64_t* n_skipped = nullptr) {
    if (n_skipped) *n_skipped = 0;
    return vgs_detail::cluster_field_stats(ctx(), K < 0 ? count(VGS_N_KEPT) : K, field, n, channels, stride_bytes, labels, n_skipped);
  }
  std::vector<ClusterClassHistogram> getLabelClassHistogram(const int32_t* labels, const int32_t* classes, int64_t n, int32_t n_classes,
                                                            int64_t K = -1, int64_t* n_skipped = nullptr) {
    if (n_skipped) *n_skipped = 0;
    return vgs_detail::cluster_class_histogram(ctx(), K < 0 ? count(VGS_N_KEPT) : K, classes, n, n_classes, labels, n_skipped);
  }
  // Extension (no SS line): the connected parts of a per-point labelling (n int32 in input order, negative = no label) over the supervoxel
  // adjacency (vgs_point_label_components, include/vgs.h); K < 0: the clusters' label range
  LabelComponents getLabelComponents(const int32_t* labels, int64_t n, int64_t K = -1) {
    return vgs_detail::label_components(ctx(), K < 0 ? count(VGS_N_KEPT) : K, labels, n);
  }
  // Extension (no SS line): the adjacency graph of a per-point labelling (vgs_point_label_graph, include/vgs.h), labels and K as
  // getLabelComponents
  LabelGraph getLabelGraph(const int32_t* labels, int64_t n, int64_t K = -1) {
    return vgs_detail::label_graph(ctx(), K < 0 ? count(VGS_N_KEPT) : K, labels, n);
  }
  // Extension (no SS line): the labelling with its small parts absorbed into the neighbour they touch most
  // (vgs_absorb_point_label_parts, include/vgs.h), labels and K as getLabelComponents
  AbsorbedLabels absorbLabelParts(const int32_t* labels, int64_t n, int64_t min_points, int64_t island_points, int32_t max_rounds = 8,
                                  bool drop = false, int64_t K = -1) {
    return vgs_detail::absorb_label_parts(ctx(), K < 0 ? count(VGS_N_KEPT) : K, labels, n, min_points, island_points, max_rounds, drop);
  }
  // Extension (no SS line): one label per input point, refined at the cluster boundaries (vgs_refine_point_labels, include/vgs.h); label i
  // names getClusterIdx()[i].  patch_radius < 0: the default (the supervoxel size)
  std::vector<int32_t> refineClusterLabels(float patch_radius = -1.0f, float switch_ratio = 0.25f, bool fill = true) {
    return vgs_detail::refined_labels(ctx(), count(VGS_N_POINTS), patch_radius, switch_ratio, fill);
  }
  vgs_ctx* ctx() { return ctx_.get(); }

 private:
  void chk(vgs_status s, const char* what) { vgs_detail::check(ctx_.get(), s, what); }
  int64_t count(int which) {
    int64_t c[VGS_N_COUNTS];
    chk(vgs_get_counts(ctx(), c), "vgs_get_counts");
    return c[which];
  }
  vgs_params p_;
  std::unique_ptr<vgs_ctx, vgs_detail::CtxDeleter> ctx_;
  PCXYZPtr cloud_;
};

}  // namespace pcl

#endif  // VGS_SEGMENTATION_HPP_
