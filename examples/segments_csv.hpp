// examples/segments_csv.hpp -- the --segments CSV of the front ends (vgs_run, vgs_tiles_run): one row per kept cluster, row i = cluster
// i (label i): label, n_points, n_nodes, bbox (6), centroid (3), eigenvalues (3, ascending), normal (3), major axis (3), the eight eigen
// features -- doubles as %.17g, floats as %.9g, so every value reads back exactly.  One writer, so the two front ends cannot drift apart.
// The --segment-graph CSV of the same front ends: one row per edge, ascending (a, b): a, b, n_pairs, n_finite, nodes_a, nodes_b, w_mean
// (w_sum / n_finite, NaN without a finite weight), w_min, w_max.
// The --segment-boxes CSV of vgs_run: one row per kept cluster, row i = cluster i: label, center (3), half (3), frame (9: [r*3+j] =
// component r of axis j), lo (3), hi (3), every value as %.17g.
// The --segment-fields CSV of vgs_run: one row per kept cluster: label, then per field n_valid, mean, var (%.17g), min, max (%.9g); the
// --segment-classes CSV: label, majority, majority_count, n_outside, hist_0 .. hist_{C-1}.
// The --segment-matches CSV of vgs_run: one row per kept cluster: label, n_annotated, n_refs, best_ref, best_n, best_iou (%.17g); the
// --truth-matches CSV: one row per reference id: ref_id, n_points, n_dropped, best_seg, best_n, best_iou (%.17g).
#ifndef VGS_EXAMPLES_SEGMENTS_CSV_HPP_
#define VGS_EXAMPLES_SEGMENTS_CSV_HPP_

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "vgs_segmentation.hpp"

inline int writeSegmentsCsv(const std::string& path, const std::vector<pcl::ClusterDescriptor>& desc) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "label,n_points,n_nodes,min_x,min_y,min_z,max_x,max_y,max_z,cx,cy,cz,l0,l1,l2,nx,ny,nz,ax,ay,az,"
                  "f0,f1,f2,f3,f4,f5,f6,f7\n");
  for (size_t i = 0; i < desc.size(); ++i) {
    const pcl::ClusterDescriptor& d = desc[i];
    std::fprintf(f, "%zu,%lld,%d", i, (long long)d.n_points, (int)d.n_nodes);
    for (int a = 0; a < 6; ++a) std::fprintf(f, ",%.9g", (double)d.bbox[a]);
    for (int a = 0; a < 3; ++a) std::fprintf(f, ",%.17g", d.centroid[a]);
    for (int a = 0; a < 3; ++a) std::fprintf(f, ",%.17g", d.evals[a]);
    for (int r = 0; r < 3; ++r) std::fprintf(f, ",%.17g", d.evecs[3 * r + 0]);   // normal: eigenvector of the smallest eigenvalue
    for (int r = 0; r < 3; ++r) std::fprintf(f, ",%.17g", d.evecs[3 * r + 2]);   // major axis: eigenvector of the largest
    for (int a = 0; a < 8; ++a) std::fprintf(f, ",%.9g", (double)d.eigen8[a]);
    std::fprintf(f, "\n");
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

inline int writeGraphCsv(const std::string& path, const std::vector<pcl::ClusterEdge>& g) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "a,b,n_pairs,n_finite,nodes_a,nodes_b,w_mean,w_min,w_max\n");
  for (const pcl::ClusterEdge& e : g) {
    const double mean = e.n_finite > 0 ? e.w_sum / (double)e.n_finite : std::nan("");
    std::fprintf(f, "%d,%d,%lld,%lld,%d,%d,%.17g,%.9g,%.9g\n", (int)e.a, (int)e.b, (long long)e.n_pairs, (long long)e.n_finite, (int)e.nodes_a,
                 (int)e.nodes_b, mean, (double)e.w_min, (double)e.w_max);
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

// the --refined-graph / --class-graph CSV of vgs_run: one row per edge of the adjacency graph of a per-point labelling (getLabelGraph),
// ascending (a, b): the columns of --segment-graph plus n_shared behind b
inline int writeLabelGraphCsv(const std::string& path, const pcl::LabelGraph& g) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "a,b,n_shared,n_pairs,n_finite,nodes_a,nodes_b,w_mean,w_min,w_max\n");
  for (const pcl::LabelEdge& e : g.edges) {
    const double mean = e.n_finite > 0 ? e.w_sum / (double)e.n_finite : std::nan("");
    std::fprintf(f, "%d,%d,%lld,%lld,%lld,%d,%d,%.17g,%.9g,%.9g\n", (int)e.a, (int)e.b, (long long)e.n_shared, (long long)e.n_pairs,
                 (long long)e.n_finite, (int)e.nodes_a, (int)e.nodes_b, mean, (double)e.w_min, (double)e.w_max);
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

inline int writeBoxesCsv(const std::string& path, const std::vector<pcl::ClusterBox>& boxes) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "label,cx,cy,cz,hx,hy,hz,w00,w01,w02,w10,w11,w12,w20,w21,w22,lo0,lo1,lo2,hi0,hi1,hi2\n");
  for (size_t i = 0; i < boxes.size(); ++i) {
    const pcl::ClusterBox& b = boxes[i];
    std::fprintf(f, "%zu", i);
    for (int a = 0; a < 3; ++a) std::fprintf(f, ",%.17g", b.center[a]);
    for (int a = 0; a < 3; ++a) std::fprintf(f, ",%.17g", b.half[a]);
    for (int a = 0; a < 9; ++a) std::fprintf(f, ",%.17g", b.frame[a]);
    for (int a = 0; a < 3; ++a) std::fprintf(f, ",%.17g", b.lo[a]);
    for (int a = 0; a < 3; ++a) std::fprintf(f, ",%.17g", b.hi[a]);
    std::fprintf(f, "\n");
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

// the same rows for the parts of a labelling over the ranks of the tiled driver (vgs_tiles_get_point_label_components): the shared-grid code
// of the part's first node in place of the node id, which means nothing across ranks
inline int writeTileComponentsCsv(const std::string& path, const std::vector<int32_t>& part_label, const std::vector<int64_t>& part_points,
                                  const std::vector<int32_t>& part_nodes, const std::vector<uint64_t>& part_first_code,
                                  const std::vector<int32_t>& label_largest) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "part,label,n_points,n_nodes,first_code,largest\n");
  for (size_t p = 0; p < part_label.size(); ++p) {
    const int32_t l = part_label[p];
    const bool largest = l >= 0 && (size_t)l < label_largest.size() && label_largest[(size_t)l] == (int32_t)p;
    std::fprintf(f, "%zu,%d,%lld,%d,%llu,%d\n", p, (int)l, (long long)part_points[p], (int)part_nodes[p], (unsigned long long)part_first_code[p], largest ? 1 : 0);
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

// one row per connected part of a labelling (getLabelComponents), in part order: part, label, n_points, n_nodes, first_node, and
// largest = 1 for the part with the most points of its label
inline int writeComponentsCsv(const std::string& path, const pcl::LabelComponents& c) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "part,label,n_points,n_nodes,first_node,largest\n");
  for (size_t p = 0; p < c.part_label.size(); ++p) {
    const int32_t l = c.part_label[p];
    const bool largest = l >= 0 && (size_t)l < c.label_largest.size() && c.label_largest[(size_t)l] == (int32_t)p;
    std::fprintf(f, "%zu,%d,%lld,%d,%d,%d\n", p, (int)l, (long long)c.part_points[p], (int)c.part_nodes[p], (int)c.part_first_node[p], largest ? 1 : 0);
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

inline int writeFieldStatsCsv(const std::string& path, const std::vector<std::string>& names, const std::vector<pcl::ClusterFieldStats>& stats) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "label");
  for (const std::string& n : names) std::fprintf(f, ",%s_n_valid,%s_mean,%s_var,%s_min,%s_max", n.c_str(), n.c_str(), n.c_str(), n.c_str(), n.c_str());
  std::fprintf(f, "\n");
  for (size_t i = 0; i < stats.size(); ++i) {
    const pcl::ClusterFieldStats& s = stats[i];
    std::fprintf(f, "%zu", i);
    for (size_t c = 0; c < names.size() && c < s.n_valid.size(); ++c)
      std::fprintf(f, ",%lld,%.17g,%.17g,%.9g,%.9g", (long long)s.n_valid[c], s.mean[c], s.var[c], (double)s.vmin[c], (double)s.vmax[c]);
    std::fprintf(f, "\n");
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

inline int writeClassHistCsv(const std::string& path, int n_classes, const std::vector<pcl::ClusterClassHistogram>& hist) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "label,majority,majority_count,n_outside");
  for (int j = 0; j < n_classes; ++j) std::fprintf(f, ",hist_%d", j);
  std::fprintf(f, "\n");
  for (size_t i = 0; i < hist.size(); ++i) {
    const pcl::ClusterClassHistogram& h = hist[i];
    std::fprintf(f, "%zu,%d,%lld,%lld", i, (int)h.majority, (long long)h.majority_count, (long long)h.n_outside);
    for (int64_t v : h.hist) std::fprintf(f, ",%lld", (long long)v);
    std::fprintf(f, "\n");
  }
  return std::fclose(f) == 0 ? 0 : -1;
}

inline int writeSegmentMatchesCsv(const std::string& path, const pcl::ClusterLabelComparison& m) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "label,n_annotated,n_refs,best_ref,best_n,best_iou\n");
  for (size_t i = 0; i < m.seg_annotated.size(); ++i)
    std::fprintf(f, "%zu,%lld,%d,%d,%lld,%.17g\n", i, (long long)m.seg_annotated[i], (int)m.seg_refs[i], (int)m.seg_best_ref[i],
                 (long long)m.seg_best_n[i], m.seg_best_iou[i]);
  return std::fclose(f) == 0 ? 0 : -1;
}

inline int writeTruthMatchesCsv(const std::string& path, const pcl::ClusterLabelComparison& m) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  std::fprintf(f, "ref_id,n_points,n_dropped,best_seg,best_n,best_iou\n");
  for (size_t i = 0; i < m.ref_id.size(); ++i)
    std::fprintf(f, "%d,%lld,%lld,%d,%lld,%.17g\n", (int)m.ref_id[i], (long long)m.ref_points[i], (long long)m.ref_dropped[i],
                 (int)m.ref_best_seg[i], (long long)m.ref_best_n[i], m.ref_best_iou[i]);
  return std::fclose(f) == 0 ? 0 : -1;
}

#endif  // VGS_EXAMPLES_SEGMENTS_CSV_HPP_
