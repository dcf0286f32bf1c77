// examples/drivers.hpp -- the reference's two drivers (`test`:9-86 segmentationVGS, `test`:91-170 segmentationSVGS)
// written against include/vgs_segmentation.hpp: same objects, same call order, same parameter unpacking from the
// task vector (0-based line index).  The viewer calls (showColoredClusters) are dropped; saving is left to the caller.
#ifndef VGS_EXAMPLE_DRIVERS_HPP_
#define VGS_EXAMPLE_DRIVERS_HPP_

#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "vgs_segmentation.hpp"
#include "vgs_debug_export.hpp"

struct DriverSummary { long points = 0, voxels = 0, supervoxels = 0, clusters = 0, kept = 0, labelled = 0; };
// what the drivers hand back of the cluster adjacency graph: getClusterGraph() and getClusterAdjacency() of the same run
struct DriverGraph {
  std::vector<pcl::ClusterEdge> edges;
  std::multimap<uint32_t, uint32_t> adjacency;
};

// absorbLabelParts over a labelling the drivers hold (the refined labels, or the class field of DriverFields) when `on`
struct DriverAbsorb {
  bool on = false;
  int64_t min_points = 0, island_points = 0;
  int32_t max_rounds = 8;
  bool drop = false;
  pcl::AbsorbedLabels out;
};

// per-point attributes handed to the drivers and what comes back: getClusterFieldStats over `field` (n x channels floats, row-major) when
// channels > 0, getClusterClassHistogram over `classes` (n int32) when n_classes > 0, compareClusterLabels over `truth` when have_truth;
// want_stats / want_hist off: the input is loaded for the refined labels' table only (DriverRefine::fields); getLabelComponents over
// `part_classes` (n int32, negative = no class) with parts_K labels when parts_K >= 0, getLabelGraph over the same when want_parts_graph,
// absorbLabelParts over the same when absorb.on
struct DriverFields {
  std::vector<float> field;
  int channels = 0;
  std::vector<int32_t> classes;
  int n_classes = 0;
  bool want_stats = true, want_hist = true;
  std::vector<pcl::ClusterFieldStats> stats;
  std::vector<pcl::ClusterClassHistogram> hist;
  // a reference labelling (n int32, negative = no annotation) when have_truth, and compareClusterLabels over it
  std::vector<int32_t> truth;
  bool have_truth = false;
  pcl::ClusterLabelComparison matches;
  std::vector<int32_t> part_classes;
  int64_t parts_K = -1;
  pcl::LabelComponents parts;
  bool want_parts = true, want_parts_graph = false;
  pcl::LabelGraph parts_graph;
  DriverAbsorb absorb;
};
// point-level refinement of the cluster labels (refineClusterLabels): when `on`, the drivers put the refined clusters into
// clusters_points_idx -- clusters in label order, points in ascending index -- and the refined labels into `labels`
struct DriverRefine {
  bool on = false;
  float patch_radius = -1.0f;   // < 0: the default
  float switch_ratio = 0.25f;
  bool fill = true;
  std::vector<int32_t> labels;
  // the tables of the REFINED labels, beside the ones that describe the voxel labels: getLabelDescriptors / getLabelBoxes(box_frame) /
  // compareClusterLabels(truth, labels) when wanted (truth: n int32, not null); getLabelFieldStats / getLabelClassHistogram over the
  // field / classes of `fields` when wanted; getLabelComponents and getLabelGraph when wanted; absorbLabelParts when absorb.on (last:
  // every table above describes the refined labels themselves)
  bool want_descriptors = false, want_boxes = false, want_stats = false, want_hist = false, want_components = false, want_graph = false;
  pcl::LabelComponents components;
  pcl::LabelGraph graph;
  DriverAbsorb absorb;
  const DriverFields* fields = nullptr;
  std::vector<pcl::ClusterFieldStats> stats;
  std::vector<pcl::ClusterClassHistogram> hist;
  int box_frame = VGS_BOX_PRINCIPAL;
  const std::vector<int32_t>* truth = nullptr;
  std::vector<pcl::ClusterDescriptor> descriptors;
  std::vector<pcl::ClusterBox> boxes;
  pcl::ClusterLabelComparison matches;
};
template <typename S>
inline void driverRefine(S& structure, DriverRefine& r, std::vector<std::vector<int>>& clusters_points_idx) {
  r.labels = structure.refineClusterLabels(r.patch_radius, r.switch_ratio, r.fill);
  const int64_t n = (int64_t)r.labels.size();
  if (r.want_descriptors) r.descriptors = structure.getLabelDescriptors(r.labels.data(), n);
  if (r.want_boxes) r.boxes = structure.getLabelBoxes(r.labels.data(), n, r.box_frame);
  if (r.truth) r.matches = structure.compareClusterLabels(r.truth->data(), (int64_t)r.truth->size(), r.labels.data());
  if (r.want_stats && r.fields && r.fields->channels > 0)
    r.stats = structure.getLabelFieldStats(r.labels.data(), r.fields->field.data(), (int64_t)(r.fields->field.size() / (size_t)r.fields->channels),
                                           r.fields->channels, 4 * (int64_t)r.fields->channels);
  if (r.want_hist && r.fields && r.fields->n_classes > 0)
    r.hist = structure.getLabelClassHistogram(r.labels.data(), r.fields->classes.data(), (int64_t)r.fields->classes.size(), r.fields->n_classes);
  if (r.want_components) r.components = structure.getLabelComponents(r.labels.data(), n);
  if (r.want_graph) r.graph = structure.getLabelGraph(r.labels.data(), n);
  if (r.absorb.on)
    r.absorb.out = structure.absorbLabelParts(r.labels.data(), n, r.absorb.min_points, r.absorb.island_points, r.absorb.max_rounds, r.absorb.drop);
  for (auto& c : clusters_points_idx) c.clear();
  for (size_t i = 0; i < r.labels.size(); ++i)
    if (r.labels[i] >= 0 && (size_t)r.labels[i] < clusters_points_idx.size()) clusters_points_idx[(size_t)r.labels[i]].push_back((int)i);
}
template <typename S>
inline void driverFields(S& structure, DriverFields& f) {
  if (f.channels > 0 && f.want_stats)
    f.stats = structure.getClusterFieldStats(f.field.data(), (int64_t)(f.field.size() / (size_t)f.channels), f.channels, 4 * (int64_t)f.channels);
  if (f.n_classes > 0 && f.want_hist) f.hist = structure.getClusterClassHistogram(f.classes.data(), (int64_t)f.classes.size(), f.n_classes);
  if (f.have_truth) f.matches = structure.compareClusterLabels(f.truth.data(), (int64_t)f.truth.size());
  if (f.parts_K >= 0 && f.want_parts) f.parts = structure.getLabelComponents(f.part_classes.data(), (int64_t)f.part_classes.size(), f.parts_K);
  if (f.parts_K >= 0 && f.want_parts_graph) f.parts_graph = structure.getLabelGraph(f.part_classes.data(), (int64_t)f.part_classes.size(), f.parts_K);
  if (f.parts_K >= 0 && f.absorb.on)
    f.absorb.out = structure.absorbLabelParts(f.part_classes.data(), (int64_t)f.part_classes.size(), f.absorb.min_points, f.absorb.island_points,
                                              f.absorb.max_rounds, f.absorb.drop, f.parts_K);
}

// debug_prefix: when not empty, the reference's three voxel drawings (VS:510, 654, 1016) are written as
// <prefix>_voxels.ply, <prefix>_clustered_voxels.ply, <prefix>_normals.ply
// descriptors: when not null, receives getClusterDescriptors() (one per entry of clusters_points_idx, same order)
// graph: when not null, receives getClusterGraph() and getClusterAdjacency() (cluster indices of clusters_points_idx)
// boxes: when not null, receives getClusterBoxes(box_frame) (one per entry of clusters_points_idx, same order)
// fields: when not null, its stats / hist receive getClusterFieldStats / getClusterClassHistogram of its inputs (same order)
// refine: when not null and on, clusters_points_idx holds the clusters of refineClusterLabels instead of getClusterIdx's (the tables above
// keep describing the voxel labels)
inline int segmentationVGS(PCXYZPtr input_cloud, const std::vector<std::string>& input_vector,
                           std::vector<std::vector<int>>& clusters_points_idx, DriverSummary* sum = nullptr,
                           const std::string& debug_prefix = std::string(), double ctor_resolution = 0.0,
                           std::vector<pcl::ClusterDescriptor>* descriptors = nullptr, DriverGraph* graph = nullptr,
                           std::vector<pcl::ClusterBox>* boxes = nullptr, int box_frame = VGS_BOX_PRINCIPAL,
                           DriverFields* fields = nullptr, DriverRefine* refine = nullptr) {
  float voxel_size = 0.15f, graph_size = 0.5f, sig_p = 0.2f, sig_n = 0.2f, sig_o = 0.2f, sig_e = 0.2f, sig_c = 0.2f, sig_w = 2.0f,
        cut_thred = 0.3f;
  int points_min = 10, adjacency_min = 3, voxels_min = 3;
  if (input_vector.size() > 50) {  // the twelve numbers sit on every second line from 28 on (test:25-37)
    auto num = [&](size_t line) { return std::atof(input_vector[line].c_str()); };
    float* const f[] = {&voxel_size, &graph_size, &sig_p, &sig_n, &sig_o, &sig_e, &sig_c, &sig_w, &cut_thred};
    for (size_t k = 0; k < 9; ++k) *f[k] = (float)num(28 + 2 * k);
    points_min = (int)num(46); adjacency_min = (int)num(48); voxels_min = (int)num(50);
  }
  double min_x = 0, min_y = 0, min_z = 0, max_x = 0, max_y = 0, max_z = 0;

  // Voxelization (test:51-57)
  // (ctor_resolution: tests only -- an octree resolution that differs from the one setVoxelSize is given afterwards)
  pcl::VoxelBasedSegmentation<pcl::PointXYZ> voxel_structure(ctor_resolution > 0.0 ? ctor_resolution : (double)voxel_size);
  voxel_structure.setInputCloud(input_cloud);
  voxel_structure.getCloudPointNum(input_cloud);
  voxel_structure.addPointsFromInputCloud();
  voxel_structure.setVoxelSize(voxel_size, points_min, voxels_min, adjacency_min);
  voxel_structure.getBoundingBox(min_x, min_y, min_z, max_x, max_y, max_z);
  voxel_structure.setBoundingBox(min_x, min_y, min_z, max_x, max_y, max_z);
  // centres (test:60-62)
  voxel_structure.setVoxelCenters();
  auto voxel_centers = voxel_structure.getVoxelCenters();
  const int voxels = voxel_structure.getVoxelNum();
  // features, adjacency, segmentation (test:65-71)
  voxel_structure.calcualteVoxelCloudAttributes(input_cloud);
  voxel_structure.findAllVoxelAdjacency(graph_size);
  voxel_structure.segmentVoxelCloudWithGraphModel(cut_thred, sig_p, sig_n, sig_o, sig_e, sig_c, sig_w);
  // output (test:74-76)
  PCXYZRGBPtr clustered_cloud(new PCXYZRGB);
  voxel_structure.drawColorMapofPointsinClusters(clustered_cloud);
  clusters_points_idx = voxel_structure.getClusterIdx();
  if (descriptors) *descriptors = voxel_structure.getClusterDescriptors();
  if (graph) { graph->edges = voxel_structure.getClusterGraph(); voxel_structure.getClusterAdjacency(graph->adjacency); }
  if (boxes) *boxes = voxel_structure.getClusterBoxes(box_frame);
  if (fields) driverFields(voxel_structure, *fields);
  if (refine && refine->on) driverRefine(voxel_structure, *refine, clusters_points_idx);
  if (sum) {
    sum->points = (long)input_cloud->points.size(); sum->voxels = voxels; sum->clusters = voxel_structure.getClusterNum();
    sum->kept = (long)clusters_points_idx.size();
    sum->labelled = 0;
    for (auto& c : clusters_points_idx) sum->labelled += (long)c.size();
  }
  (void)voxel_centers;
  if (!debug_prefix.empty()) {
    pcl::PolygonMesh::Ptr colored_voxels(new pcl::PolygonMesh), clustered_voxels(new pcl::PolygonMesh), normes_voxels(new pcl::PolygonMesh);
    drawColorMapofVoxels(voxel_structure.ctx(), voxel_size, colored_voxels);
    drawColorMapofClusteredVoxels(voxel_structure.ctx(), voxel_size, clustered_voxels);
    drawNormofVoxels(voxel_structure.ctx(), voxel_size, normes_voxels);
    if (savePolygonMeshPLY(debug_prefix + "_voxels.ply", *colored_voxels) != 0 ||
        savePolygonMeshPLY(debug_prefix + "_clustered_voxels.ply", *clustered_voxels) != 0 ||
        savePolygonMeshPLY(debug_prefix + "_normals.ply", *normes_voxels) != 0)
      return -1;
  }
  return 0;
}

inline int segmentationSVGS(PCXYZPtr input_cloud, const std::vector<std::string>& input_vector,
                            std::vector<std::vector<int>>& clusters_points_idx, DriverSummary* sum = nullptr,
                            std::vector<pcl::ClusterDescriptor>* descriptors = nullptr, DriverGraph* graph = nullptr,
                            std::vector<pcl::ClusterBox>* boxes = nullptr, int box_frame = VGS_BOX_PRINCIPAL,
                            DriverFields* fields = nullptr, DriverRefine* refine = nullptr) {
  // Task_File_SVGS.txt values
  float voxel_size = 0.05f, seed_size = 0.25f, graph_size = 0.5f, sig_p = 0.2f, sig_n = 0.2f, sig_o = 0.2f, sig_e = 0.2f, sig_c = 0.2f,
        sig_w = 1.0f, sig_a = 0.0f, sig_b = 0.25f, cut_thred = 0.5f;
  int points_min = 0, voxels_min = 3, adjacency_min = 3;
  if (input_vector.size() > 60) {  // every second line from 28 on (test:108-125)
    auto num = [&](size_t line) { return std::atof(input_vector[line].c_str()); };
    float* const f[] = {&voxel_size, &seed_size, &graph_size, &sig_p, &sig_n, &sig_o, &sig_e, &sig_c, &sig_w, &sig_a, &sig_b};
    for (size_t k = 0; k < 11; ++k) *f[k] = (float)num(28 + 2 * k);
    sig_c = (float)num(50);  // the reference reuses sig_c for the normal importance (test:120): the convexity sigma of line 42 is lost
    cut_thred = (float)num(52);
    points_min = (int)num(54); voxels_min = (int)num(58); adjacency_min = (int)num(60);
  } else {
    sig_c = 0.75f;  // normal importance of Task_File_SVGS.txt, carried in sig_c as above
  }
  double min_x = 0, min_y = 0, min_z = 0, max_x = 0, max_y = 0, max_z = 0;

  pcl::SuperVoxelBasedSegmentation<pcl::PointXYZ> supervoxel_structure(voxel_size);  // test:138
  supervoxel_structure.setInputCloud(input_cloud);
  supervoxel_structure.getCloudPointNum(input_cloud);
  supervoxel_structure.addPointsFromInputCloud();
  supervoxel_structure.setVoxelSize(voxel_size, points_min);                          // test:144-146
  supervoxel_structure.setSupervoxelSize(seed_size, voxels_min, points_min, adjacency_min);
  supervoxel_structure.setGraphSize(seed_size * 2, graph_size);
  supervoxel_structure.getBoundingBox(min_x, min_y, min_z, max_x, max_y, max_z);      // test:148-149
  supervoxel_structure.setBoundingBox(min_x, min_y, min_z, max_x, max_y, max_z);
  supervoxel_structure.setSupervoxelCentersCentroids();                               // test:152-153
  supervoxel_structure.getVoxelNum();
  supervoxel_structure.segmentSupervoxelCloudWithGraphModel(sig_a, sig_b, sig_c, cut_thred, sig_p, sig_n, sig_o, sig_e, sig_c, sig_w);  // test:156
  PCXYZRGBPtr clustered_cloud(new PCXYZRGB);
  supervoxel_structure.drawColorMapofPointsinClusters(clustered_cloud);               // test:159-160
  clusters_points_idx = supervoxel_structure.getClusterIdx();
  if (descriptors) *descriptors = supervoxel_structure.getClusterDescriptors();
  if (graph) { graph->edges = supervoxel_structure.getClusterGraph(); supervoxel_structure.getClusterAdjacency(graph->adjacency); }
  if (boxes) *boxes = supervoxel_structure.getClusterBoxes(box_frame);
  if (fields) driverFields(supervoxel_structure, *fields);
  if (refine && refine->on) driverRefine(supervoxel_structure, *refine, clusters_points_idx);
  if (sum) {
    sum->points = (long)input_cloud->points.size(); sum->voxels = supervoxel_structure.getVoxelNum();
    sum->supervoxels = supervoxel_structure.getSuperVoxelNum(); sum->clusters = supervoxel_structure.getClusterNum();
    sum->kept = (long)clusters_points_idx.size();
    sum->labelled = 0;
    for (auto& c : clusters_points_idx) sum->labelled += (long)c.size();
  }
  return 0;
}

#endif  // VGS_EXAMPLE_DRIVERS_HPP_
