// examples/vgs_run.cpp -- the task-file front end the reference implies: read a task file
// (Task_File_VGS.txt / Task_File_SVGS.txt layout), dispatch on its "Method" entry (line 24: 2 = VGS, 3 = SVGS), load
// the input PCD, segment, write the coloured clusters as PCD -- what `main` around the reference's `test` drivers does
// with input_vector[12]/[15] (input path / name) and [18]/[21] (output path / name), minus the viewer.
//   usage: vgs_run <task file> [--in <file.pcd|.ply>] [--out <file.pcd>] [--seed <n>] [--ascii] [--debug-meshes <prefix>]
//                  [--segments <file.csv>] [--segment-graph <file.csv>] [--segment-adjacency <file.txt>]
//                  [--segment-boxes <file.csv> [--box-frame principal|upright]]
// --debug-meshes (VGS only) also writes the reference's voxel drawings as <prefix>_voxels.ply, _clustered_voxels.ply, _normals.ply.
// --in / --out replace the path + name entries of the task file (the shipped ones hold Windows paths).
// --segments writes one CSV row per kept cluster (getClusterDescriptors, row i = cluster i of the output): label, n_points, n_nodes,
// bbox (6), centroid (3), eigenvalues (3, ascending), normal (3), major axis (3), the eight eigen features -- doubles as %.17g, floats as
// %.9g, so every value reads back exactly.
// --segment-graph writes one CSV row per edge of the cluster adjacency graph (getClusterGraph, ascending (a, b), cluster indices of the
// output): a, b, n_pairs, n_finite, nodes_a, nodes_b, w_mean (w_sum / n_finite, NaN without a finite weight), w_min, w_max -- doubles as
// %.17g, floats as %.9g.  --segment-adjacency writes getClusterAdjacency (PCL's getSupervoxelAdjacency idiom: both directions of every
// edge), one "a,b" line per multimap entry in its iteration order.
// --segment-boxes writes one CSV row per kept cluster (getClusterBoxes, row i = cluster i of the output): label, center (3), half (3),
// frame (9), lo (3), hi (3), every value as %.17g; --box-frame selects the frame, principal (the default) or upright.
// Prints "<method> <points> <voxels> <supervoxels> <all clusters> <kept clusters> <labelled points>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "drivers.hpp"
#include "point_clouds_io.hpp"
#include "segments_csv.hpp"

static int writeAdjacency(const std::string& path, const std::multimap<uint32_t, uint32_t>& adj) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return -1;
  for (const auto& kv : adj) std::fprintf(f, "%u,%u\n", kv.first, kv.second);
  return std::fclose(f) == 0 ? 0 : -1;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <task file> [--in file.pcd] [--out file.pcd] [--seed n] [--ascii] [--debug-meshes prefix] [--segments file.csv] "
                 "[--segment-graph file.csv] [--segment-adjacency file.txt] [--segment-boxes file.csv [--box-frame principal|upright]]\n",
                 argv[0]);
    return 2;
  }
  std::string in_file, out_file, debug_prefix, segments_file, graph_file, adjacency_file, boxes_file;
  int box_frame = VGS_BOX_PRINCIPAL;
  uint64_t seed = 0;
  bool ascii = false;
  for (int a = 2; a < argc; ++a) {
    if (!std::strcmp(argv[a], "--in") && a + 1 < argc) in_file = argv[++a];
    else if (!std::strcmp(argv[a], "--out") && a + 1 < argc) out_file = argv[++a];
    else if (!std::strcmp(argv[a], "--seed") && a + 1 < argc) seed = std::strtoull(argv[++a], nullptr, 10);
    else if (!std::strcmp(argv[a], "--ascii")) ascii = true;
    else if (!std::strcmp(argv[a], "--debug-meshes") && a + 1 < argc) debug_prefix = argv[++a];
    else if (!std::strcmp(argv[a], "--segments") && a + 1 < argc) segments_file = argv[++a];
    else if (!std::strcmp(argv[a], "--segment-graph") && a + 1 < argc) graph_file = argv[++a];
    else if (!std::strcmp(argv[a], "--segment-adjacency") && a + 1 < argc) adjacency_file = argv[++a];
    else if (!std::strcmp(argv[a], "--segment-boxes") && a + 1 < argc) boxes_file = argv[++a];
    else if (!std::strcmp(argv[a], "--box-frame") && a + 1 < argc) {
      ++a;
      if (!std::strcmp(argv[a], "principal")) box_frame = VGS_BOX_PRINCIPAL;
      else if (!std::strcmp(argv[a], "upright")) box_frame = VGS_BOX_UPRIGHT;
      else { std::fprintf(stderr, "--box-frame %s: principal or upright\n", argv[a]); return 2; }
    }
    else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
  }
  const std::vector<std::string> task = inputTaskTxtFile(argv[1]);
  if (task.size() < 51) { std::fprintf(stderr, "%s: not a task file (%zu lines)\n", argv[1], task.size()); return 2; }
  const int method = std::atoi(task[24].c_str());
  if (method != 2 && method != 3) { std::fprintf(stderr, "%s: method %d is neither 2 (VGS) nor 3 (SVGS)\n", argv[1], method); return 2; }
  if (method == 3 && task.size() < 61) { std::fprintf(stderr, "%s: SVGS task files have 61 lines\n", argv[1]); return 2; }
  if (in_file.empty()) in_file = task[12] + task[15];
  if (out_file.empty()) {
    std::string name = task[21];
    if (name.size() >= 4) name.replace(name.size() - 4, 4, ".pcd");  // test:78 / test:163
    out_file = task[18] + name;
  }
  PCXYZPtr cloud(new PCXYZ);
  const bool ply = in_file.size() > 4 && in_file.substr(in_file.size() - 4) == ".ply";
  if ((ply ? inputPointCloudData2(in_file, cloud) : inputPointCloudData(in_file, cloud)) != 0) return 1;
  std::vector<std::vector<int>> clusters;
  DriverSummary sum;
  std::vector<pcl::ClusterDescriptor> desc;
  std::vector<pcl::ClusterDescriptor>* want = segments_file.empty() ? nullptr : &desc;
  DriverGraph graph;
  DriverGraph* want_graph = (graph_file.empty() && adjacency_file.empty()) ? nullptr : &graph;
  std::vector<pcl::ClusterBox> boxes;
  std::vector<pcl::ClusterBox>* want_boxes = boxes_file.empty() ? nullptr : &boxes;
  try {
    if (method == 2) {
      if (segmentationVGS(cloud, task, clusters, &sum, debug_prefix, 0.0, want, want_graph, want_boxes, box_frame) != 0) { std::fprintf(stderr, "cannot write the debug meshes\n"); return 1; }
    } else {
      segmentationSVGS(cloud, task, clusters, &sum, want, want_graph, want_boxes, box_frame);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  if (saveColoredClusters(out_file, cloud, clusters, seed, !ascii) != 0) return 1;
  if (want && writeSegmentsCsv(segments_file, desc) != 0) { std::fprintf(stderr, "cannot write %s\n", segments_file.c_str()); return 1; }
  if (!graph_file.empty() && writeGraphCsv(graph_file, graph.edges) != 0) { std::fprintf(stderr, "cannot write %s\n", graph_file.c_str()); return 1; }
  if (want_boxes && writeBoxesCsv(boxes_file, boxes) != 0) { std::fprintf(stderr, "cannot write %s\n", boxes_file.c_str()); return 1; }
  if (!adjacency_file.empty() && writeAdjacency(adjacency_file, graph.adjacency) != 0) {
    std::fprintf(stderr, "cannot write %s\n", adjacency_file.c_str());
    return 1;
  }
  std::printf("%d %ld %ld %ld %ld %ld %ld\n", method, sum.points, sum.voxels, sum.supervoxels, sum.clusters, sum.kept, sum.labelled);
  return 0;
}
