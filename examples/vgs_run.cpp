// examples/vgs_run.cpp -- the task-file front end the reference implies: read a task file
// (Task_File_VGS.txt / Task_File_SVGS.txt layout), dispatch on its "Method" entry (line 24: 2 = VGS, 3 = SVGS), load
// the input PCD, segment, write the coloured clusters as PCD -- what `main` around the reference's `test` drivers does
// with input_vector[12]/[15] (input path / name) and [18]/[21] (output path / name), minus the viewer.
//   usage: vgs_run <task file> [--in <file.pcd|.ply>] [--out <file.pcd>] [--seed <n>] [--ascii] [--debug-meshes <prefix>]
//                  [--segments <file.csv>] [--segment-graph <file.csv>] [--segment-adjacency <file.txt>]
//                  [--segment-boxes <file.csv> [--box-frame principal|upright]]
//                  [--segment-fields <file.csv> --fields a[,b,...]] [--segment-classes <file.csv> --class-field <name> --classes <C>]
//                  [--segment-matches <file.csv> --truth-field <name> [--truth-matches <file.csv>]]
//                  [--refine [--patch-radius <r>] [--switch-ratio <s>] [--no-fill]]
//                  [--refined-segments <file.csv>] [--refined-segment-boxes <file.csv>]
//                  [--refined-segment-fields <file.csv> --fields a[,b,...]] [--refined-segment-classes <file.csv> --class-field <name> --classes <C>]
//                  [--refined-matches <file.csv> --truth-field <name> [--refined-truth-matches <file.csv>]]
//                  [--refined-components <file.csv>] [--class-components <file.csv> --class-field <name> --classes <C>]
//                  [--component-ids <file.i32>]
//                  [--refined-graph <file.csv>] [--class-graph <file.csv> --class-field <name> --classes <C>]
//                  [--absorbed-labels <file.i32> [--absorb-islands <points>] [--absorb-min-points <points>] [--absorb-rounds <r>] [--absorb-drop]]
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
// --segment-fields writes one CSV row per kept cluster (getClusterFieldStats over the fields --fields names, read from the input PCD: any
// numeric type, COUNT 1): label, then per field n_valid, mean, var (%.17g), min, max (%.9g).  --segment-classes writes one row per kept
// cluster (getClusterClassHistogram over the field --class-field names, classes 0 .. C-1 with C = --classes in 1 .. 1024): label, majority,
// majority_count, n_outside, hist_0 .. hist_{C-1}.  A flag without its companions, or either with a PLY input, is a usage error (status 2).
// --segment-matches scores the clusters against the reference labelling in the field --truth-field names (compareClusterLabels; read from
// the input PCD as exact integers, any numeric type, COUNT 1; a negative value = no annotation; a value that is not an integer or does not
// fit int32 ends the run with an error, nothing is rounded) and writes one CSV row per kept cluster: label, n_annotated, n_refs, best_ref,
// best_n, best_iou (%.17g).  --truth-matches adds one row per reference id: ref_id, n_points, n_dropped, best_seg, best_n, best_iou.  A
// second and third line on stdout carry the summary ("matches" and its twelve numbers) and the scores at IoU > 0.5 ("scores matched
// precision recall f1 purity completeness ari", %.17g).  The same usage rules.
// --refine writes the coloured PCD from the point-level refined labels (refineClusterLabels: boundary points take the label of the nearest
// planar patch, the points of unused voxels and dropped clusters are filled unless --no-fill): clusters in label order, points in
// ascending index; every CSV keeps describing the voxel labels.  --patch-radius (default: the voxel size, the supervoxel size for SVGS),
// --switch-ratio in [0, 1] (default 0.25) and --no-fill need --refine.
// --refined-segments, --refined-segment-boxes (which honours --box-frame) and --refined-matches (which reads the --truth-field that
// --segment-matches reads; --refined-truth-matches beside it) write the same CSVs -- same writers, same columns, same exact round trip --
// over the REFINED labels (getLabelDescriptors, getLabelBoxes, compareClusterLabels with the labels): the tables of the result the PCD
// holds.  The flags above keep writing the voxel-label tables, and a run may write both.  --refined-matches adds the stdout lines
// "refined-matches" and "refined-scores".  Each needs --refine (a usage error, status 2, without it).
// --refined-segment-fields and --refined-segment-classes write the files of --segment-fields / --segment-classes -- same writers, same
// columns -- over the REFINED labels (getLabelFieldStats, getLabelClassHistogram), from the same --fields / --class-field / --classes,
// which may be given for a refined file alone.  Both need --refine and a PCD input.
// --refined-components writes one CSV row per connected part of the REFINED labels (getLabelComponents: two (label, node) pairs are joined
// when either node's adjacency row holds the other): part, label, n_points, n_nodes, first_node, largest (1 for the part with the most
// points of its label) -- the stranded islands a refinement left per cluster.  It needs --refine.  --class-components writes the same
// table for the integer class field --class-field names (read from the input PCD as exact integers, like --truth-field; a negative value =
// no class; classes 0 .. C-1 with C = --classes, a class >= C ends the run with an error): the instances of every class over the scene's
// own neighbourhood graph.  It needs --class-field, --classes and a PCD input.  --component-ids writes the part of every point (int32,
// input order, -1 = none) of whichever of the two tables was asked for, raw; with both, or with neither, it is a usage error.
// --refined-graph writes one CSV row per edge of the adjacency graph of the REFINED labels (getLabelGraph, ascending (a, b)): a, b,
// n_shared (nodes that hold points of both), then the columns of --segment-graph over the contacts of a and b -- n_pairs, n_finite,
// nodes_a, nodes_b, w_mean, w_min, w_max, doubles as %.17g, floats as %.9g.  It needs --refine.  --class-graph writes the same table for
// the class field of --class-components (same reading, same rules): which classes touch, and across how much boundary.
// --absorbed-labels writes one label per point (int32, input order, -1 = none, raw like --component-ids): the source labelling with its
// stranded and small connected parts absorbed into the neighbour they touch most (absorbLabelParts).  The source is --refine (the refined
// labels, K = the kept clusters) or --class-field <name> --classes <C> (the class field, read like --class-components); with both it is a
// usage error.  At least one threshold is needed: --absorb-islands <points> (parts below it that are not the largest of their label)
// and/or --absorb-min-points <points> (any part below it); --absorb-rounds <r> (0 .. 64, default 8) caps the rounds, --absorb-drop gives
// what is still too small afterwards -1.  A further stdout line carries the eight counts: "absorbed rounds parts points candidates
// candidate_points dropped parts_left skipped".  With --refine every --refined-* table keeps describing the refined labels.
// Prints "<method> <points> <voxels> <supervoxels> <all clusters> <kept clusters> <labelled points>".
#include <algorithm>
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
                 "[--segment-graph file.csv] [--segment-adjacency file.txt] [--segment-boxes file.csv [--box-frame principal|upright]] "
                 "[--segment-fields file.csv --fields a[,b,...]] [--segment-classes file.csv --class-field name --classes C] "
                 "[--segment-matches file.csv --truth-field name [--truth-matches file.csv]] "
                 "[--refine [--patch-radius r] [--switch-ratio s] [--no-fill]] [--refined-segments file.csv] [--refined-segment-boxes file.csv] "
                 "[--refined-segment-fields file.csv --fields a[,b,...]] [--refined-segment-classes file.csv --class-field name --classes C] "
                 "[--refined-matches file.csv --truth-field name [--refined-truth-matches file.csv]] "
                 "[--refined-components file.csv] [--class-components file.csv --class-field name --classes C] [--component-ids file.i32] "
                 "[--refined-graph file.csv] [--class-graph file.csv --class-field name --classes C] "
                 "[--absorbed-labels file.i32 [--absorb-islands points] [--absorb-min-points points] [--absorb-rounds r] [--absorb-drop]]\n",
                 argv[0]);
    return 2;
  }
  std::string in_file, out_file, debug_prefix, segments_file, graph_file, adjacency_file, boxes_file, fields_file, classes_file, class_field, matches_file, truth_field, truth_file;
  std::string r_segments_file, r_boxes_file, r_matches_file, r_truth_file, r_fields_file, r_classes_file;
  std::string r_parts_file, c_parts_file, part_ids_file, r_graph_file, c_graph_file, absorbed_file;
  DriverAbsorb absorb;
  bool absorb_opts = false, absorb_threshold = false;
  std::vector<std::string> field_names;
  bool have_fields = false, have_classes = false;
  long n_classes = 0;
  int box_frame = VGS_BOX_PRINCIPAL;
  uint64_t seed = 0;
  bool ascii = false;
  DriverRefine refine;
  bool refine_opts = false;
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
    else if (!std::strcmp(argv[a], "--segment-fields") && a + 1 < argc) fields_file = argv[++a];
    else if (!std::strcmp(argv[a], "--fields") && a + 1 < argc) {
      have_fields = true;
      const std::string list = argv[++a];
      for (size_t b = 0; b <= list.size();) {
        const size_t e = std::min(list.find(',', b), list.size());
        if (e > b) field_names.push_back(list.substr(b, e - b));
        b = e + 1;
      }
    }
    else if (!std::strcmp(argv[a], "--segment-classes") && a + 1 < argc) classes_file = argv[++a];
    else if (!std::strcmp(argv[a], "--class-field") && a + 1 < argc) class_field = argv[++a];
    else if (!std::strcmp(argv[a], "--classes") && a + 1 < argc) {
      have_classes = true;
      char* end = nullptr;
      n_classes = std::strtol(argv[++a], &end, 10);
      if (end == argv[a] || *end != 0 || n_classes < 1 || n_classes > 1024) { std::fprintf(stderr, "--classes %s: a number in 1 .. 1024\n", argv[a]); return 2; }
    }
    else if (!std::strcmp(argv[a], "--segment-matches") && a + 1 < argc) matches_file = argv[++a];
    else if (!std::strcmp(argv[a], "--truth-field") && a + 1 < argc) truth_field = argv[++a];
    else if (!std::strcmp(argv[a], "--truth-matches") && a + 1 < argc) truth_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segments") && a + 1 < argc) r_segments_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segment-boxes") && a + 1 < argc) r_boxes_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segment-fields") && a + 1 < argc) r_fields_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-segment-classes") && a + 1 < argc) r_classes_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-matches") && a + 1 < argc) r_matches_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-truth-matches") && a + 1 < argc) r_truth_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-components") && a + 1 < argc) r_parts_file = argv[++a];
    else if (!std::strcmp(argv[a], "--class-components") && a + 1 < argc) c_parts_file = argv[++a];
    else if (!std::strcmp(argv[a], "--component-ids") && a + 1 < argc) part_ids_file = argv[++a];
    else if (!std::strcmp(argv[a], "--refined-graph") && a + 1 < argc) r_graph_file = argv[++a];
    else if (!std::strcmp(argv[a], "--class-graph") && a + 1 < argc) c_graph_file = argv[++a];
    else if (!std::strcmp(argv[a], "--absorbed-labels") && a + 1 < argc) absorbed_file = argv[++a];
    else if (!std::strcmp(argv[a], "--absorb-drop")) { absorb.drop = true; absorb_opts = true; }
    else if ((!std::strcmp(argv[a], "--absorb-islands") || !std::strcmp(argv[a], "--absorb-min-points") || !std::strcmp(argv[a], "--absorb-rounds")) &&
             a + 1 < argc) {
      const char which = argv[a][9];   // i, m or r
      char* end = nullptr;
      const long long v = std::strtoll(argv[++a], &end, 10);
      if (end == argv[a] || *end != 0 || v < 0 || (which == 'r' && v > 64)) {
        std::fprintf(stderr, "%s %s: %s\n", argv[a - 1], argv[a], which == 'r' ? "a number in 0 .. 64" : "a number of points, not negative");
        return 2;
      }
      if (which == 'i') absorb.island_points = v; else if (which == 'm') absorb.min_points = v; else absorb.max_rounds = (int32_t)v;
      absorb_opts = true;
      if (which != 'r') absorb_threshold = true;
    }
    else if (!std::strcmp(argv[a], "--refine")) refine.on = true;
    else if (!std::strcmp(argv[a], "--no-fill")) { refine.fill = false; refine_opts = true; }
    else if ((!std::strcmp(argv[a], "--patch-radius") || !std::strcmp(argv[a], "--switch-ratio")) && a + 1 < argc) {
      const bool radius = argv[a][2] == 'p';
      char* end = nullptr;
      const float v = std::strtof(argv[++a], &end);
      if (end == argv[a] || *end != 0 || !std::isfinite(v) || v < 0.0f || (!radius && v > 1.0f)) {
        std::fprintf(stderr, "%s %s: %s\n", argv[a - 1], argv[a], radius ? "a finite number, not negative" : "a number in [0, 1]");
        return 2;
      }
      (radius ? refine.patch_radius : refine.switch_ratio) = v;
      refine_opts = true;
    }
    else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
  }
  if (refine_opts && !refine.on) { std::fprintf(stderr, "--patch-radius / --switch-ratio / --no-fill need --refine\n"); return 2; }
  if (!fields_file.empty() && (!have_fields || field_names.empty())) { std::fprintf(stderr, "--segment-fields needs --fields a[,b,...]\n"); return 2; }
  if (!r_fields_file.empty() && (!have_fields || field_names.empty())) { std::fprintf(stderr, "--refined-segment-fields needs --fields a[,b,...]\n"); return 2; }
  if (!r_classes_file.empty() && class_field.empty()) { std::fprintf(stderr, "--refined-segment-classes needs --class-field <name>\n"); return 2; }
  if (!r_classes_file.empty() && !have_classes) { std::fprintf(stderr, "--refined-segment-classes needs --classes <C>\n"); return 2; }
  if (!(fields_file.empty() && r_fields_file.empty()) && field_names.size() > 64) { std::fprintf(stderr, "--fields: at most 64 fields\n"); return 2; }
  if (!c_parts_file.empty() && class_field.empty()) { std::fprintf(stderr, "--class-components needs --class-field <name>\n"); return 2; }
  if (!c_parts_file.empty() && !have_classes) { std::fprintf(stderr, "--class-components needs --classes <C>\n"); return 2; }
  if (!r_parts_file.empty() && !refine.on) { std::fprintf(stderr, "--refined-components needs --refine\n"); return 2; }
  if (!c_graph_file.empty() && class_field.empty()) { std::fprintf(stderr, "--class-graph needs --class-field <name>\n"); return 2; }
  if (!c_graph_file.empty() && !have_classes) { std::fprintf(stderr, "--class-graph needs --classes <C>\n"); return 2; }
  if (!r_graph_file.empty() && !refine.on) { std::fprintf(stderr, "--refined-graph needs --refine\n"); return 2; }
  if (absorb_opts && absorbed_file.empty()) {
    std::fprintf(stderr, "--absorb-islands / --absorb-min-points / --absorb-rounds / --absorb-drop need --absorbed-labels <file.i32>\n");
    return 2;
  }
  const bool absorb_class = !absorbed_file.empty() && !refine.on;   // the class field is the source
  if (!absorbed_file.empty()) {
    const bool cls = have_classes || !class_field.empty();
    if (refine.on == cls) {
      std::fprintf(stderr, "--absorbed-labels absorbs the labels of exactly one of --refine and --class-field <name> --classes <C> (%s given)\n",
                   cls ? "both" : "neither");
      return 2;
    }
    if (absorb_class && class_field.empty()) { std::fprintf(stderr, "--absorbed-labels needs --class-field <name>\n"); return 2; }
    if (absorb_class && !have_classes) { std::fprintf(stderr, "--absorbed-labels needs --classes <C>\n"); return 2; }
    if (!absorb_threshold) { std::fprintf(stderr, "--absorbed-labels needs --absorb-islands <points> and/or --absorb-min-points <points>\n"); return 2; }
  }
  absorb.on = !absorbed_file.empty();
  if (!part_ids_file.empty() && r_parts_file.empty() == c_parts_file.empty()) {
    std::fprintf(stderr, "--component-ids writes the parts of exactly one of --refined-components and --class-components (%s given)\n",
                 r_parts_file.empty() ? "neither" : "both");
    return 2;
  }
  if (!classes_file.empty() && class_field.empty()) { std::fprintf(stderr, "--segment-classes needs --class-field <name>\n"); return 2; }
  if (!classes_file.empty() && !have_classes) { std::fprintf(stderr, "--segment-classes needs --classes <C>\n"); return 2; }
  if (fields_file.empty() && r_fields_file.empty() && have_fields) {
    std::fprintf(stderr, "--fields needs --segment-fields <file.csv> (or --refined-segment-fields)\n");
    return 2;
  }
  if (classes_file.empty() && r_classes_file.empty() && c_parts_file.empty() && c_graph_file.empty() && !absorb_class && (have_classes || !class_field.empty())) {
    std::fprintf(stderr, "--class-field / --classes need --segment-classes <file.csv> (or --refined-segment-classes, --class-components, --class-graph, --absorbed-labels)\n");
    return 2;
  }
  if (!matches_file.empty() && truth_field.empty()) { std::fprintf(stderr, "--segment-matches needs --truth-field <name>\n"); return 2; }
  if (!refine.on && !(r_segments_file.empty() && r_boxes_file.empty() && r_matches_file.empty() && r_truth_file.empty() && r_fields_file.empty() &&
                      r_classes_file.empty())) {
    std::fprintf(stderr, "--refined-segments / --refined-segment-boxes / --refined-segment-fields / --refined-segment-classes / --refined-matches / "
                 "--refined-truth-matches need --refine\n");
    return 2;
  }
  if (!r_matches_file.empty() && truth_field.empty()) { std::fprintf(stderr, "--refined-matches needs --truth-field <name>\n"); return 2; }
  if (r_matches_file.empty() && !r_truth_file.empty()) { std::fprintf(stderr, "--refined-truth-matches needs --refined-matches <file.csv>\n"); return 2; }
  if (matches_file.empty() && ((!truth_field.empty() && r_matches_file.empty()) || !truth_file.empty())) {
    std::fprintf(stderr, "--truth-field / --truth-matches need --segment-matches <file.csv> (--truth-field serves --refined-matches too)\n");
    return 2;
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
  const bool want_truth = !(matches_file.empty() && r_matches_file.empty());
  const bool any_fields = !(fields_file.empty() && r_fields_file.empty()), any_classes = !(classes_file.empty() && r_classes_file.empty());
  const bool class_labels = !(c_parts_file.empty() && c_graph_file.empty()) || absorb_class;   // the class field read as a labelling of its own
  if (ply && (any_fields || any_classes || want_truth || class_labels)) {   // (a usage error: nothing has been loaded yet)
    std::fprintf(stderr, "--segment-fields / --segment-classes / --refined-segment-fields / --refined-segment-classes / --segment-matches / "
                 "--refined-matches / --class-components / --class-graph / --absorbed-labels read their fields from a PCD input, not from %s\n", in_file.c_str());
    return 2;
  }
  if ((ply ? inputPointCloudData2(in_file, cloud) : inputPointCloudData(in_file, cloud)) != 0) return 1;
  DriverFields fields;
  DriverFields* want_fields = (!any_fields && !any_classes && !want_truth && !class_labels) ? nullptr : &fields;
  if (want_fields) {   // the attributes ride in the input PCD, one row per point of the cloud
    std::string err;
    if (any_fields) {
      if (vgs_io::read_pcd_fields(in_file, field_names, fields.field, err) != 0) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
      fields.channels = (int)field_names.size();
      fields.want_stats = !fields_file.empty();
    }
    if (any_classes) {
      std::vector<float> v;
      if (vgs_io::read_pcd_fields(in_file, {class_field}, v, err) != 0) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
      fields.classes.resize(v.size());
      for (size_t i = 0; i < v.size(); ++i) fields.classes[i] = (v[i] >= -2147483648.0f && v[i] < 2147483648.0f) ? (int32_t)v[i] : -1;
      fields.n_classes = (int)n_classes;
      fields.want_hist = !classes_file.empty();
    }
    if (class_labels) {
      if (vgs_io::read_pcd_field_int32(in_file, class_field, fields.part_classes, err) != 0) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
      fields.parts_K = (int64_t)n_classes;
      fields.want_parts = !c_parts_file.empty();
      fields.want_parts_graph = !c_graph_file.empty();
      if (absorb_class) fields.absorb = absorb;
    }
    if (want_truth) {
      if (vgs_io::read_pcd_field_int32(in_file, truth_field, fields.truth, err) != 0) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
      fields.have_truth = !matches_file.empty();   // (the voxel labels are scored only when their table is asked for)
      if (!r_matches_file.empty()) refine.truth = &fields.truth;
    }
  }
  refine.want_descriptors = !r_segments_file.empty();
  refine.want_boxes = !r_boxes_file.empty();
  refine.want_stats = !r_fields_file.empty();
  refine.want_hist = !r_classes_file.empty();
  refine.want_components = !r_parts_file.empty();
  refine.want_graph = !r_graph_file.empty();
  if (absorb.on && !absorb_class) refine.absorb = absorb;
  refine.fields = &fields;
  refine.box_frame = box_frame;
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
      if (segmentationVGS(cloud, task, clusters, &sum, debug_prefix, 0.0, want, want_graph, want_boxes, box_frame, want_fields, &refine) != 0) { std::fprintf(stderr, "cannot write the debug meshes\n"); return 1; }
    } else {
      segmentationSVGS(cloud, task, clusters, &sum, want, want_graph, want_boxes, box_frame, want_fields, &refine);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  if (refine.on) {   // the summary's last number counts what the output holds
    sum.labelled = 0;
    for (const auto& c : clusters) sum.labelled += (long)c.size();
  }
  if (saveColoredClusters(out_file, cloud, clusters, seed, !ascii) != 0) return 1;
  if (want && writeSegmentsCsv(segments_file, desc) != 0) { std::fprintf(stderr, "cannot write %s\n", segments_file.c_str()); return 1; }
  if (!graph_file.empty() && writeGraphCsv(graph_file, graph.edges) != 0) { std::fprintf(stderr, "cannot write %s\n", graph_file.c_str()); return 1; }
  if (want_boxes && writeBoxesCsv(boxes_file, boxes) != 0) { std::fprintf(stderr, "cannot write %s\n", boxes_file.c_str()); return 1; }
  if (!fields_file.empty() && writeFieldStatsCsv(fields_file, field_names, fields.stats) != 0) { std::fprintf(stderr, "cannot write %s\n", fields_file.c_str()); return 1; }
  if (!classes_file.empty() && writeClassHistCsv(classes_file, fields.n_classes, fields.hist) != 0) { std::fprintf(stderr, "cannot write %s\n", classes_file.c_str()); return 1; }
  if (!matches_file.empty() && writeSegmentMatchesCsv(matches_file, fields.matches) != 0) { std::fprintf(stderr, "cannot write %s\n", matches_file.c_str()); return 1; }
  if (!truth_file.empty() && writeTruthMatchesCsv(truth_file, fields.matches) != 0) { std::fprintf(stderr, "cannot write %s\n", truth_file.c_str()); return 1; }
  if (!r_segments_file.empty() && writeSegmentsCsv(r_segments_file, refine.descriptors) != 0) { std::fprintf(stderr, "cannot write %s\n", r_segments_file.c_str()); return 1; }
  if (!r_boxes_file.empty() && writeBoxesCsv(r_boxes_file, refine.boxes) != 0) { std::fprintf(stderr, "cannot write %s\n", r_boxes_file.c_str()); return 1; }
  if (!r_fields_file.empty() && writeFieldStatsCsv(r_fields_file, field_names, refine.stats) != 0) { std::fprintf(stderr, "cannot write %s\n", r_fields_file.c_str()); return 1; }
  if (!r_classes_file.empty() && writeClassHistCsv(r_classes_file, fields.n_classes, refine.hist) != 0) { std::fprintf(stderr, "cannot write %s\n", r_classes_file.c_str()); return 1; }
  if (!r_matches_file.empty() && writeSegmentMatchesCsv(r_matches_file, refine.matches) != 0) { std::fprintf(stderr, "cannot write %s\n", r_matches_file.c_str()); return 1; }
  if (!r_truth_file.empty() && writeTruthMatchesCsv(r_truth_file, refine.matches) != 0) { std::fprintf(stderr, "cannot write %s\n", r_truth_file.c_str()); return 1; }
  if (!r_parts_file.empty() && writeComponentsCsv(r_parts_file, refine.components) != 0) { std::fprintf(stderr, "cannot write %s\n", r_parts_file.c_str()); return 1; }
  if (!c_parts_file.empty() && writeComponentsCsv(c_parts_file, fields.parts) != 0) { std::fprintf(stderr, "cannot write %s\n", c_parts_file.c_str()); return 1; }
  if (!r_graph_file.empty() && writeLabelGraphCsv(r_graph_file, refine.graph) != 0) { std::fprintf(stderr, "cannot write %s\n", r_graph_file.c_str()); return 1; }
  if (!c_graph_file.empty() && writeLabelGraphCsv(c_graph_file, fields.parts_graph) != 0) { std::fprintf(stderr, "cannot write %s\n", c_graph_file.c_str()); return 1; }
  if (!part_ids_file.empty()) {
    const std::vector<int32_t>& ids = r_parts_file.empty() ? fields.parts.part_of_point : refine.components.part_of_point;
    FILE* f = std::fopen(part_ids_file.c_str(), "wb");
    const bool ok = f && std::fwrite(ids.data(), sizeof(int32_t), ids.size(), f) == ids.size();
    if (!f || std::fclose(f) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", part_ids_file.c_str()); return 1; }
  }
  const pcl::AbsorbedLabels& absorbed = absorb_class ? fields.absorb.out : refine.absorb.out;
  if (absorb.on) {
    FILE* f = std::fopen(absorbed_file.c_str(), "wb");
    const bool ok = f && std::fwrite(absorbed.labels.data(), sizeof(int32_t), absorbed.labels.size(), f) == absorbed.labels.size();
    if (!f || std::fclose(f) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", absorbed_file.c_str()); return 1; }
  }
  if (!adjacency_file.empty() && writeAdjacency(adjacency_file, graph.adjacency) != 0) {
    std::fprintf(stderr, "cannot write %s\n", adjacency_file.c_str());
    return 1;
  }
  std::printf("%d %ld %ld %ld %ld %ld %ld\n", method, sum.points, sum.voxels, sum.supervoxels, sum.clusters, sum.kept, sum.labelled);
  if (absorb.on)
    std::printf("absorbed %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)absorbed.rounds, (long long)absorbed.parts_absorbed,
                (long long)absorbed.points_relabelled, (long long)absorbed.candidates_left, (long long)absorbed.candidate_points_left,
                (long long)absorbed.points_dropped, (long long)absorbed.n_parts, (long long)absorbed.n_skipped);
  if (!matches_file.empty()) {
    std::printf("matches");
    for (int i = 0; i < 12; ++i) std::printf(" %lld", (long long)fields.matches.summary[i]);
    const pcl::ClusterLabelScores sc = pcl::clusterLabelScores(fields.matches, 0.5);
    std::printf("\nscores %lld %.17g %.17g %.17g %.17g %.17g %.17g\n", (long long)sc.matched, sc.precision, sc.recall, sc.f1, sc.purity, sc.completeness, sc.ari);
  }
  if (!r_matches_file.empty()) {
    std::printf("refined-matches");
    for (int i = 0; i < 12; ++i) std::printf(" %lld", (long long)refine.matches.summary[i]);
    const pcl::ClusterLabelScores sc = pcl::clusterLabelScores(refine.matches, 0.5);
    std::printf("\nrefined-scores %lld %.17g %.17g %.17g %.17g %.17g %.17g\n", (long long)sc.matched, sc.precision, sc.recall, sc.f1, sc.purity, sc.completeness, sc.ari);
  }
  return 0;
}
