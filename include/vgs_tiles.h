/* include/vgs_tiles.h -- C-ABI of the native tiled driver (libvgs_tiles.so): one process per GPU, spatial tiles, one
 * exchange of boundary records (BASELINE.json configs[4]).
 *
 * The reference is single-process (segmentationVGS, `test`:9-86); this is what a caller with a scene larger than one GPU
 * puts around the same stages.  The data path of include/vgs.h stays on each rank's GPU; the only data-path exchange is ONE
 * all-gather of boundary-voxel records per run (plus two small ones for the shared grid).  The collectives run over RCCL:
 * the caller hands in its ncclComm_t (as void*, so that this header needs no rccl.h).  The Python twin of this driver
 * (vgs-svgs-segmentation_amd/dist.py, torch.distributed) is kept as the test harness; both give the same labels.
 *
 * Protocol per run (csrc/tiles.cpp): shared octree grid (all-gather of the tiles' bounding boxes, the growth replayed on the
 * host, a GPU scan + broadcast only where a box leaves the step open) -> the four stages on tile + halo -> unique boundary
 * voxels (code, local root, owned voxels of that root) and the number of purely local segments leave the GPU -> ncclAllGather
 * -> the same union-find over (rank, root) on every rank, size filter on global sizes -> labels applied on the GPU.  Per-segment
 * descriptors on request afterwards: a second collective of their own (vgs_tiles_get_segment_descriptors).  The segment adjacency graph
 * on request: a third collective of its own (vgs_tiles_get_segment_graph).  Oriented boxes on request: the descriptor table (its collective,
 * unless it is cached) and one collective of their own per frame (vgs_tiles_get_segment_boxes).  Statistics of the caller's point
 * attributes on request: one collective per call, nothing cached (vgs_tiles_segment_field_stats, vgs_tiles_segment_class_histogram).
 * The score against the caller's reference labels on request: one collective per call, nothing cached (vgs_tiles_compare_labels).
 * Point-level label refinement on request: one collective per call (vgs_tiles_refine_point_labels).
 */
#ifndef VGS_TILES_H_
#define VGS_TILES_H_

#include "vgs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vgs_tiles vgs_tiles;

/* Communicator.  kind VGS_TILES_COMM_RCCL: `handle` is an ncclComm_t over `world` ranks (RCCL over xGMI inside a node), this
 * process is rank `rank` and uses HIP device p->device.  kind VGS_TILES_COMM_LOCAL: `handle` comes from
 * vgs_tiles_local_group_create -- `world` driver THREADS of one process meet in shared memory (what the tests use to run
 * several ranks on a single GPU, where RCCL refuses two ranks on one device). */
enum { VGS_TILES_COMM_RCCL = 0, VGS_TILES_COMM_LOCAL = 1, VGS_TILES_COMM_CALLBACKS = 2 };

/* kind VGS_TILES_COMM_CALLBACKS: `handle` points to this struct (copied by vgs_tiles_create) -- the caller's own transport over HOST
 * buffers (MPI, gloo, a test harness that runs two processes on one GPU).  Both return 0 on success.  all_gather: every rank sends
 * `bytes` bytes, recv holds world * bytes in rank order.  bcast: `bytes` bytes from rank `root` to everyone, in place. */
typedef struct vgs_tiles_callbacks {
  void* user;
  int (*all_gather)(void* user, const void* send, void* recv, uint64_t bytes);
  int (*bcast)(void* user, void* buf, uint64_t bytes, int root);
} vgs_tiles_callbacks;

/* Failures.  A rank that fails locally (a stage error, out of memory, an injected fault) still takes part in the next collective and
 * sends its status as a word of that payload, so that no peer is left waiting inside a collective: the failing rank returns its own
 * status and message, every other rank returns VGS_E_PEER naming it.  After either, the process should exit non-zero and let the
 * launcher end the job; a vgs_tiles handle is not usable after a failed run.  An error of the collective itself (RCCL, a callback)
 * is returned as VGS_E_HIP. */

vgs_status vgs_tiles_local_group_create(int world, void** group);
void vgs_tiles_local_group_destroy(void* group);
/* a rank thread that fails calls this so that the others leave their collectives with an error instead of waiting for it */
void vgs_tiles_local_group_abort(void* group);

/* layout: tiles_x x tiles_y tiles of side `pitch` centred on (center_x, center_y); rank k owns tile (k % tiles_x, k / tiles_x),
 * the outer tiles are open ended.  pitch <= 0: the largest x-extent over the ranks' clouds (agreed with one all-gather at the
 * first vgs_tiles_set_points). */
vgs_status vgs_tiles_create(const vgs_params* p, int comm_kind, void* comm_handle, int rank, int world, int tiles_x, int tiles_y,
                            double pitch, double center_x, double center_y, vgs_tiles** out);
void vgs_tiles_destroy(vgs_tiles* t);
const char* vgs_tiles_last_error_string(const vgs_tiles* t);

/* options.  VGS_TILES_OPT_STRICT_REGION (0 / 1, default 0): points a rank holds outside its own region may come back unlabelled
 * (their voxels are owned and cut by another rank).  0: vgs_tiles_set_points warns once on stderr; 1: it fails with VGS_E_ARG on that
 * rank and VGS_E_PEER on the others.  vgs_tiles_get_info reports the count either way. */
enum { VGS_TILES_OPT_STRICT_REGION = 1 };
vgs_status vgs_tiles_set_option(vgs_tiles* t, int32_t option, int64_t value);

/* this rank's points (host memory, stride_bytes 12 or 16).  The ranks exchange their border strips (2 * graph_size + voxel_size
 * wide, one all-gather: data loading, not part of a run) and every rank uploads its tile + halo. */
vgs_status vgs_tiles_set_points(vgs_tiles* t, const float* xyz_host, int64_t n, int32_t stride_bytes);
/* shared grid, the four stages, the boundary exchange, global labels */
vgs_status vgs_tiles_run(vgs_tiles* t);
/* host wall time of the last run's phases on this rank, milliseconds: shared grid (collectives included), the four stages,
 * boundary records off the GPU, the exchange (ONE all-gather), the boundary union-find, labels applied on the GPU, total */
enum { VGS_TILES_T_GRID = 0, VGS_TILES_T_STAGES = 1, VGS_TILES_T_RECORDS = 2, VGS_TILES_T_EXCHANGE = 3, VGS_TILES_T_MERGE = 4,
       VGS_TILES_T_LABELS = 5, VGS_TILES_T_TOTAL = 6, VGS_TILES_T_COUNT = 7 };
vgs_status vgs_tiles_get_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_T_COUNT */);
/* labels of this rank's own points (global segment ids, -1 = dropped), the number of segments kept over all ranks */
vgs_status vgs_tiles_get_point_labels(vgs_tiles* t, int32_t* labels /* n */, int64_t* kept_global);
/* points this rank holds outside its own region (they may come back unlabelled: load by region) */
vgs_status vgs_tiles_get_info(vgs_tiles* t, int64_t* n_outside, int64_t* n_local /* tile + halo */, int64_t* n_boundary_records);
/* the last run's boundary exchange as this rank saw it: payload bytes sent and received, and how many collectives carried them (1: every
 * rank's records fit the fixed-size all-gather of 8192 records; 3: a size word and one padded all-gather behind it) */
vgs_status vgs_tiles_get_exchange(vgs_tiles* t, int64_t* bytes_sent, int64_t* bytes_received, int32_t* collectives);
/* The boundary merge on its own (host arithmetic, no context, no GPU; for tests): rank r's records are entries rec_off[r] ..
 * rec_off[r+1] of code / root / cnt (vgs_get_boundary_roots), kept_local[r] its purely local segments.  Outputs: base[r] (labels of
 * rank r's local segments start there), per rank the unique local roots named by records (uroot, entries uoff[r] .. uoff[r+1]) and
 * their global labels (-1 = dropped by the `> voxels_min` filter on the GLOBAL size), the number of segments kept over all ranks.
 * uroot / ulabel hold at most rec_off[world] entries. */
vgs_status vgs_tiles_merge_boundary(int world, const int64_t* rec_off, const uint64_t* code, const int32_t* root, const int32_t* cnt,
                                    const int64_t* kept_local, int voxels_min, int64_t* base, int64_t* uoff, int32_t* uroot, int32_t* ulabel,
                                    int64_t* kept_total);
/* Per-segment descriptors over all ranks: the fields, layout and conventions of vgs_get_segment_descriptors (include/vgs.h), K =
 * kept_global rows (vgs_tiles_get_point_labels); row k describes exactly the points, over all ranks, that vgs_tiles_get_point_labels
 * labels k.  n_points, bbox6, centroid3 and cov6 are those points' count, exact float box, fp64 mean and population covariance; n_nodes
 * counts the voxels of the shared grid that hold label k, each once, by the rank that owns it (the voxel sizes the boundary merge's
 * `> voxels_min` filter sums).
 * A call with every array pointer NULL only writes *K (no collective).  Otherwise the call is COLLECTIVE: after one vgs_tiles_run every
 * rank makes it, and every rank receives the same bytes, bit-identical from call to call and from run to run on the same input and
 * layout.  Protocol (csrc/tiles.cpp): each rank's moments of its own points and owned voxels (vgs_get_own_segment_moments, one small
 * pipeline on its GPU) -> ONE all_gather_varlen of those records with a status word -> the same host fold on every rank
 * (vgs_tiles_fold_moments) -> the per-segment algebra on the rank's GPU (vgs_segment_descriptors_from_moments).  The table is cached:
 * a second call makes no collective; the next vgs_tiles_run or vgs_tiles_set_points drops it.  Failures as in vgs_tiles_run: a rank
 * whose local step fails still joins the exchange with its status word, returns its own error, and every other rank returns VGS_E_PEER
 * naming it (tests inject one with VGS_TILES_FAIL_AT=descriptors).  VGS_E_STATE (no collective) before a run.  vgs_tiles_run itself
 * gains no launch and no collective. */
vgs_status vgs_tiles_get_segment_descriptors(vgs_tiles* t, int64_t* K, int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3,
                                             double* cov6, double* evals3, double* evecs9, float* eigen8);
/* host wall time of the last descriptor collective on this rank, milliseconds: own moments on the GPU (with their download), the
 * exchange, the fold, the algebra on the GPU (with upload and download), total */
enum { VGS_TILES_D_MOMENTS = 0, VGS_TILES_D_EXCHANGE = 1, VGS_TILES_D_FOLD = 2, VGS_TILES_D_ALGEBRA = 3, VGS_TILES_D_TOTAL = 4, VGS_TILES_D_COUNT = 5 };
vgs_status vgs_tiles_get_descriptor_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_D_COUNT */);
/* The descriptor fold on its own (host arithmetic, no context, no GPU; for tests): rank r's records are entries rec_off[r] .. rec_off[r+1]
 * of label / n_points / n_nodes / bbox6 / anchor3 / s9 (vgs_get_own_segment_moments).  Outputs: K rows of folded moments, every pointer
 * required.  Per label, ranks in ascending order: the anchor a is the anchor of the lowest rank with n_points > 0; with delta = a_r - a in
 * fp64, S1 += S1_r + n_r delta and S2 += S2_r + S1_r delta^T + delta S1_r^T + n_r delta delta^T; n_points and n_nodes add, boxes take min
 * and max.  A row no record reaches: zero counts, sums and anchor, box +inf / -inf.  VGS_E_ARG for a label outside 0 .. K-1. */
vgs_status vgs_tiles_fold_moments(int world, const int64_t* rec_off, const int32_t* label, const int64_t* n_points, const int32_t* n_nodes,
                                  const float* bbox6, const float* anchor3, const double* s9, int64_t K, int64_t* n_points_out,
                                  int32_t* n_nodes_out, float* bbox6_out, float* anchor3_out, double* s9_out);
/* Segment adjacency graph over all ranks.
 * vgs_tiles_get_segment_graph returns the table of vgs_get_segment_graph (include/vgs.h) with the same fields, types, edge order and NaN
 * rules.  It is taken over the voxels of the shared grid and the global labels 0 .. kept_global-1 that vgs_tiles_get_point_labels reports.
 *   * A node is a used voxel of the shared grid with a kept global label.
 *   * An edge is a label pair a < b with a node pair {u, v}, v in u's stored adjacency row.
 *   * w(u, v) = vm_pair_weight(node[lower id], node[higher id]).  "Lower id" means the larger voxel code.  Every rank numbers its voxels
 *     in descending code order of the same grid, so the comparison v > u gives the same answer on every rank.
 * Counting rule.  It makes each contribution exist on exactly one rank:
 *   * A node pair {u, v} is counted by the rank that OWNS its lower-id endpoint u (vgs_set_owned_region), whoever owns v.
 *   * A node u of a "with a neighbour in b" (nodes_ab) is counted by the rank that owns u.
 * So a rank walks the rows of its owned used voxels only, and those rows include halo voxels.  The halo is 2 * graph_size + voxel_size
 * wide and the strips are assembled in rank order, so a halo voxel inside an owned voxel's row is complete and carries the same node
 * record as on its owner.  Its label comes from its owner: every owned voxel with a voxel of another rank in its row is a boundary voxel
 * of the run's exchange, so the records every rank already holds name (code, global label) of every such voxel; the driver hands them to
 * the context (vgs_set_halo_labels) and a used halo voxel in an owned row without one fails the call (VGS_E_UNSUPPORTED, the count in the
 * message) instead of shrinking the table.
 *
 * n_edges is required.  The call is COLLECTIVE whenever the table is not cached -- also with every array NULL, the size query, because the
 * size is not known before the ranks' tables meet: after one vgs_tiles_run every rank makes the first call.  Once it has returned VGS_OK
 * the table is cached on this rank: further calls (the size query, then the call with arrays of *n_edges rows; any pointer may be NULL)
 * make no collective and may be made by any rank alone, until the next vgs_tiles_run or vgs_tiles_set_points drops the table.
 * Protocol (csrc/tiles.cpp): the halo labels from the kept boundary records -> this rank's partial table (vgs_get_own_segment_graph, one
 * small pipeline on its GPU) -> ONE all_gather_varlen of 48-byte edge records behind a header of record count and status word -> the
 * same host fold on every rank (vgs_tiles_fold_edges).  Every rank receives the same bytes, bit-identical from call to call and from run
 * to run on the same input and layout.  Failures as in vgs_tiles_run: a rank whose local step fails still joins the exchange with its
 * status word, returns its own error, and every other rank returns VGS_E_PEER naming it (tests inject one with VGS_TILES_FAIL_AT=graph).
 * VGS_E_STATE (no collective) before a run.  vgs_tiles_run itself gains no launch and no collective; the point labels and the
 * descriptors are not touched. */
vgs_status vgs_tiles_get_segment_graph(vgs_tiles* t, int64_t* n_edges, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                       double* w_sum, float* w_min, float* w_max);
/* host wall time of the last graph collective on this rank, milliseconds: the halo labels (list and upload), the own table on the GPU (with
 * its download), the exchange, the fold, total */
enum { VGS_TILES_G_HALO = 0, VGS_TILES_G_OWN = 1, VGS_TILES_G_EXCHANGE = 2, VGS_TILES_G_FOLD = 3, VGS_TILES_G_TOTAL = 4, VGS_TILES_G_COUNT = 5 };
vgs_status vgs_tiles_get_graph_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_G_COUNT */);
/* the last graph collective's payload on this rank: (code, label) pairs handed to its context, edges of its own table, bytes it put into
 * the all-gather (header included, before padding to the largest rank's) */
vgs_status vgs_tiles_get_graph_payload(vgs_tiles* t, int64_t* halo_labels, int64_t* own_edges, int64_t* bytes_sent);
/* The edge fold on its own (host arithmetic, no context, no GPU; for tests): rank r's table is rows rec_off[r] .. rec_off[r+1] (rec_off[0]
 * = 0) of seg_ab / n_pairs / n_finite / nodes_ab / w_sum / w_min / w_max, ascending in (a, b), over the labels 0 .. K-1.  The tables are
 * merged by (a, b); per edge the ranks are taken in ascending order: n_pairs, n_finite and nodes_ab add, w_sum adds in fp64 in that
 * order starting from 0, w_min / w_max are the smallest / largest over the ranks with n_finite > 0 (the others' values are ignored) and NaN
 * when the total n_finite is 0.  *n_edges rows are written, at most rec_off[world]; any output array may be NULL.  VGS_E_ARG for a label
 * outside 0 .. K-1, for a >= b, and for a rank table that is not strictly ascending. */
vgs_status vgs_tiles_fold_edges(int world, const int64_t* rec_off, const int32_t* seg_ab, const int64_t* n_pairs, const int64_t* n_finite,
                                const int32_t* nodes_ab, const double* w_sum, const float* w_min, const float* w_max, int64_t K,
                                int64_t* n_edges, int32_t* seg_ab_out, int64_t* n_pairs_out, int64_t* n_finite_out, int32_t* nodes_ab_out,
                                double* w_sum_out, float* w_min_out, float* w_max_out);
/* Oriented bounding boxes over all ranks: the fields, layout and conventions of vgs_get_segment_boxes (include/vgs.h) -- frame, center3,
 * half3, frame9, lo3, hi3, every array K rows of doubles, any pointer may be NULL -- with K = kept_global rows; row k covers exactly the
 * points, over all ranks, that vgs_tiles_get_point_labels labels k (the points the tiled descriptors' n_points counts: each by the rank
 * that loaded it).  c is the centroid3 row and W the frame made from the evecs9 / cov6 rows of vgs_tiles_get_segment_descriptors, by the
 * same device code as on one engine; lo3 / hi3 are min / max of exact fp64 projections, which do not depend on the order, so the table is
 * the bit-exact function of the points, c and W that vgs_get_segment_boxes defines, and every rank receives the same bytes, bit-identical
 * from call to call and from run to run on the same input and layout (a zero bound may carry either sign).  A row that no point reaches
 * (a global label without a labelled point on any rank, n_points = 0 in the descriptor table): lo = hi = half = 0, center3 = its
 * centroid3, frame9 as computed.
 * VGS_E_ARG for another frame value and VGS_E_STATE before a run are decided locally (no collective).  A call with every array pointer NULL
 * only writes *K (no collective).  Otherwise the call is COLLECTIVE while this frame's table is not cached: after one vgs_tiles_run every
 * rank makes it.  Protocol (csrc/tiles.cpp): the global descriptor table through vgs_tiles_get_segment_descriptors' own path (nothing if
 * it is cached, else that call's one collective) -> this rank's extents of its own points (vgs_get_own_segment_extents, one small
 * pipeline on its GPU) -> ONE all_gather_varlen of 56-byte records (int32 label, int32 pad, lo[3], hi[3]) behind a header of record count
 * and status word -> the same host fold on every rank (vgs_tiles_fold_extents) -> half and centre on the rank's GPU
 * (vgs_segment_boxes_from_extents).  So the first box call costs at most two collectives, the other frame one more.  The table is cached
 * per frame and both frames may be cached at once: a cached call makes no collective and may be made by one rank alone; the next
 * vgs_tiles_run or vgs_tiles_set_points drops both.  Failures as in vgs_tiles_run: a rank whose local step fails still joins the exchange
 * with its status word, returns its own error, and every other rank returns VGS_E_PEER naming it (tests inject one with
 * VGS_TILES_FAIL_AT=boxes).  vgs_tiles_run itself gains no launch and no collective; point labels, descriptors and the graph are not
 * touched. */
vgs_status vgs_tiles_get_segment_boxes(vgs_tiles* t, int32_t frame, int64_t* K, double* center3, double* half3, double* frame9, double* lo3,
                                       double* hi3);
/* host wall time of the last box collective on this rank (the descriptor collective in front of it is not included), milliseconds: own
 * extents on the GPU (with upload and download), the exchange, the fold, the finish on the GPU (with upload and download), total */
enum { VGS_TILES_B_EXTENTS = 0, VGS_TILES_B_EXCHANGE = 1, VGS_TILES_B_FOLD = 2, VGS_TILES_B_FINISH = 3, VGS_TILES_B_TOTAL = 4, VGS_TILES_B_COUNT = 5 };
vgs_status vgs_tiles_get_box_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_B_COUNT */);
/* The extent fold on its own (host arithmetic, no context, no GPU; for tests): rank r's records are entries rec_off[r] .. rec_off[r+1] of
 * label / lo3 / hi3 (vgs_get_own_segment_extents).  Outputs: K rows, every pointer required for K > 0.  Per label, ranks in ascending
 * order: lo takes the smaller and hi the larger value (a zero keeps the sign met first); reached[k] = 1 if a record names k.  A row no
 * record reaches: +inf / -inf and reached = 0.  VGS_E_ARG for a label outside 0 .. K-1. */
vgs_status vgs_tiles_fold_extents(int world, const int64_t* rec_off, const int32_t* label, const double* lo3, const double* hi3, int64_t K,
                                  double* lo3_out, double* hi3_out, uint8_t* reached_out);
/* Per-segment statistics of point attributes the CALLER supplies, over all ranks: the tables, fields, types and NaN rules of
 * vgs_segment_field_stats and vgs_segment_class_histogram (include/vgs.h) with K = kept_global rows; row k covers exactly the points, over
 * all ranks, that vgs_tiles_get_point_labels labels k.  No attribute travels between ranks, only per-segment records: every point is
 * counted by the rank that loaded it (the rule of the tiled descriptors' n_points and of the tiled boxes), so a rank hands in one row per
 * point of its own load, in the order it gave them to vgs_tiles_set_points -- n must equal that call's n; channels, stride_bytes and the
 * class limits as in include/vgs.h.  Outputs are host arrays of K rows, any may be NULL; *K is written.  The _device variants read the
 * input from HBM in place (this rank's device, complete before the call).
 * Nothing is cached, because the input is the caller's: EVERY call is collective -- after one vgs_tiles_run every rank makes it, with
 * the same n_channels / n_classes -- and makes exactly ONE all_gather_varlen.  vgs_tiles_run gains no launch and no collective; labels,
 * descriptors, graph and boxes are not touched.
 * Field statistics (csrc/tiles.cpp): each rank's moments of its own rows (vgs_get_own_segment_field_moments, one small pipeline on its
 * GPU) -> one exchange of words of 8 bytes: a header of status word, record count and n_channels, then per record the label and per
 * channel n_valid, anchor, S1, S2 and min | max (1 + 5 n_channels words) -> the same host fold on every rank
 * (vgs_tiles_fold_field_moments) -> mean, var, vmin and vmax on the rank's GPU (vgs_segment_field_stats_from_moments: the finishing
 * kernel of vgs_segment_field_stats itself).  `anchor` is the folded table's own shift: per (k, channel) the anchor of the lowest rank
 * with a valid value.  Every rank receives the same bytes, bit-identical from call to call and from run to run on the same input and
 * layout; with one rank the table is vgs_segment_field_stats' byte for byte.
 * Histogram: each rank's rows (vgs_get_own_segment_class_counts) -> one exchange of int64 words (header of status word, record count and
 * n_classes; per record label, n_outside, hist[n_classes]) -> integer adds and the majority rule on the host
 * (vgs_tiles_fold_class_counts).
 * Failures.  VGS_E_STATE before a run is decided locally (no collective).  Everything a rank can get wrong on its own -- a wrong n, a NULL
 * input with n > 0, a bad channel, class or stride value, a failing context call, the injected VGS_TILES_FAIL_AT=fields -- travels in the
 * status word, so no peer waits: the failing rank returns its own status and message, the others VGS_E_PEER naming it.  Ranks that are
 * each valid but disagree on n_channels or n_classes all return VGS_E_ARG after the exchange; the message names the lowest rank that
 * differs from rank 0. */
vgs_status vgs_tiles_segment_field_stats(vgs_tiles* t, const float* field_host, int64_t n, int32_t n_channels, int64_t stride_bytes, int64_t* K,
                                         int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax);
vgs_status vgs_tiles_segment_field_stats_device(vgs_tiles* t, const float* field_dev, int64_t n, int32_t n_channels, int64_t stride_bytes,
                                                int64_t* K, int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax);
vgs_status vgs_tiles_segment_class_histogram(vgs_tiles* t, const int32_t* cls_host, int64_t n, int32_t n_classes, int64_t* K, int64_t* hist,
                                             int64_t* n_outside, int32_t* majority, int64_t* majority_count);
vgs_status vgs_tiles_segment_class_histogram_device(vgs_tiles* t, const int32_t* cls_dev, int64_t n, int32_t n_classes, int64_t* K, int64_t* hist,
                                                    int64_t* n_outside, int32_t* majority, int64_t* majority_count);
/* host wall time of the last attribute collective on this rank (field statistics or histogram, of the node labels or of a caller's point
 * labelling -- vgs_tiles_point_label_field_stats / _class_histogram stamp the same slots -- whichever came last), milliseconds: own
 * records on the GPU (with upload and download), the exchange, the fold, the finish on the GPU (with upload and download; 0 for the
 * histogram, whose majority rule is part of the fold), total */
enum { VGS_TILES_F_OWN = 0, VGS_TILES_F_EXCHANGE = 1, VGS_TILES_F_FOLD = 2, VGS_TILES_F_FINISH = 3, VGS_TILES_F_TOTAL = 4, VGS_TILES_F_COUNT = 5 };
vgs_status vgs_tiles_get_field_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_F_COUNT */);
/* that collective's payload on this rank: records of its own, bytes it put into the all-gather (header included, before padding) */
vgs_status vgs_tiles_get_field_payload(vgs_tiles* t, int64_t* own_records, int64_t* bytes_sent);
/* The attribute folds on their own (host arithmetic, no context, no GPU; for tests): rank r's records are entries rec_off[r] ..
 * rec_off[r+1] of the arrays vgs_get_own_segment_field_moments / vgs_get_own_segment_class_counts give.  Outputs: K rows, every pointer
 * required for K > 0.
 * Field moments, per (label, channel), ranks in ascending order: the anchor a is the anchor of the lowest rank with n_valid > 0, whose sums
 * are taken as they are; with delta = a_r - a in fp64 a later rank adds S1 += S1_r + n_r delta and S2 += S2_r + S1_r delta + delta S1_r
 * + n_r delta delta; n_valid adds; vmin / vmax take min / max.  An entry no valid value reaches: n_valid 0, anchor and sums 0, +inf / -inf.
 * Class counts: integer adds, then majority = the lowest class with the largest count, -1 and 0 when every count is 0.
 * VGS_E_ARG for a label outside 0 .. K-1. */
vgs_status vgs_tiles_fold_field_moments(int world, const int64_t* rec_off, const int32_t* label, int32_t n_channels, const int64_t* n_valid,
                                        const double* anchor, const double* s1, const double* s2, const float* vmin, const float* vmax, int64_t K,
                                        int64_t* n_valid_out, double* anchor_out, double* s1_out, double* s2_out, float* vmin_out, float* vmax_out);
vgs_status vgs_tiles_fold_class_counts(int world, const int64_t* rec_off, const int32_t* label, int32_t n_classes, const int64_t* hist,
                                       const int64_t* n_outside, int64_t K, int64_t* hist_out, int64_t* n_outside_out, int32_t* majority_out,
                                       int64_t* majority_count_out);
/* Score the segmentation against reference labels the CALLER supplies, over all ranks: the tables, fields, types, tie rules and summary of
 * vgs_compare_labels (include/vgs.h) with K = kept_global segment rows, over the points of all ranks -- byte for byte what one context
 * would give on the gathered points.  `ref` holds one int32 per point the rank gave to vgs_tiles_set_points, in that order (negative = not
 * annotated); n must equal that call's n.  *K, *n_cells, *n_refs and summary[12] may be NULL.  The _device variant reads ref from HBM in
 * place (this rank's device, complete before the call).
 * Protocol (csrc/tiles.cpp).  Every point is counted by the rank that loaded it; no label and no reference id travels, only cells
 * (L, g, n): the rank's cells over its own points (vgs_own_label_cells, one small pipeline on its GPU) -> ONE all_gather_varlen of int64
 * words: a header of status word, own cell count and own unannotated count, then per cell two words, (L + 1) << 32 | g and n -- 16 bytes
 * per cell -> the lists of all ranks, in rank order, are merged on the rank's GPU and the three tables and the summary are built there
 * (vgs_label_comparison_from_cells with the summed unannotated count); there is no host fold.  Every rank receives the same bytes.
 * Nothing is cached, because the input is the caller's: EVERY call is collective -- after one vgs_tiles_run every rank makes it -- and
 * makes exactly ONE all_gather_varlen.  vgs_tiles_run gains no launch and no collective; labels, descriptors, graph, boxes and attribute
 * tables are not touched.  One consequence of exchanging cells: a reference with one id per point has one cell per point, so the
 * exchange is then as large as the points themselves.  That is the caller's choice of ids, not a defect.
 * vgs_tiles_get_label_comparison copies the tables of the last tiled compare from the rank's context (the fourteen arrays of
 * vgs_get_label_comparison, sizes as the compare returned them, K rows for the segment table; any may be NULL).  It is not collective.
 * VGS_E_STATE when there is no compare since the last run or the last vgs_tiles_set_points.
 * Failures.  VGS_E_STATE before a run is decided locally (no collective).  Everything a rank can get wrong on its own -- a wrong n, a NULL
 * ref with n > 0, a failing context call, the injected VGS_TILES_FAIL_AT=compare -- travels in the status word, so no peer waits: the
 * failing rank returns its own status and message, the others VGS_E_PEER naming it. */
vgs_status vgs_tiles_compare_labels(vgs_tiles* t, const int32_t* ref_host, int64_t n, int64_t* K, int64_t* n_cells, int64_t* n_refs,
                                    int64_t* summary /* 12 */);
vgs_status vgs_tiles_compare_labels_device(vgs_tiles* t, const int32_t* ref_dev, int64_t n, int64_t* K, int64_t* n_cells, int64_t* n_refs,
                                           int64_t* summary /* 12 */);
vgs_status vgs_tiles_get_label_comparison(vgs_tiles* t, int32_t* cell_seg, int32_t* cell_ref, int64_t* cell_n, int32_t* ref_id,
                                          int64_t* ref_points, int64_t* ref_dropped, int32_t* ref_best_seg, int64_t* ref_best_n,
                                          double* ref_best_iou, int64_t* seg_annotated, int32_t* seg_refs, int32_t* seg_best_ref,
                                          int64_t* seg_best_n, double* seg_best_iou);
/* host wall time of the last tiled compare on this rank, milliseconds: own cells on the GPU (with upload and download), the exchange, the
 * tables on the GPU (with the upload of the gathered cells), total */
enum { VGS_TILES_C_OWN = 0, VGS_TILES_C_EXCHANGE = 1, VGS_TILES_C_TABLES = 2, VGS_TILES_C_TOTAL = 3, VGS_TILES_C_COUNT = 4 };
vgs_status vgs_tiles_get_compare_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_C_COUNT */);
/* that compare's payload on this rank: cells of its own, bytes it put into the all-gather (header included, before padding) */
vgs_status vgs_tiles_get_compare_payload(vgs_tiles* t, int64_t* own_cells, int64_t* bytes_sent);
/* Point-level label refinement over all ranks: the rule of vgs_refine_point_labels (include/vgs.h) applied to the whole scene over the
 * shared grid.  kept_label is the global label that vgs_tiles_get_point_labels reports, the nodes are the voxels of the shared grid, node
 * ids compare as on one context (every rank numbers its voxels in descending code order).  Each point is evaluated by the rank that
 * loaded it; the output is one int32 per point of the rank's own load, in the order given to vgs_tiles_set_points.  The concatenation over
 * the ranks equals, with ==, what the rule gives on the gathered points with those global labels.
 * Who refines what.  A rank refines a node when the node holds at least one point of its own load and the node's centre lies at most
 * reach = max(graph_size, 0.5001 voxel_size) outside the rank's region, per axis.  That covers the nodes the rank owns, the nodes whose
 * cube crosses its border (0.5001 voxel_size: the geometric part of the straddle test of the ownership pass) and the nodes of objects
 * that reach over a tile's edge by up to graph_size.  With points loaded by region it covers every point: a point lies inside the cube of
 * its voxel, so its rank owns the voxel or the cube reaches over the border into the rank's region.  Own points in any other node were
 * loaded further outside the region than that; their rows are not complete on this rank, so they keep their label of
 * vgs_tiles_get_point_labels and are counted in counts[4] (0 with points loaded by region, or within graph_size of it).
 * Why the rank holds what it needs.  A refined node's centre lies at most reach outside the region, per axis.  Its candidates lie within
 * graph_size of that centre, and their cubes end within reach + graph_size + 0.5 voxel_size of the border: with reach = graph_size that
 * is inside the halo of 2 graph_size + voxel_size, so the adjacency row is complete and every node in it carries the same record as on
 * its owner (the graph section above; a node's record and its used flag depend on its own points only).
 * What the rank lacks is the LABEL of a candidate another rank owns.  The run's boundary records bring it for the rows of owned used
 * voxels only; the rows of unused voxels (fill) and of voxels another rank owns reach further.  So every rank publishes (code, global
 * label) of its owned used voxels whose centre lies within reach + graph_size + 0.5 voxel_size of a border line of its region -- the
 * band; adjacent tiles share their border lines, so a candidate within reach + graph_size of a neighbour's region is in its owner's
 * band.  The effective label of a voxel is its own label for an owned used voxel and an entry of the refinement's halo table for any
 * other: the band records of the other ranks and, for codes they do not name, the run's boundary records.  That table is separate from
 * the segment graph's, so neither call invalidates the other.  A used candidate whose label is still unknown fails the call on that rank
 * (VGS_E_UNSUPPORTED, the count in the message) instead of changing the result.
 * EVERY call is COLLECTIVE -- after one vgs_tiles_run every rank makes it, with the same parameters -- and makes exactly ONE
 * all_gather_varlen of 16-byte records (uint64 code, int32 label, int32 pad) behind a header of two such entries: status word and fill,
 * record count and the bits of patch_radius and switch_ratio.  The records are compacted on the device in ascending voxel id, so the
 * payload has the same bytes from call to call.  The first call after a run carries the band; the table is kept until the next
 * vgs_tiles_run or vgs_tiles_set_points and later calls send the header only.  rp == NULL: vgs_refine_params_default of the context.
 * counts (may be NULL), all this rank's share, each adds over the ranks to the whole scene's figure: 0 owned working nodes, 1 own points
 * examined, 2 own labelled points changed, 3 own unlabelled points filled, 4 own points left unrefined beyond the strip.  No float
 * atomics: the output is bit-identical from call to call.  vgs_tiles_run gains no launch and no collective; point labels, descriptors,
 * graph, boxes, attribute tables and comparison are not touched.
 * vgs_tiles_get_refined_labels copies the labels of the last refine (n int32); it is not collective.  VGS_E_STATE without a refine since
 * the last run or the last vgs_tiles_set_points.
 * Failures.  VGS_E_STATE before a run is decided locally (no collective).  A bad parameter (negative or non-finite patch_radius,
 * switch_ratio outside [0, 1]) and the injected VGS_TILES_FAIL_AT=refine travel in the status word: the failing rank returns its own
 * status and message, the others VGS_E_PEER naming it.  Ranks that are each valid but disagree on a parameter all return VGS_E_ARG after
 * the exchange; the message names the lowest rank that differs from rank 0.  A failure of the local refinement behind the exchange (the
 * unknown label above) is returned by that rank and travels in the status word of its next collective. */
vgs_status vgs_tiles_refine_point_labels(vgs_tiles* t, const vgs_refine_params* rp /* NULL: the context's defaults */, int64_t* counts /* 5 */);
vgs_status vgs_tiles_get_refined_labels(vgs_tiles* t, int32_t* labels /* n */);
/* host wall time of the last refine on this rank, milliseconds: own band records on the GPU (with their download; 0 records after the
 * first call), the exchange, the halo table (list, upload, lookup), the refinement on the GPU, total */
enum { VGS_TILES_R_BAND = 0, VGS_TILES_R_EXCHANGE = 1, VGS_TILES_R_TABLE = 2, VGS_TILES_R_REFINE = 3, VGS_TILES_R_TOTAL = 4, VGS_TILES_R_COUNT = 5 };
vgs_status vgs_tiles_get_refine_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_R_COUNT */);
/* that refine's payload on this rank: band records it sent, bytes it put into the all-gather (header included, before padding) */
vgs_status vgs_tiles_get_refine_payload(vgs_tiles* t, int64_t* band_records, int64_t* bytes_sent);
/* Tables of ANY per-point labelling the caller supplies, over all ranks: the refined labels of vgs_tiles_get_refined_labels, ground-truth
 * instances, anything made from the driver's output.  The rows, fields, types and rules are those of vgs_point_label_descriptors,
 * vgs_point_label_boxes and vgs_compare_point_labels (include/vgs.h) with K rows of the caller's, over the points of all ranks.  `labels`
 * holds one int32 per point the rank gave to vgs_tiles_set_points, in that order; n must equal that call's n.  Label l belongs to row l
 * for 0 <= l < K, a negative label to no row, a label >= K is VGS_E_ARG; 0 <= K <= 2^31 - 1, the same on every rank.  Every output may be
 * NULL.  The _device variants read the labelling (and ref) from HBM in place (this rank's device, complete before the call).
 * Protocol (csrc/tiles.cpp).  Every point is handled by the rank that loaded it; no point, label or id leaves its rank, only per-label
 * records; every rank receives the same bytes; there are no float atomics, so the tables are bit-identical from call to call and run to
 * run.  Nothing is cached, because the input is the caller's: EVERY call is collective, K = 0 included (the ranks still agree on
 * n_skipped).  vgs_tiles_run gains no launch and no collective; the run, the cached descriptor, box and graph tables and the refine halo
 * table are not touched.
 *   vgs_tiles_point_label_descriptors  ONE all_gather_varlen of 128-byte entries: a header (status word, moment-record count, K,
 *     pair-record count, own n_skipped), this rank's moment records of its own points (vgs_own_point_label_moments, one small pipeline on
 *     its GPU; the MomentRec wire format of the descriptor exchange), then its 16-byte pair records (uint64 voxel code, int32 label, int32
 *     pad), eight to an entry.  Behind it, the same on every rank: vgs_tiles_fold_moments, unchanged; vgs_tiles_fold_label_pairs;
 *     n_nodes = folded n_nodes + n_nodes_add; the per-segment algebra on the rank's GPU (vgs_segment_descriptors_from_moments).
 *     *n_skipped is the sum over the ranks.  A label no point carries on any rank gives the empty row of vgs_point_label_descriptors.
 *   n_nodes counts the distinct voxels of the shared grid among a label's points over ALL ranks, once: a rank counts the voxels that
 *     hold none of another rank's points and sends (code, label) for those that do (include/vgs.h, vgs_own_point_label_moments); the
 *     distinct pairs are counted behind the exchange.  With points loaded by region every rank that loaded a point of a straddling voxel
 *     sees the others' points of it inside its halo, so all of them send the pair and it is counted exactly once.  With points outside
 *     a rank's region a straddling voxel may be counted twice in n_nodes; every other field stays exact.
 *   vgs_tiles_point_label_boxes  TWO collectives: the descriptor exchange above, of THIS labelling; then one all_gather_varlen of the
 *     56-byte extent records of the box exchange (vgs_get_own_point_label_extents), folded by vgs_tiles_fold_extents unchanged and
 *     finished by vgs_segment_boxes_from_extents.  Nothing outlives the call.
 *   vgs_tiles_compare_point_labels  ONE collective: the cell exchange of vgs_tiles_compare_labels (K as one more word behind the cells),
 *     fed by vgs_own_point_label_cells, then vgs_label_comparison_from_cells.  The tables become the driver's last comparison:
 *     vgs_tiles_get_label_comparison serves them, with K rows for the segment table.
 * Failures.  VGS_E_STATE before a run is decided locally (no collective).  Everything a rank can get wrong on its own -- a wrong n, a NULL
 * labelling with n > 0, K out of range, a label >= K (the message names the first offending index and its value), a bad frame, a failing
 * context call, the injected VGS_TILES_FAIL_AT=point_labels -- travels in the status word, so no peer waits: the failing rank returns its
 * own status and message, the others VGS_E_PEER naming it.  Ranks that are each valid but pass different K all return VGS_E_ARG after the
 * exchange; the message names the lowest rank that differs from rank 0. */
vgs_status vgs_tiles_point_label_descriptors(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_skipped, int64_t* n_points,
                                             int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3, double* evecs9,
                                             float* eigen8);
vgs_status vgs_tiles_point_label_descriptors_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_skipped,
                                                    int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6,
                                                    double* evals3, double* evecs9, float* eigen8);
vgs_status vgs_tiles_point_label_boxes(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int32_t frame, double* center3, double* half3,
                                       double* frame9, double* lo3, double* hi3);
vgs_status vgs_tiles_point_label_boxes_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int32_t frame, double* center3,
                                              double* half3, double* frame9, double* lo3, double* hi3);
vgs_status vgs_tiles_compare_point_labels(vgs_tiles* t, const int32_t* seg_labels_host, int64_t K, const int32_t* ref_host, int64_t n, int64_t* n_cells,
                                          int64_t* n_refs, int64_t* summary /* 12 */);
vgs_status vgs_tiles_compare_point_labels_device(vgs_tiles* t, const int32_t* seg_labels_dev, int64_t K, const int32_t* ref_dev, int64_t n,
                                                 int64_t* n_cells, int64_t* n_refs, int64_t* summary /* 12 */);
/* Field statistics and class histogram of ANY per-point labelling the caller supplies, over all ranks: the tables, fields, types and NaN
 * rules of vgs_point_label_field_stats and vgs_point_label_class_histogram (include/vgs.h) with K rows of the caller's, over the points of
 * all ranks -- mean intensity or majority class of the REFINED segments of a tiled scene, which the node tables above cannot give (a
 * boundary voxel holds two or three refined labels).  labels, field and cls hold one row per point the rank gave to vgs_tiles_set_points,
 * in that order; n must equal that call's n.  Label rules as vgs_tiles_point_label_descriptors; channels, stride_bytes, classes and the
 * limit of 2^27 entries (VGS_E_UNSUPPORTED) as in include/vgs.h.  Outputs are host arrays of K rows, any may be NULL.  The _device variants
 * read both inputs from HBM in place (this rank's device, complete before the call).
 * Protocol (csrc/tiles.cpp).  No point, label or attribute leaves its rank; every point is counted once, by the rank that loaded it.  No
 * field counts nodes, so a voxel that holds points of several ranks needs no pair records: the folds add per-point quantities only.
 * Nothing is cached: EVERY call is collective, K = 0 included (the ranks still agree on n_skipped), and makes exactly ONE
 * all_gather_varlen of 8-byte words: a header of five words (status word, record count, n_channels or n_classes, K, the rank's own
 * n_skipped), then the rank's records of its own points (vgs_own_point_label_field_moments / vgs_own_point_label_class_counts, one sort
 * and one small pipeline on its GPU) in the wire format of the two exchanges above, unchanged.  Behind it, the same on every rank:
 * vgs_tiles_fold_field_moments then vgs_segment_field_stats_from_moments, or vgs_tiles_fold_class_counts (the majority rule is part of the
 * fold); both folds unchanged.  *n_skipped is the sum over the ranks.  `anchor` is the folded table's own shift: per (k, channel) the
 * anchor of the lowest rank with a valid value.  A label no point carries on any rank gives the empty row of the single-context calls.
 * Every rank receives the same bytes, bit-identical from call to call and run to run; with one rank the table is the single context's byte
 * for byte.  vgs_tiles_run gains no launch and no collective; the run, all cached tables and the refine halo table are not touched.
 * Failures.  VGS_E_STATE before a run is decided locally (no collective).  Everything a rank can get wrong on its own -- a wrong n, a NULL
 * array with n > 0, bad channels, classes or stride, K out of range, a label >= K (the message names the first offending index and its
 * value), a failing context call, the injected VGS_TILES_FAIL_AT=point_labels -- travels in the status word: the failing rank returns its
 * own status and message, the others VGS_E_PEER naming it.  Ranks that are each valid but disagree on K, n_channels or n_classes all
 * return VGS_E_ARG after the exchange; the message names the lowest rank that differs from rank 0.
 * The calls stamp the slots of vgs_tiles_get_field_times and vgs_tiles_get_field_payload. */
vgs_status vgs_tiles_point_label_field_stats(vgs_tiles* t, const int32_t* labels_host, int64_t K, const float* field_host, int64_t n, int32_t n_channels,
                                             int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor, double* mean, double* var,
                                             float* vmin, float* vmax);
vgs_status vgs_tiles_point_label_field_stats_device(vgs_tiles* t, const int32_t* labels_dev, int64_t K, const float* field_dev, int64_t n,
                                                    int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor,
                                                    double* mean, double* var, float* vmin, float* vmax);
vgs_status vgs_tiles_point_label_class_histogram(vgs_tiles* t, const int32_t* labels_host, int64_t K, const int32_t* cls_host, int64_t n, int32_t n_classes,
                                                 int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority, int64_t* majority_count);
vgs_status vgs_tiles_point_label_class_histogram_device(vgs_tiles* t, const int32_t* labels_dev, int64_t K, const int32_t* cls_dev, int64_t n,
                                                        int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority,
                                                        int64_t* majority_count);
/* host arithmetic only, no context (tests): per label 0 .. K-1 the number of distinct (code, label) pairs among the pair records of all
 * ranks, rec_off[r] .. rec_off[r + 1] being rank r's.  VGS_E_ARG for a label outside 0 .. K-1. */
vgs_status vgs_tiles_fold_label_pairs(int world, const int64_t* rec_off /* world + 1 */, const uint64_t* code, const int32_t* label, int64_t K,
                                      int32_t* n_nodes_add /* K */);
/* host wall time of the last descriptor or box call of a point labelling on this rank, milliseconds (a box call: both of its collectives
 * added): own records on the GPU (with upload and download), the exchange, the host fold, the finish on the GPU, total */
enum { VGS_TILES_L_OWN = 0, VGS_TILES_L_EXCHANGE = 1, VGS_TILES_L_FOLD = 2, VGS_TILES_L_FINISH = 3, VGS_TILES_L_TOTAL = 4, VGS_TILES_L_COUNT = 5 };
vgs_status vgs_tiles_get_point_label_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_L_COUNT */);
/* that call's payload on this rank: moment records and pair records of its own, bytes it put into the all-gathers (headers included,
 * before padding) */
vgs_status vgs_tiles_get_point_label_payload(vgs_tiles* t, int64_t* own_records, int64_t* own_pairs, int64_t* bytes_sent);
/* Connected parts of ANY per-point labelling the caller supplies, over all ranks: is a refined segment, or a semantic class, of a scene
 * larger than one GPU one object or several?  A part that crosses a tile border is invisible to any single rank.
 * Definition: that of vgs_point_label_components (include/vgs.h) over the whole scene; the nodes are the voxels of the shared grid.
 *   Vertices.  The distinct pairs (label, voxel code) with at least one point, on any rank, that carries the label in that voxel.  A voxel
 *     that holds points of several ranks under the same label is ONE vertex.
 *   Edges.  As on one context: (l, v) and (l, w) are joined when w is in v's adjacency row or v in w's.
 *   Numbering.  Ascending (label, smallest node id of the part).  Every rank numbers voxels in descending code order, so this is ascending
 *     label, then DESCENDING largest voxel code of the part.
 * The result equals what one context's vgs_point_label_components gives on the gathered points (the ranks' loads concatenated in rank
 * order, the order the shared grid is chained in): part_of_point concatenated over the ranks, part_label, part_points, part_nodes,
 * label_first, label_largest, n_parts and n_skipped (the sum over the ranks).  part_first_node means nothing across ranks; the table gives
 * part_first_code instead, the shared-grid code of that node.  Everything is integer; every rank receives the same bytes, bit-identical
 * from call to call and from run to run.  labels: one int32 per point the rank gave to vgs_tiles_set_points, in that order; n must equal
 * that call's n; label rules as vgs_tiles_point_label_descriptors.  The _device variant reads the labels from HBM in place.
 * Precondition, as for vgs_tiles_refine_point_labels and n_nodes: the points are loaded by region.  Outside it the rows of a node further
 * outside the rank's region than graph_size are not complete on the rank, and a part may come apart there.
 * Protocol (csrc/tiles.cpp, csrc/labelcc_tiles.hip): TWO all_gather_varlen of 8-byte words per call, K = 0 included; nothing is cached.
 *   1. Own parts on each rank's GPU (vgs_own_point_label_parts): the pass of one context over the rank's own points.  Complete because an
 *      own vertex's node holds an own point, so its cube meets the region; its row ends within graph_size + voxel_size of the border,
 *      inside the halo of 2 graph_size + voxel_size.
 *   2. Exchange 1: a header of four words (status word, band count, K, own n_skipped), then two words a BAND record (code; label << 32 |
 *      local part).  The band: the own vertices whose node centre lies within near = graph_size + voxel_size of a border line of the
 *      region.  That is enough: a vertex w of another rank adjacent to v holds a point of that rank's region, so w's centre is outside
 *      this region or at most half a voxel inside it, and v is within graph_size of it per axis.  Outer tiles are open ended, and an
 *      infinite border never matches.
 *   3. Cross links on each rank's GPU (vgs_link_point_label_parts) over the OTHER ranks' band records: for every own band vertex (l, v) and
 *      every neighbour w != v of v's row, one triple (own local part, rank, part) for every record with key (l, w); sorted and unique.
 *      Each rank walks only the rows of its own vertices, which are complete on it: r finds w in row(v), s finds v in row(w), and the
 *      union over the ranks is the "either row" rule.  A stored row pruned to used neighbours is covered by the other side's full row.
 *   4. Exchange 2: a header of four words (status word -- a failure of step 3 travels here --, part count, link count, K), three words a
 *      local part (label << 32 | nodes; points; code of its first node), two words a link (own part << 32 | rank; part).
 *   5. The same host fold on every rank (vgs_tiles_fold_label_parts): a union-find over (rank, local part), united along the links and
 *      along EQUAL (code, label) keys among the band records of different ranks -- the shared voxel, which always lies in both bands.  A key
 *      with m records is one node: m - 1 comes off the merged part's node count.  Label, points (sum), nodes (sum - surplus), first code
 *      (max); sorted by (label ascending, first code descending); label_first; label_largest (most points, lowest id on a tie).
 *   6. vgs_apply_point_label_part_ids: one gather writes the part id of every own point, in the order of the rank's load.
 * The result is kept, like the refined labels, until the next call, the next run or the next vgs_tiles_set_points;
 * vgs_tiles_get_point_label_components copies it out (part_of_point: n entries of this rank; the tables: n_parts rows, K + 1 and K
 * rows); any pointer may be NULL; it is not collective and answers VGS_E_STATE without a result.  vgs_tiles_run gains no launch and no
 * collective; the call invalidates no cached descriptor, box or graph table, no refine halo table, not the refined labels, and does not
 * change the last comparison.
 * Failures: the contract of vgs_tiles_point_label_descriptors.  VGS_E_STATE before a run is decided locally (no collective).  A wrong n, a
 * NULL labelling, K out of range, a label >= K (the message names the first offending index and its value), a failing context call and
 * the injected VGS_TILES_FAIL_AT=components travel in the status word of exchange 1: the failing rank returns its own status and message,
 * the others VGS_E_PEER naming it.  Ranks that are each valid but disagree on K all return VGS_E_ARG behind exchange 1. */
vgs_status vgs_tiles_point_label_components(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_skipped);
vgs_status vgs_tiles_point_label_components_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_skipped);
vgs_status vgs_tiles_get_point_label_components(vgs_tiles* t, int32_t* part_of_point /* n */, int32_t* part_label, int64_t* part_points,
                                                int32_t* part_nodes, uint64_t* part_first_code, int64_t* label_first, int32_t* label_largest);
/* host arithmetic only, no context (tests): step 5 on flattened per-rank records, rank r's entries being off[r] .. off[r + 1] of the local
 * parts, the band records and the links.  map: the global part of every local part (part_off[world] entries); the out_ tables hold at
 * most part_off[world] rows, *n_parts of them written; label_first K + 1 and label_largest K rows.  Any output may be NULL.  VGS_E_ARG
 * for a label outside 0 .. K-1, a link or band record naming a part that does not exist, or a link between different labels. */
vgs_status vgs_tiles_fold_label_parts(int world, int64_t K, const int64_t* part_off, const int32_t* part_label, const int64_t* part_points,
                                      const int32_t* part_nodes, const uint64_t* part_first_code, const int64_t* band_off, const uint64_t* band_code,
                                      const int32_t* band_label, const int32_t* band_part, const int64_t* link_off, const int32_t* link_own,
                                      const int32_t* link_rank, const int32_t* link_part, int64_t* n_parts, int32_t* map, int32_t* out_label,
                                      int64_t* out_points, int32_t* out_nodes, uint64_t* out_first_code, int64_t* label_first, int32_t* label_largest);
/* host wall time of the last components call on this rank, milliseconds: own parts on the GPU (with upload and download), exchange 1,
 * the link step on the GPU, exchange 2, the host fold, the part ids on the GPU, total */
enum { VGS_TILES_CC_OWN = 0, VGS_TILES_CC_EXCHANGE1 = 1, VGS_TILES_CC_LINK = 2, VGS_TILES_CC_EXCHANGE2 = 3, VGS_TILES_CC_FOLD = 4, VGS_TILES_CC_APPLY = 5,
       VGS_TILES_CC_TOTAL = 6, VGS_TILES_CC_COUNT = 7 };
vgs_status vgs_tiles_get_point_label_component_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_CC_COUNT */);
/* that call's payload on this rank: band records, local parts and link triples of its own, bytes it put into the two all-gathers */
vgs_status vgs_tiles_get_point_label_component_payload(vgs_tiles* t, int64_t* band_records, int64_t* parts, int64_t* links, int64_t* bytes_sent);
/* Adjacency graph of ANY per-point labelling the caller supplies, over all ranks: which refined segments, parts or classes of a scene
 * larger than one GPU touch, across how much boundary and how strongly (vgs_tiles_get_segment_graph describes the voxel labels only).
 * Definition: that of vgs_point_label_graph (include/vgs.h) over the whole scene, the nodes being the voxels of the shared grid.  Every
 * rank receives the same table with the fields, types, edge order and NaN rules of vgs_get_point_label_graph.  It equals what one
 * context's vgs_point_label_graph gives on the gathered points (the ranks' loads concatenated in rank order): seg_ab, n_shared, n_pairs,
 * n_finite, nodes_ab, w_min, w_max byte for byte; w_sum within 1e-10 relative, because the ranks' partial sums are added in rank order
 * and the summation shape differs from one context's.  With one rank the table is the single context's byte for byte, w_sum included.
 * The table is bit-identical from call to call.  n_skipped is the sum over the ranks.  VGS only.  No point and no label of a point leaves
 * its rank.  labels, n, K and the _device variant: as vgs_tiles_point_label_components; so is the precondition (points loaded by region).
 * COUNTING RULE.  Every voxel of the shared grid has exactly one owner, the rank whose region holds its centre (vgs_compute_owned).  A
 * vertex (label, node) exists when any rank holds a point with that label in that node.  EVERY RECORD OF csrc/labelgraph.hip LIVES ON
 * THE RANK THAT OWNS THE NODE OF THE VERTEX IT SPEAKS FOR -- a vertex's own per-label records and the proxy records written on its
 * behalf alike.  Hence:
 *   Contacts.  A contact {(A, u), (B, x)} is counted by the walker of its counting side exactly as on one context (the walker of u counts
 *     it at entry x when u < x or x's row lacks u), and that walker runs on owner(u) only.  Node ids are in descending code order of the
 *     same grid on every rank, so the comparison agrees across ranks; with VGS "x's row holds u" depends on whether x is used alone, and
 *     node records of halo voxels equal their owner's, so the predicate agrees as well.
 *   Shared nodes.  A shared node is counted by its owner.
 *   nodes_ab.  A vertex's own record and all its proxies are on one rank, so the fold's "first record of a vertex counts it" rule counts
 *     it once over all ranks.  A proxy arises only under pruned stored rows, from the built row of an unused node x towards a used node u:
 *     on owner(u) the vertices at NON-OWNED unused nodes of the merged list walk their built rows in a proxy-only mode (no record of
 *     their own, no counts, only proxies whose target node is owned), and a vertex at an owned node writes no proxy whose target node it
 *     does not own.  Without pruned rows no non-owned vertex walks.
 * What a rank needs for this is the complete label set of every owned node and of every node adjacent to one.  Labels of its own points
 * it has; labels carried by another rank's points arrive as that rank's band records (code, label) -- the band of
 * vgs_tiles_point_label_components: own vertices whose node centre lies within graph_size + voxel_size of a border line (DESIGN.md 8 has
 * the argument).
 * Protocol (csrc/tiles.cpp, csrc/labelgraph_tiles.hip): TWO all_gather_varlen per call, K <= 1 included; nothing is cached.
 *   1. Own pass on each rank's GPU (vgs_own_point_label_band): the (label, node) vertices of the own points, the band records.
 *   2. Exchange 1: a header record (status word, band count, K, own n_skipped), then 16 bytes a band record (code, label).
 *   3. Merged vertices and 4. the walk on each rank's GPU (vgs_own_point_label_graph): the other ranks' records looked up in the local
 *      grid (a code the rank does not hold drops out), concatenated with the own vertices, sorted, unique -- a vertex two ranks publish is
 *      one vertex; then the walk in tile mode and the unchanged sort, chunk and fold pipeline give the rank's partial table.
 *   5. Exchange 2: a header record (status word, record count), then 56 bytes an edge of the partial table.
 *   6. The same host fold on every rank (vgs_tiles_fold_label_edges): the tables merged by (a, b), ranks in ascending order; n_shared,
 *      n_pairs, n_finite and nodes_ab add, w_sum adds in fp64 in rank order, the extrema come from the ranks with n_finite > 0.
 * The table is kept until the next call, the next run or the next vgs_tiles_set_points; vgs_tiles_get_point_label_graph copies it out
 * (n_edges rows; any pointer may be NULL), is not collective and answers VGS_E_STATE without a result.  vgs_tiles_run gains no launch
 * and no collective.  The call's own pass overwrites the vertex arrays of vgs_tiles_point_label_components' own pass, so it drops that
 * call's result (vgs_tiles_get_point_label_components answers VGS_E_STATE until the next components call); a components call leaves the
 * graph's table alone.  No other cached table is touched.
 * Failures: the contract of vgs_tiles_point_label_components.  VGS_E_STATE before a run is decided locally.  A local failure of step 1
 * and the injected VGS_TILES_FAIL_AT=label_graph travel in the header of exchange 1, a failure of steps 3 and 4 in that of exchange 2:
 * the failing rank returns its own status and message, the others VGS_E_PEER naming it.  Ranks that disagree on K all return VGS_E_ARG. */
vgs_status vgs_tiles_point_label_graph(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped);
vgs_status vgs_tiles_point_label_graph_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped);
vgs_status vgs_tiles_get_point_label_graph(vgs_tiles* t, int32_t* seg_ab, int64_t* n_shared, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                           double* w_sum, float* w_min, float* w_max);
/* host arithmetic only, no context (tests): step 6 on flattened per-rank partial tables, rank r's edges being rec_off[r] ..
 * rec_off[r + 1].  The outputs hold at most rec_off[world] rows, *n_edges of them written; any output array may be NULL.  VGS_E_ARG for
 * a label outside 0 .. K-1, a >= b, or a rank table that is not strictly ascending in (a, b). */
vgs_status vgs_tiles_fold_label_edges(int world, int64_t K, const int64_t* rec_off /* world + 1 */, const int32_t* seg_ab, const int64_t* n_shared,
                                      const int64_t* n_pairs, const int64_t* n_finite, const int32_t* nodes_ab, const double* w_sum,
                                      const float* w_min, const float* w_max, int64_t* n_edges, int32_t* seg_ab_out, int64_t* n_shared_out,
                                      int64_t* n_pairs_out, int64_t* n_finite_out, int32_t* nodes_ab_out, double* w_sum_out, float* w_min_out,
                                      float* w_max_out);
/* host wall time of the last label-graph call on this rank, milliseconds: the own pass on the GPU (with upload and download), exchange
 * 1, the partial table on the GPU, exchange 2, the host fold, total */
enum { VGS_TILES_LG_OWN = 0, VGS_TILES_LG_EXCHANGE1 = 1, VGS_TILES_LG_TABLE = 2, VGS_TILES_LG_EXCHANGE2 = 3, VGS_TILES_LG_FOLD = 4, VGS_TILES_LG_TOTAL = 5,
       VGS_TILES_LG_COUNT = 6 };
vgs_status vgs_tiles_get_label_graph_times(vgs_tiles* t, double* ms, int32_t n /* <= VGS_TILES_LG_COUNT */);
/* that call's payload on this rank: band records of its own, other ranks' records whose code it found in its grid, edges of its partial table,
 * bytes it put into the two all-gathers */
vgs_status vgs_tiles_get_label_graph_payload(vgs_tiles* t, int64_t* band_records, int64_t* foreign_hits, int64_t* own_edges, int64_t* bytes_sent);
/* the rank's engine context (read-only use: counts, stage times) */
vgs_ctx* vgs_tiles_context(vgs_tiles* t);

#ifdef __cplusplus
}
#endif
#endif /* VGS_TILES_H_ */
