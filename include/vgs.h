/* include/vgs.h -- C-ABI of the MI355X-native VGS / SVGS segmentation engine (libvgs_hip.so).
 *
 * Drop-in boundary for the hot path of Yusheng-Xu/VGS-SVGS-Segmentation.  The reference has no
 * FFI layer: its boundary is the public surface of two header-only class templates plus the
 * Task_File line indices.  Each entry point below names the reference member
 * function(s) it replaces (paths under the reference repo):
 *   VS: = voxel_segmentation.h   SS: = supervoxel_segmentation.h   T: = test   IOC: = point_clouds_IO.cpp
 * include/vgs_segmentation.hpp re-creates the two classes (same method names and call order) on top
 * of these functions; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes only; all outputs are caller-allocated (size query first);
 * every function returns a vgs_status; a context owns one HIP stream and is not re-entrant.
 * There is no CPU fallback: without a HIP device vgs_create fails with VGS_E_HIP.
 */
#ifndef VGS_H_
#define VGS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  VGS_OK = 0,
  VGS_E_ARG = 1,          /* bad argument */
  VGS_E_STATE = 2,        /* call-order contract violated (getVoxelNum before attributes ...) */
  VGS_E_HIP = 3,          /* HIP runtime error / no device */
  VGS_E_NOMEM = 4,
  VGS_E_UNSUPPORTED = 5,  /* configuration outside the built kernels' limits (message says which) */
  VGS_E_IO = 6,
  VGS_E_PEER = 7          /* tiled driver (vgs_tiles.h): another rank reported a failure; this rank stopped with it */
} vgs_status;

/* Parameter surface = Task_File_VGS.txt / Task_File_SVGS.txt (T:25-37, T:108-125). */
typedef struct {
  int32_t method;        /* 2 = VGS, 3 = SVGS (task line 24) */
  float voxel_size;      /* line 28 */
  float graph_size;      /* VGS line 30, SVGS line 32 */
  float sig_p, sig_n, sig_o, sig_e, sig_c, sig_w;
  float cut_thred;
  int32_t points_min, adjacency_min, voxels_min;
  float seed_size;       /* SVGS line 30 */
  float color_impt, spatial_impt, normal_impt; /* SVGS sig_a, sig_b, sig_c(2nd) lines 46,48,50 */
  int32_t q7_count_as_index; /* 1 = reproduce closestCheck reading the neighbour count as a voxel id (VS:2243) */
  int32_t device;        /* HIP device ordinal */
  int32_t vccs_mode;     /* svgs_supervoxels: 1 (the default of vgs_params_default_svgs since round 6) = pcl::SupervoxelClustering's own
                          * order: supervoxels take their turns one after the other in label order, 2-ring normals, seed rejection, the
                          * adjacency octree's own lattice, refineNormals, re-seeding by the nearest of all voxels;
                          * 0 = a faster synchronous variant (every voxel decides from the state at the start of a round): a DIFFERENT
                          * algorithm whose final segments are not within P2 of mode 1's (csrc/vccs.hip; unpinned against PCL either way) */
} vgs_params;

typedef struct vgs_ctx vgs_ctx;

/* counts returned by vgs_get_counts */
enum {
  VGS_N_POINTS = 0,      /* getCloudPointNum()  VS:94 */
  VGS_N_FINITE = 1,      /* points that entered the octree */
  VGS_N_VOXELS = 2,      /* getVoxelNum()       VS:104 */
  VGS_N_USED = 3,        /* voxels with > points_min points (VS:322) */
  VGS_N_ADJ = 4,         /* sum of adjacency list lengths over used voxels */
  VGS_N_CLUSTERS = 5,    /* getClusterNum()     VS:111 (all clusters, singletons included) */
  VGS_N_KEPT = 6,        /* clusters with > voxels_min voxels = getClusterIdx().size()  VS:969 */
  VGS_N_PAIRS = 7,       /* pair affinities evaluated by the local-graph kernel */
  VGS_N_DEPTH = 8,       /* octree depth */
  VGS_N_ISOLATED = 9,    /* closestCheck candidates */
  VGS_N_REATTACHED = 10, /* closestCheck successes */
  VGS_N_SUPERVOXELS = 11,
  VGS_N_COUNTS = 16
};

/* stage timers (milliseconds, HIP events on the context's stream) */
enum {
  VGS_T_VOXELIZE = 0, VGS_T_FEATURES = 1, VGS_T_ADJACENCY = 2, VGS_T_LOCALCUT = 3 /* incl. its hand-over kernels that end inside the merge stage */, VGS_T_MERGE = 4,
  VGS_T_LABELS = 5 /* cluster filter + voxel and point labels: the last part of VGS_T_MERGE, not added to the total again */, VGS_T_TOTAL = 6, VGS_T_LOCALCUT_KERNEL = 7, VGS_T_SUPERVOXEL = 8,
  VGS_T_LOCALCUT_BULK = 9, /* the one launch of the bulk-class local-cut kernel (k_localcut_wave<96,448,1>), HIP events on its stream */
  VGS_T_COUNT = 12
};

/* ---- parameters ------------------------------------------------------------------------ */
vgs_status vgs_params_default_vgs(vgs_params* p);   /* Task_File_VGS.txt values  */
vgs_status vgs_params_default_svgs(vgs_params* p);  /* Task_File_SVGS.txt values */
/* inputTaskTxtFile + the fixed line indices of segmentationVGS/SVGS (IOC:148-169, T:25-37, T:108-125);
 * strips CR; in_name/out_name (may be NULL) receive lines 15 and 21. */
vgs_status vgs_parse_task_file(const char* path, vgs_params* p, char* in_name, char* out_name, int name_cap);

/* ---- lifetime -------------------------------------------------------------------------- */
/* VoxelBasedSegmentation(res) / SuperVoxelBasedSegmentation(res) ctor + setVoxelSize (+ setSupervoxelSize,
 * setGraphSize) (VS:84,124  SS:85,143-164) */
vgs_status vgs_create(const vgs_params* p, vgs_ctx** out);
void vgs_destroy(vgs_ctx* ctx);
/* The reference passes parameters when a stage is called (setVoxelSize VS:124, findAllVoxelAdjacency(graph_size)
 * VS:223, segmentVoxelCloudWithGraphModel(cut, sigmas) VS:372).  Replaces the context's parameters; stages whose
 * inputs changed must be re-run (the context's stage state is rolled back accordingly). method/device are fixed. */
vgs_status vgs_set_params(vgs_ctx* ctx, const vgs_params* p);
const char* vgs_last_error_string(const vgs_ctx* ctx); /* ctx may be NULL: last create error */

/* ---- input: setInputCloud + getCloudPointNum (T:52-53, VS:94) ---------------------------- */
/* stride_bytes 12 (packed xyz) or 16 (pcl::PointXYZ).  Host variant copies once to HBM. */
vgs_status vgs_set_points(vgs_ctx* ctx, const float* xyz_host, int64_t n, int32_t stride_bytes);
/* device variant: no copy, the caller keeps the buffer alive and unchanged until results are read */
vgs_status vgs_set_points_device(vgs_ctx* ctx, const float* xyz_dev, int64_t n, int32_t stride_bytes);

/* A sequence of clouds (no reference counterpart: the reference loads one PCD, T:41-49).  vgs_stage_points starts the copy
 * of the NEXT cloud into the context's second input buffer on a copy stream and returns at once; the current cloud, its
 * stages and its results stay untouched.  vgs_commit_points makes the staged cloud the current one, like vgs_set_points
 * without the host-side wait (the stages' stream waits for the copy on the device).  The host buffer must stay unchanged
 * until the commit's first stage has run; pinned memory (vgs_host_alloc / vgs_host_register) makes the copy asynchronous
 * and about twice as fast, pageable memory works. */
vgs_status vgs_stage_points(vgs_ctx* ctx, const float* xyz_host, int64_t n, int32_t stride_bytes);
vgs_status vgs_commit_points(vgs_ctx* ctx);
/* pinned host memory for the two calls above and for vgs_get_point_labels_async (hipHostMalloc / hipHostRegister) */
vgs_status vgs_host_alloc(void** p, uint64_t bytes);
vgs_status vgs_host_free(void* p);
vgs_status vgs_host_register(void* p, uint64_t bytes);
vgs_status vgs_host_unregister(void* p);

/* ---- VGS stages, in the reference's call order (T:54-74) --------------------------------- */
vgs_status vgs_voxelize(vgs_ctx* ctx);   /* addPointsFromInputCloud + getBoundingBox/setBoundingBox + setVoxelCenters + getVoxelNum (T:54-62, VS:146-189) */
vgs_status vgs_features(vgs_ctx* ctx);   /* calcualteVoxelCloudAttributes (VS:290-369) */
vgs_status vgs_adjacency(vgs_ctx* ctx);  /* findAllVoxelAdjacency(graph_size) (VS:223-265) */
vgs_status vgs_segment(vgs_ctx* ctx);    /* segmentVoxelCloudWithGraphModel (VS:372-421) + drawColorMapofPointsinClusters' cluster filter (VS:963-1009) */
vgs_status vgs_run(vgs_ctx* ctx);        /* all stages for ctx's method (segmentationVGS T:51-76 / segmentationSVGS T:138-160) */

/* ---- SVGS ------------------------------------------------------------------------------- */
/* segmentSupervoxelCloudWithGraphModel from a caller-supplied supervoxel labelling (what
 * pcl::SupervoxelClustering::getLabeledCloud returns, SS:283): labels_dev/labels_host hold one int32 per
 * point, 0 = unassigned; max_label = getMaxLabel().  (SS:279-421)
 * Only the labels 1 .. max_label - 1 make supervoxels (SS:313); a negative label, or one of max_label or above, leaves its point
 * unassigned.  A point with a non-finite coordinate (NaN, +-inf) belongs to no supervoxel, whatever label it carries: it is left out
 * of the supervoxel table and ends with point label -1, as in VGS. */
vgs_status svgs_set_supervoxel_labels(vgs_ctx* ctx, const int32_t* labels_host, int32_t max_label);
vgs_status svgs_supervoxels(vgs_ctx* ctx);  /* createSupervoxels: VCCS-style clustering on the GPU (SS:245-331) */
vgs_status svgs_segment(vgs_ctx* ctx);      /* attributes + neighbours + local cuts + merge (SS:362-421) */
/* getLabeledCloud / getMaxLabel (SS:283-284): one label per point (0 = unassigned) */
vgs_status svgs_get_supervoxel_labels(vgs_ctx* ctx, int32_t* labels, int32_t* max_label);

/* ---- results ---------------------------------------------------------------------------- */
/* Every getter below reports the LAST run of the stages on the CURRENT cloud and parameters, whatever the context ran before: a reused
 * context returns what a fresh context returns for the same cloud and parameters.  That includes the empty frames -- no point, no finite
 * point (every point's voxel and label -1), no voxel, no used voxel, no kept segment -- after which every count, list, table and schedule
 * counter is what a fresh context gives: zeros and empty tables, never the previous cloud's numbers. */
vgs_status vgs_get_counts(vgs_ctx* ctx, int64_t* counts /* VGS_N_COUNTS */);
vgs_status vgs_get_stage_times(vgs_ctx* ctx, double* ms /* VGS_T_COUNT */);
/* Schedule diagnostics of the last local cut (no reference counterpart; tests use them to see that an input reached the
 * path it was built for).  out[0..7]: 0 rounds the lazy schedule gave up in, 1 voxels it handed over because a shell or
 * phase B overflowed its list, 2 handed over to the dense kernel (all causes), 3 sent on by the dense kernel to the
 * general kernel (a list of 2048 edges overflowed), 4 handed over by the classes above 128 neighbours, 5 voxels
 * outside every kernel's limits (result incomplete: vgs_segment reports it), 6 rows crossValidation put off, 7 voxels for which a dense
 * kernel took a phase in bands of descending weight (more edges than its list holds) */
vgs_status vgs_get_schedule_counters(vgs_ctx* ctx, int64_t* out /* 8 */);
/* The same with room to grow (n <= 16): 8 neighbourhoods above 2048 used voxels, cut by the extra-large instantiation of the general
 * kernel (the reference sizes its matrix to any n, VS:1815-1818; round 4 -- such a voxel used to end the run with VGS_E_UNSUPPORTED) */
/* round 5: 9 voxels cut by the pair-list kernel (csrc/localcut_pg.hpp), 10 entries of the pair lists built for them (csrc/pairlist.hpp),
 * 11 one-wavefront voxels handed over without a try on the strength of the scene's samples (LwParams::vote), 12 rows that found the
 * pair lists' pool exhausted */
vgs_status vgs_get_schedule_counters_ex(vgs_ctx* ctx, int64_t* out, int32_t n);
/* Screening table of the dense hand-over kernels for a parameter set (host arithmetic, no context, no GPU; for tests): a
 * pair of valid positions and normals whose squared centroid distance d2 is >= *d2_stop, or whose dot(n1, n2) lies in
 * [-1, ctab[min(63, int(d2 * *ctab_scale))]], weighs at most 1 - cut_thred and is not evaluated (csrc/localcut.hip). */
vgs_status vgs_screen_table(const vgs_params* params, float* d2_stop, float* ctab_scale, float* ctab /* 64 */);
vgs_status vgs_get_bbox(vgs_ctx* ctx, double* min3_max3);                 /* getBoundingBox (T:56) */
/* voxel table in leaf order: key 3*V, start V+1 (offsets into point_idx), point_idx N' ; any may be NULL */
vgs_status vgs_get_voxel_table(vgs_ctx* ctx, uint32_t* key, int32_t* start, int32_t* point_idx);
vgs_status vgs_get_voxel_centers(vgs_ctx* ctx, float* center3V);          /* getVoxelCenters (VS:191) */
vgs_status vgs_get_point_voxel(vgs_ctx* ctx, int32_t* voxel_of_point /* N, -1 = not in octree */);
/* per-node attributes (voxels for VGS, supervoxels for SVGS): centroid 3*V, normal 3*V, eigen 8*V, used V */
vgs_status vgs_get_attributes(vgs_ctx* ctx, float* centroid, float* normal, float* eigen8, uint8_t* used);
/* ragged lists, two-call protocol: pass idx == NULL to get offsets (n_nodes+1, int64) and the total first.
 * which: 0 adjacency (getOneVoxelAdjacency order, VS:268; every voxel, used or not, with every neighbour, as findAllVoxelAdjacency
 *        builds them VS:236-263 -- computed on request, the hot path keeps only what the cuts read), 1 connect lists after the local cut,
 *        2 after crossValidation (VS:2111), 3 after closestCheck (VS:2181) */
vgs_status vgs_get_lists(vgs_ctx* ctx, int32_t which, int64_t* offsets, int32_t* idx);
/* Element order of the connect lists (which >= 1) and of getClusterIdx.  VGS_ORDER_VOXEL_ID: members in the order of the
 * adjacency row / ascending voxel id -- what the hot path keeps (a flag per adjacency slot).  VGS_ORDER_REFERENCE: the
 * reference's own order: cutGraphSegmentation returns its vertex list in merge-history order (every merge appends the absorbed
 * segment's vertices, VS:1986-1998, 2003-2026), crossValidation filters it in place, closestCheck appends (VS:2293-2294).
 * Computed on request by replaying the scan inside every list that was found (csrc/cutorder.hip); ties as the oracle's lean
 * flavour (the reference's std::sort of both orientations of a pair leaves them unspecified).
 * Limit of VGS_ORDER_REFERENCE: rows of any length the local cut accepts (8192 stored entries), connect lists after the local cut of up
 * to 4224 nodes (the largest ball the local cut takes whole).  A cloud with a longer one gets VGS_E_UNSUPPORTED from
 * vgs_get_lists_ordered (which >= 1) and vgs_get_clusters_ordered, the message naming the list's length and the limit; the default
 * order has no such limit. */
enum { VGS_ORDER_VOXEL_ID = 0, VGS_ORDER_REFERENCE = 1 };
vgs_status vgs_get_lists_ordered(vgs_ctx* ctx, int32_t which, int32_t order, int64_t* offsets, int32_t* idx);
/* voxels_adjacency_idx_[v][0] (VS:253): the number of neighbours of every node inside graph_size, itself included; 0 for a
 * node that has no list (unused voxels, see `which` above) */
vgs_status vgs_get_adjacency_counts(vgs_ctx* ctx, int32_t* n_all /* n_nodes */);
/* The affinity matrix buildAdjacencyGraph fills for one node (VS:1796-1910; SS twin): weights[a * n + b] =
 * distanceWeight(measuringDistance(ids[a], ids[b])), ids = the node's stored adjacency row (the used neighbours when unused
 * voxels are inert, every neighbour otherwise), ids[0] = the node itself.  Two-call protocol: ids == NULL returns n (0 for a
 * node without a local graph).  Diagnostics / parity tests: the hot path never materialises this matrix. */
vgs_status vgs_get_local_weights(vgs_ctx* ctx, int32_t node_id, int32_t* n, int32_t* ids, float* weights);
vgs_status vgs_get_node_labels(vgs_ctx* ctx, int32_t* component_root /* V: smallest node id of its cluster */,
                               int32_t* kept_label /* V: index into kept clusters or -1 */);
vgs_status vgs_get_point_labels(vgs_ctx* ctx, int32_t* labels /* N host; -1 = dropped */);
/* starts the copy of the labels to `labels` (N int32, ideally pinned) on a copy stream and returns; the next run of the
 * stages writes a second label buffer, so the copy overlaps it.  vgs_wait_point_labels blocks until `labels` is complete.
 * One copy in flight per context: a second call waits for the first. */
vgs_status vgs_get_point_labels_async(vgs_ctx* ctx, int32_t* labels);
vgs_status vgs_wait_point_labels(vgs_ctx* ctx);
vgs_status vgs_get_point_labels_device(vgs_ctx* ctx, const int32_t** labels_dev /* N, valid until next run */);
/* getClusterIdx (VS:117): offsets (kept+1, int64) and point indices grouped by cluster (cluster order =
 * ascending smallest voxel id, as the reference; inside a cluster ascending voxel id then point index) */
vgs_status vgs_get_clusters(vgs_ctx* ctx, int64_t* offsets, int32_t* point_idx);
/* The same with a choice of the order inside a cluster.  VGS_ORDER_REFERENCE is the reference's own: nodes in the pre-order
 * of recursionSearch over the final connect lists with the seed appended LAST (VS:2032-2053, 2064-2080; SS:2079-2103), the
 * points of each node in ascending index (VS:981-999; SS:2109-2126) -- element for element what getClusterIdx() holds.
 * (Output formatting: the walk runs on the host over the downloaded lists.) */
vgs_status vgs_get_clusters_ordered(vgs_ctx* ctx, int32_t order, int64_t* offsets, int32_t* point_idx);
/* getClusterIdx left in HBM (round 5; csrc/clusters.hip): the lists of vgs_get_clusters (default order) as device pointers --
 * offsets_dev[kept + 1] (int64), point_idx_dev[offsets[kept]] (int32) -- made by one stable sort of the leaf order by label; valid
 * until the next run of the stages.  vgs_get_clusters[_ordered] with the default order copies exactly these to the host. */
vgs_status vgs_get_clusters_device(vgs_ctx* ctx, const int64_t** offsets_dev, const int32_t** point_idx_dev);
/* Per-segment descriptors (no reference counterpart: what a caller does next with getClusterIdx).  Row k describes exactly the points
 * whose label (vgs_get_point_labels) is k, K = counts[VGS_N_KEPT] rows; every array is K rows long and any pointer may be NULL:
 *   n_points   int64   points with label k
 *   n_nodes    int32   voxels (VGS) or supervoxels (SVGS) with label k
 *   bbox6      float   min x, y, z, max x, y, z of the points (exact: min / max of the input floats; a bound that is zero may carry
 *                      either sign when the segment holds both +0.0 and -0.0 there; the sign is not specified)
 *   centroid3  double  mean of the points
 *   cov6       double  population covariance (1/n): xx, xy, xz, yy, yz, zz
 *   evals3     double  eigenvalues of cov6, ascending, clamped to >= 0
 *   evecs9     double  [r*3+j] = component r of eigenvector j (vm_eigen33's layout): column 0 the normal, column 2 the major axis; each
 *                      column's component of largest magnitude is positive (lowest index on a tie)
 *   eigen8     float   vm_eigen_features (csrc/vgs_math.h) of the float-rounded eigenvalues, in the order of the context's method (the
 *                      eight features of vgs_get_attributes' eigen8, so node and segment features compare directly)
 * A segment of one point has zero covariance, eigenvalues and features and identity eigenvectors.  Computed on the device on the first
 * request after a run (fp64 sums about a point of the segment, a fixed summation order: bit-identical from call to call) and cached until
 * the next run.  VGS_E_STATE before the context is segmented and for a tile context (vgs_set_owned_region / vgs_set_own_point_range);
 * K = 0 writes nothing. */
vgs_status vgs_get_segment_descriptors(vgs_ctx* ctx, int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6,
                                       double* evals3, double* evecs9, float* eigen8);
/* the same table left in HBM: device pointers (any may be NULL), valid until the next run of the stages */
vgs_status vgs_get_segment_descriptors_device(vgs_ctx* ctx, const int64_t** n_points, const int32_t** n_nodes, const float** bbox6,
                                              const double** centroid3, const double** cov6, const double** evals3, const double** evecs9,
                                              const float** eigen8);
/* Per-segment moments of a tile context (the tiled driver, include/vgs_tiles.h: vgs_tiles_get_segment_descriptors builds the global table
 * from them).  After vgs_apply_tile_labels, vox_label holds GLOBAL labels 0 .. K-1 (K = kept_global).  One record per label k for which
 * this context has an own labelled point (input index in the vgs_set_own_point_range range) or an owned voxel (vgs_set_owned_region),
 * in ascending label order; every array holds up to K records and any may be NULL; *n_records is written:
 *   label      int32   k
 *   n_points   int64   own points with label k
 *   n_nodes    int32   owned voxels with label k
 *   bbox6      float   min x, y, z, max x, y, z of those own points (+inf / -inf without one)
 *   anchor3    float   the first own point of k in the order of the descriptor chunks (sorted nodes, each node's points in order); 0 without one
 *   s9         double  sum d (x, y, z) and sum d d^T (xx, xy, xz, yy, yz, zz) over the own points, d = p - anchor in fp64
 * Computed on the device every call (no cache: the driver keeps the table).  VGS_E_STATE before the context is segmented and for a
 * context that is not a tile context. */
vgs_status vgs_get_own_segment_moments(vgs_ctx* ctx, int64_t K, int64_t* n_records, int32_t* label, int64_t* n_points, int32_t* n_nodes,
                                       float* bbox6, float* anchor3, double* s9);
/* The descriptor table from moments already folded per label (K rows, the layout of vgs_get_own_segment_moments without `label`; the
 * anchor a point of the segment, s9 about it): the per-segment algebra of vgs_get_segment_descriptors -- centroid, covariance, Jacobi,
 * sign rule, features, the same device code -- on this context's GPU.  Writes the eight arrays of vgs_get_segment_descriptors (any may be
 * NULL; n_points / n_nodes / bbox6 pass through).  Uses the context's descriptor buffers: a cached table of the context itself is
 * dropped. */
vgs_status vgs_segment_descriptors_from_moments(vgs_ctx* ctx, int64_t K, const int64_t* n_points, const int32_t* n_nodes, const float* bbox6,
                                                const float* anchor3, const double* s9, int64_t* n_points_out, int32_t* n_nodes_out,
                                                float* bbox6_out, double* centroid3, double* cov6, double* evals3, double* evecs9, float* eigen8);
/* Oriented bounding boxes of the kept segments (no reference counterpart: the size of a segment along its own axes; the principal frame is
 * the PCA box of pcl::MomentOfInertiaEstimation::getOBB).  Row k describes exactly the points whose label is k, K = counts[VGS_N_KEPT]
 * rows; every array is K rows of doubles and any pointer may be NULL.  With c the centroid3 row of vgs_get_segment_descriptors, W the
 * frame ([r*3+j] = component r of axis j, evecs9's layout), d = p - c in fp64 and t_j(p) = (W[0][j] dx + W[1][j] dy) + W[2][j] dz:
 *   center3    c[r] + ((W[r][0] mid[0] + W[r][1] mid[1]) + W[r][2] mid[2]), mid = (lo + hi) / 2: the centre of the box
 *   half3      (hi - lo) / 2: the half extent along axis j
 *   frame9     W as used
 *   lo3, hi3   min and max of t_j over the points of the segment (a bound that is zero may carry either sign, as in bbox6)
 * frame selects W:
 *   VGS_BOX_PRINCIPAL  the evecs9 row of the descriptor table, byte for byte: axis 0 the normal, axis 2 the major axis
 *   VGS_BOX_UPRIGHT    axis 2 = (0, 0, 1) exactly; axes 0 and 1 the eigenvectors of the block (xx, xy; xy, yy) of cov6 -- one Jacobi
 *                      rotation in fp64 -- by ascending eigenvalue (axis 0 minor, axis 1 major; xy = 0 with xx <= yy gives the identity),
 *                      each with evecs9's sign rule and a z component of exactly 0
 * Every product and sum above is a single fp64 operation in the association written (no FMA) and min / max do not depend on the order, so
 * lo3, hi3, half3 and center3 are an exact function of the float points, c and W: bit-identical from call to call and engine to engine.  A
 * segment of one point gives lo = hi = half = 0 and center = that point.  Computed on the device on the first request after a run (the
 * descriptor table first, if it is not cached; then a second pass over the points) and cached per frame until the next run; both frames
 * may be cached at once.  frame9 is the table's own copy: vgs_segment_descriptors_from_moments does not change a cached box table.
 * VGS_E_ARG for another frame value; VGS_E_STATE before the context is segmented and for a tile context; K = 0 writes nothing. */
enum { VGS_BOX_PRINCIPAL = 0, VGS_BOX_UPRIGHT = 1 };
vgs_status vgs_get_segment_boxes(vgs_ctx* ctx, int32_t frame, double* center3, double* half3, double* frame9, double* lo3, double* hi3);
/* the same table left in HBM: device pointers (any may be NULL), valid until the next run of the stages */
vgs_status vgs_get_segment_boxes_device(vgs_ctx* ctx, int32_t frame, const double** center3, const double** half3, const double** frame9,
                                        const double** lo3, const double** hi3);
/* Box extents of a tile context (the tiled driver, include/vgs_tiles.h: vgs_tiles_get_segment_boxes builds the global table from them).
 * Inputs: K rows of the GLOBAL descriptor table -- centroid3, cov6, evecs9 (host arrays, all required for K > 0) -- and the frame.  The
 * rows are uploaded, the frames W made from them by the frame rule above (the same device code), and t_j(p) taken over this context's own
 * labelled points: exactly the points vgs_get_own_segment_moments counts in n_points (input index in the vgs_set_own_point_range range,
 * vox_label = k, global after vgs_apply_tile_labels).  One record per label with at least one such point, in ascending label order; every
 * output array holds up to K records and any may be NULL; *n_records is written:
 *   label      int32   k
 *   lo3, hi3   double  min and max of t_j over the own points of k
 * Computed on the device every call (no cache: the driver keeps the table); a cached box table of the context itself is not touched.
 * VGS_E_ARG for another frame value; VGS_E_STATE before the context is segmented and for a context that is not a tile context. */
vgs_status vgs_get_own_segment_extents(vgs_ctx* ctx, int64_t K, int32_t frame, const double* centroid3, const double* cov6, const double* evecs9,
                                       int64_t* n_records, int32_t* label, double* lo3, double* hi3);
/* The box table from extents already folded per label (K rows of lo3 / hi3 in the frame that `frame` makes from the cov6 / evecs9 rows;
 * centroid3 the row's c): half3, center3 and frame9 of vgs_get_segment_boxes by the same device code, on this context's GPU -- the
 * arithmetic is not the host compiler's.  Every input is required for K > 0; any output may be NULL.  A row that no point reaches (a label
 * without a labelled point anywhere, n_points = 0 in the tiled descriptor table) is passed as lo = hi = 0 and comes back as half = 0,
 * center3 = its centroid3 (c plus a zero), frame9 as computed.  Uses scratch of its own: a cached box table of the context itself is not
 * touched.  VGS_E_ARG for another frame value. */
vgs_status vgs_segment_boxes_from_extents(vgs_ctx* ctx, int64_t K, int32_t frame, const double* centroid3, const double* cov6,
                                          const double* evecs9, const double* lo3, const double* hi3, double* center3, double* half3,
                                          double* frame9);
/* Segment adjacency graph (no reference counterpart: which kept segments touch, and how strongly the local cut's weight links them).
 *   A node is a voxel (VGS) or a supervoxel (SVGS).  Only used nodes with a kept label >= 0 take part; unused voxels and the nodes of
 *   clusters dropped by the size filter are ignored.
 *   An edge is an unordered pair of kept labels a < b with at least one node pair {u, v} such that u has label a, v has label b, and v is
 *   in u's stored adjacency row (the adjacency stage's own predicate: float d2 < graph_size^2 between centres or centroids).
 *   Edges are listed in ascending (a, b) order; E = their number.  Per edge (every array E rows, any pointer may be NULL):
 *     seg_ab    int32 x2  a, b
 *     n_pairs   int64     node pairs {u, v} as above, each counted once
 *     n_finite  int64     those pairs whose weight is not NaN
 *     nodes_ab  int32 x2  the nodes of a with at least one such neighbour in b, and the nodes of b with one in a
 *     w_sum     double    sum of the non-NaN weights w(u, v) = vm_pair_weight(node[min(u, v)], node[max(u, v)], W) -- the lower node id first,
 *                         exactly the entry vgs_get_local_weights reports for that ordered pair -- summed in fp64 in a fixed order
 *     w_min     float     min of the non-NaN weights (NaN when n_finite == 0)
 *     w_max     float     max of the non-NaN weights (NaN when n_finite == 0)
 * n_edges is required and always written; a call with every array NULL is the size query.  Computed on the device on the first request
 * after a run (no atomics, fixed summation shapes: bit-identical from call to call and engine to engine) and cached until the next run.
 * VGS_E_STATE before the context is segmented and for a tile context; K <= 1 kept segments gives E = 0. */
vgs_status vgs_get_segment_graph(vgs_ctx* ctx, int64_t* n_edges, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                 double* w_sum, float* w_min, float* w_max);
/* the same table left in HBM: device pointers (any may be NULL), valid until the next run of the stages */
vgs_status vgs_get_segment_graph_device(vgs_ctx* ctx, int64_t* n_edges, const int32_t** seg_ab, const int64_t** n_pairs, const int64_t** n_finite,
                                        const int32_t** nodes_ab, const double** w_sum, const float** w_min, const float** w_max);
/* The segment graph of a tile context (the tiled driver, include/vgs_tiles.h: vgs_tiles_get_segment_graph folds the ranks' tables).
 * After vgs_apply_tile_labels an owned voxel holds its GLOBAL label, but a voxel of the halo holds one only if its local component has an
 * owned voxel.  vgs_set_halo_labels brings the rest: n (voxel code, global label) pairs taken from the OTHER ranks' boundary records
 * (label -1 = dropped; several pairs of one code must agree).  Every code this context holds without owning it gets that label in a table
 * of the graph's own; vox_label, the point labels and the descriptors are not touched.  A voxel of another rank without a pair stays
 * "unknown".  The table holds until the next run of the stages or the next vgs_apply_tile_labels; without a call every voxel of another
 * rank is unknown. */
vgs_status vgs_set_halo_labels(vgs_ctx* ctx, const uint64_t* code, const int32_t* label, int64_t n);
/* This context's share of the graph over the global labels 0 .. K-1 (K = kept_global): the table of vgs_get_segment_graph -- fields, edge
 * order, NaN rules -- restricted to what this rank counts: the node pairs {u, v} whose lower-id endpoint u it OWNS (whoever owns v), and
 * in nodes_ab the nodes it owns.  Effective labels: vox_label for an owned used voxel, the halo table for any other.  Summed over the
 * ranks (counts add, w_sum adds, w_min / w_max over the ranks with n_finite > 0) the tables give the graph of the whole scene, each
 * contribution from exactly one rank.  VGS_E_UNSUPPORTED, with the count in the message, if the row of an owned voxel holds a used voxel
 * of another rank whose label is unknown; VGS_E_ARG if a label is not below K.  n_edges is required; every array holds up to *n_edges
 * rows and any may be NULL.  Two-call protocol (as vgs_get_boundary_roots): a call with every array NULL computes the table on the
 * device and returns its size; a call with arrays copies that table if K is the same and neither the labels nor the halo table changed
 * since, and computes it otherwise.  Nothing else is cached: the driver keeps the folded table.  VGS_E_STATE before the context is
 * segmented and for a context that is not a tile context. */
vgs_status vgs_get_own_segment_graph(vgs_ctx* ctx, int64_t K, int64_t* n_edges, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite,
                                     int32_t* nodes_ab, double* w_sum, float* w_min, float* w_max);
/* Per-segment statistics of point attributes the CALLER supplies (no reference counterpart: what a user of a segmentation does first with
 * intensity, colour, time, class scores or a ground-truth class).  Row k covers exactly the points whose label (vgs_get_point_labels) is k,
 * K = counts[VGS_N_KEPT] rows; points with label -1 (outside the octree, dropped clusters) contribute nothing.  Any output pointer may be
 * NULL; K = 0 writes nothing.  Computed on the device on every call, nothing cached (the input is the caller's).
 * Input: n must equal counts[VGS_N_POINTS]; row i belongs to input point i; channel c of point i is the float at byte
 * i * stride_bytes + 4 * c; stride_bytes >= 4 * n_channels and a multiple of 4; 1 <= n_channels <= 64.  VGS_E_ARG otherwise (the message
 * names the argument).  The host variant uploads once into a buffer of the context; the device variant reads field_dev (HBM, the context's
 * device; complete before the call) in place.
 * Outputs, each K x n_channels, row-major.  A value is valid when it is finite: NaN and +-inf are skipped.
 *   n_valid  int64   valid values
 *   anchor   double  the shift of the sums.  One point p per segment, the same for every channel -- the segment's first point in the order of
 *                    the descriptor chunks (csrc/segdesc.hip); which one is not specified, it does not change from call to call --
 *                    anchor[k, c] = (double)field[p, c] if that value is valid, 0.0 otherwise.  Reported so that a reader can restate the
 *                    arithmetic: it keeps a field of large offset and small spread (a GPS time) from losing its variance
 *   mean     double  anchor + S1 / n            with d = (double)x - anchor per valid x, S1 = sum d, S2 = sum d * d, n = n_valid
 *   var      double  max(0, S2 / n - (S1 / n) * (S1 / n))   population variance
 *   vmin, vmax  float  min and max of the valid values (a zero may carry either sign, as in bbox6)
 * n = 0: mean, var, vmin, vmax are NaN and anchor is 0.  Every product, quotient and sum above is one fp64 operation in the association
 * written (no FMA).  The sums have a fixed shape (csrc/segdesc.hip's rule: the point of a lane depends on (chunk, lane, step) only, fixed
 * butterfly, waves in index order, partials by lane stride then butterfly) and there are no float atomics: bit-identical from call to call
 * and from engine to engine for the same cloud and parameters.
 * VGS_E_STATE before the context is segmented and for a tile context.  No side effects: the labels and every cached table stay as they are. */
vgs_status vgs_segment_field_stats(vgs_ctx* ctx, const float* field_host, int64_t n, int32_t n_channels, int64_t stride_bytes,
                                   int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax);
vgs_status vgs_segment_field_stats_device(vgs_ctx* ctx, const float* field_dev, int64_t n, int32_t n_channels, int64_t stride_bytes,
                                          int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax);
/* Per-segment histogram of a per-point class (segment voting; the contingency table of segments against ground-truth classes).  Rows, n,
 * NULL outputs, K = 0, state and side effects as above; cls holds one int32 per input point; 1 <= n_classes <= 1024 (VGS_E_ARG).
 * VGS_E_UNSUPPORTED, with the numbers in the message, if K * n_classes exceeds 2^27.
 *   hist            int64  K x n_classes: hist[k, j] = points of segment k with class j, 0 <= j < n_classes
 *   n_outside       int64  K: points of segment k whose class is negative or >= n_classes
 *   majority        int32  K: the lowest j with the largest hist[k, j]; -1 when every count is 0
 *   majority_count  int64  K: that count (0 with majority -1)
 * Integer counts: every summation order gives the same bits.  Counted per chunk in LDS, then added to the table with integer atomics. */
vgs_status vgs_segment_class_histogram(vgs_ctx* ctx, const int32_t* cls_host, int64_t n, int32_t n_classes, int64_t* hist, int64_t* n_outside,
                                       int32_t* majority, int64_t* majority_count);
vgs_status vgs_segment_class_histogram_device(vgs_ctx* ctx, const int32_t* cls_dev, int64_t n, int32_t n_classes, int64_t* hist,
                                              int64_t* n_outside, int32_t* majority, int64_t* majority_count);
/* Score the segmentation against a labelling of the same points that the CALLER supplies (no reference counterpart in code: the matching of
 * segments to reference segments by which the VGS / SVGS paper counts precision, recall and F1).  The sparse contingency
 * table between the point labels and `ref`, and the two match tables read off it.  No label is written, no other cloud is involved.
 *   ref   one int32 per input point, row i belongs to input point i; n must equal counts[VGS_N_POINTS].  Point i is ANNOTATED iff
 *         ref[i] >= 0; any non-negative int32 is a reference id, ids need not be dense.  A point with ref[i] < 0 takes no part in anything
 *         below; it is only counted, in summary[1].
 *   L[i]  the point label of vgs_get_point_labels: 0 .. K-1 (K = counts[VGS_N_KEPT]), or -1 for a dropped point.
 * Cells: one per distinct pair (L, g) over the annotated points, in ascending (L, g) order, the L = -1 row first; n_cells rows:
 *   cell_seg  int32  L            cell_ref  int32  g            cell_n  int64  annotated points with that pair
 * Reference table: n_refs = G rows, one per distinct id, ascending:
 *   ref_id        int32   the id
 *   ref_points    int64   annotated points with that id
 *   ref_dropped   int64   those with L = -1
 *   ref_best_seg  int32   the kept segment L >= 0 with the largest cell_n, the lowest label on a tie; -1 when every point of the id is dropped
 *   ref_best_n    int64   that cell_n (0 with -1)
 *   ref_best_iou  double  (double)n / (double)(seg_annotated[ref_best_seg] + ref_points - n), n = ref_best_n: one fp64 division; 0.0 with -1
 * Segment table: K rows:
 *   seg_annotated int64   annotated points with label k
 *   seg_refs      int32   distinct ids among them
 *   seg_best_ref  int32   the id with the largest cell_n, the lowest id on a tie; -1 without an annotated point
 *   seg_best_n    int64   that cell_n (0 with -1)
 *   seg_best_iou  double  (double)n / (double)(seg_annotated + ref_points[seg_best_ref] - n), n = seg_best_n; 0.0 with -1
 * summary, int64[12], C(a, 2) = a (a - 1) / 2:
 *   0 annotated points    1 unannotated points    2 annotated points with L = -1    3 G    4 n_cells    5 segments with seg_annotated > 0
 *   6 sum over k of seg_best_n    7 sum over the ids of ref_best_n    8 sum of C(cell_n, 2) over all cells
 *   9 sum of C(a, 2) over the rows, a = the annotated points of the row, the L = -1 row counted as one class    10 sum of C(ref_points, 2)
 *   11 0, reserved
 * Everything is an integer or one division of two integers converted to double: bit-identical from call to call and from engine to engine
 * (the integer atomics of csrc/segcompare.hip add in any order).
 * vgs_compare_labels computes all three tables on the device into buffers of the context and returns their sizes and the summary (each
 * of n_cells, n_refs, summary may be NULL); the host variant uploads ref once, the device variant reads ref_dev (HBM, the context's device;
 * complete before the call) in place.  A table without rows is empty and the counts say why: a cloud without points gives zero sizes and a
 * zero summary; without an annotated point n_cells = G = 0, the K segment rows read 0, 0, -1, 0, 0.0 and only summary[1] counts; with
 * K = 0 every annotated point is dropped, so the cells are the L = -1 row, every ref_best_seg is -1 and the segment table is empty.  Never
 * the previous comparison's numbers.
 * vgs_get_label_comparison copies the tables of the last compare (any pointer may be NULL; sizes as that compare returned them, K rows for
 * the segment table); vgs_get_label_comparison_device returns them as device pointers (NULL for a table without rows), valid until the next
 * compare or the next run of the stages.  Both answer VGS_E_STATE when there is no comparison since the last run of the stages or the last
 * vgs_set_points.
 * VGS_E_ARG, the message naming the argument, for n != counts[VGS_N_POINTS] and for a NULL ref with n > 0; VGS_E_STATE before the context
 * is segmented and for a tile context (a tile holds only part of its segments: the tiled driver scores over all ranks with
 * vgs_tiles_compare_labels, include/vgs_tiles.h, from the two calls further down).  No side effects: labels, descriptors, boxes, graph and
 * every other cached table stay as they are. */
vgs_status vgs_compare_labels(vgs_ctx* ctx, const int32_t* ref_host, int64_t n, int64_t* n_cells, int64_t* n_refs, int64_t* summary /* 12 */);
vgs_status vgs_compare_labels_device(vgs_ctx* ctx, const int32_t* ref_dev, int64_t n, int64_t* n_cells, int64_t* n_refs, int64_t* summary /* 12 */);
vgs_status vgs_get_label_comparison(vgs_ctx* ctx, int32_t* cell_seg, int32_t* cell_ref, int64_t* cell_n, int32_t* ref_id, int64_t* ref_points,
                                    int64_t* ref_dropped, int32_t* ref_best_seg, int64_t* ref_best_n, double* ref_best_iou, int64_t* seg_annotated,
                                    int32_t* seg_refs, int32_t* seg_best_ref, int64_t* seg_best_n, double* seg_best_iou);
vgs_status vgs_get_label_comparison_device(vgs_ctx* ctx, const int32_t** cell_seg, const int32_t** cell_ref, const int64_t** cell_n,
                                           const int32_t** ref_id, const int64_t** ref_points, const int64_t** ref_dropped,
                                           const int32_t** ref_best_seg, const int64_t** ref_best_n, const double** ref_best_iou,
                                           const int64_t** seg_annotated, const int32_t** seg_refs, const int32_t** seg_best_ref,
                                           const int64_t** seg_best_n, const double** seg_best_iou);
/* Attribute moments of a tile context (the tiled driver, include/vgs_tiles.h: vgs_tiles_segment_field_stats builds the global table from
 * them).  No attribute travels between ranks: a rank hands in one row per point of its OWN load, in the order it gave them to the driver --
 * own point i is cloud point own_first + i of vgs_set_own_point_range -- so n_own must equal that range's length; channels, stride_bytes and
 * NULL rules as vgs_segment_field_stats.  Over this context's own labelled points (input index in the own range, vox_label = k, global
 * after vgs_apply_tile_labels: the points vgs_get_own_segment_moments counts in n_points) one record per label 0 .. K-1 with at least one
 * such point, in ascending label order -- the label set of vgs_get_own_segment_extents.  *n_records is written; every array holds up to K
 * records (x n_channels) and any may be NULL:
 *   label      int32   k
 *   n_valid    int64   valid (finite) values of the channel among the own points of k; may be 0
 *   anchor     double  the value of k's first own point in the order of the descriptor chunks, 0.0 where it is not valid
 *   s1, s2     double  sum d and sum d * d over the valid values, d = (double)x - anchor, summed in the fixed shape of vgs_segment_field_stats
 *   vmin, vmax float   min and max of the valid values; +inf / -inf for n_valid = 0 (anchor, s1 and s2 are 0 then)
 * Computed on the device on every call; nothing is cached and no other table is touched.  The device variant reads field_dev in place.
 * VGS_E_STATE before the context is segmented and for a context that is not a tile context; VGS_E_ARG as vgs_segment_field_stats. */
vgs_status vgs_get_own_segment_field_moments(vgs_ctx* ctx, int64_t K, const float* field_host, int64_t n_own, int32_t n_channels,
                                             int64_t stride_bytes, int64_t* n_records, int32_t* label, int64_t* n_valid, double* anchor,
                                             double* s1, double* s2, float* vmin, float* vmax);
vgs_status vgs_get_own_segment_field_moments_device(vgs_ctx* ctx, int64_t K, const float* field_dev, int64_t n_own, int32_t n_channels,
                                                    int64_t stride_bytes, int64_t* n_records, int32_t* label, int64_t* n_valid, double* anchor,
                                                    double* s1, double* s2, float* vmin, float* vmax);
/* The field table from moments already folded per (label, channel) about `anchor` (K x n_channels each, all required for K > 0; an entry no
 * valid value reaches: n_valid 0, sums 0, vmin +inf, vmax -inf): mean, var, vmin and vmax of vgs_segment_field_stats by the same device
 * code, on this context's GPU -- the finishing kernel of vgs_segment_field_stats runs over one partial per entry, so the arithmetic is
 * not the host compiler's.  NaN rows for n_valid = 0.  Any output may be NULL.  Works on any context; nothing cached is touched. */
vgs_status vgs_segment_field_stats_from_moments(vgs_ctx* ctx, int64_t K, int32_t n_channels, const int64_t* n_valid, const double* anchor,
                                                const double* s1, const double* s2, const float* vmin, const float* vmax, double* mean,
                                                double* var, float* vmin_out, float* vmax_out);
/* Class counts of a tile context: rows, n_own, state and label set as vgs_get_own_segment_field_moments; cls holds one int32 per own point;
 * the limits of vgs_segment_class_histogram (1 .. 1024 classes, K * n_classes <= 2^27).  Compact rows: label (int32), hist (int64, n_classes
 * per record), n_outside (int64) over the own points of each label; any may be NULL. */
vgs_status vgs_get_own_segment_class_counts(vgs_ctx* ctx, int64_t K, const int32_t* cls_host, int64_t n_own, int32_t n_classes,
                                            int64_t* n_records, int32_t* label, int64_t* hist, int64_t* n_outside);
vgs_status vgs_get_own_segment_class_counts_device(vgs_ctx* ctx, int64_t K, const int32_t* cls_dev, int64_t n_own, int32_t n_classes,
                                                   int64_t* n_records, int32_t* label, int64_t* hist, int64_t* n_outside);
/* Contingency cells of a tile context (the tiled driver: vgs_tiles_compare_labels builds the global comparison from them).  No label and no
 * reference id travels between ranks: a rank hands in one int32 per point of its OWN load, in the order it gave them to the driver -- ref[i]
 * belongs to cloud point own_first + i of vgs_set_own_point_range, so n_own must equal that range's length -- and its label is the point
 * label of that point, global after vgs_apply_tile_labels (-1 .. K-1).  The result is the cells of vgs_compare_labels over the own
 * annotated points only: one per distinct pair (L, g), ascending (L, g), the L = -1 row first, with the number of own points of the pair;
 * *n_cells of them and *n_unannotated own points with ref < 0 (either may be NULL).  They stay in the context until
 * vgs_get_own_label_cells copies them (arrays of *n_cells rows, any may be NULL) or until the next comparison of any kind, the next run of
 * the stages or new labels; VGS_E_STATE from the getter then.  The call discards an earlier comparison of the context (the buffers are the
 * same) and touches no other table.  The device variant reads ref_dev in place.
 * VGS_E_STATE before the context is segmented and for a context that is not a tile context; VGS_E_ARG for a wrong n_own, a NULL ref with
 * n_own > 0, K outside 0 .. 2^31 - 1 and an own point whose label is not below K. */
vgs_status vgs_own_label_cells(vgs_ctx* ctx, int64_t K, const int32_t* ref_host, int64_t n_own, int64_t* n_cells, int64_t* n_unannotated);
vgs_status vgs_own_label_cells_device(vgs_ctx* ctx, int64_t K, const int32_t* ref_dev, int64_t n_own, int64_t* n_cells, int64_t* n_unannotated);
vgs_status vgs_get_own_label_cells(vgs_ctx* ctx, int32_t* cell_seg, int32_t* cell_ref, int64_t* cell_n);
/* The comparison tables from a list of cells instead of points: n_in host cells (seg, ref, n) in ANY order and with ANY number of entries
 * for one pair -- the lists of several ranks one after another.  On this context's GPU: the merged cells (one per distinct pair, ascending
 * (seg, ref), cell_n the int64 sum of the pair's entries), then the reference table, the segment table of K rows and the summary of
 * vgs_compare_labels by the same kernels; summary[0] = the sum of all counts, summary[1] = n_unannotated as passed in, summary[8] over the
 * merged cells.  Integer adds only, so the order of the input does not matter.  The tables become the context's last comparison:
 * vgs_get_label_comparison[_device] hand them out until the next compare, the next run of the stages or vgs_set_points.  n_cells, n_refs
 * and summary may be NULL.  n_in = 0 gives the tables of "no annotated point".  Works on any segmented context, tile or not; K is the
 * caller's (kept_global in the driver), not the context's own count.
 * VGS_E_ARG, the message naming the first offending input with its values, for a seg outside -1 .. K-1, a negative ref or a count below 1
 * (found on the device in one pass, before anything is built), and for K outside 0 .. 2^31 - 1, a negative n_in or n_unannotated and a NULL
 * array with n_in > 0.  VGS_E_UNSUPPORTED, with the numbers, for n_in >= 2^31 and for counts that add up to more than 2^32 (so that
 * C(total, 2) fits int64).  VGS_E_STATE before the context is segmented.  After an error the context holds no comparison. */
vgs_status vgs_label_comparison_from_cells(vgs_ctx* ctx, int64_t K, int64_t n_in, const int32_t* cell_seg, const int32_t* cell_ref,
                                           const int64_t* cell_n, int64_t n_unannotated, int64_t* n_cells, int64_t* n_refs,
                                           int64_t* summary /* 12 */);

/* Describe and score ANY per-point labelling of the context's cloud (no reference counterpart).  The per-segment tables above describe the
 * node labels -- a labelling that is constant on a voxel or supervoxel; these entry points take one int32 per input point that the CALLER
 * supplies: the refined labels (vgs_get_refined_labels), ground-truth instances, anything made from the engine's output.
 *   labels  n int32 in input order; n must equal counts[VGS_N_POINTS].  Label l belongs to row l for 0 <= l < K; l < 0 means no segment.
 *           A label >= K is VGS_E_ARG, the message naming the first offending index and its value (found on the device in one pass,
 *           before anything is built).  0 <= K <= 2^31 - 1; K is the caller's, not counts[VGS_N_KEPT].
 * The host variants upload once into a buffer of the context; the _device variants read HBM (the context's device; complete before the
 * call) in place.  Outputs are caller-allocated host arrays of K rows and any pointer may be NULL; K = 0 writes nothing.
 * vgs_point_label_descriptors: the fields of vgs_get_segment_descriptors.  Row k covers the points i with labels[i] == k that are in the
 * octree -- the finite points, for SVGS those of a supervoxel -- and *n_skipped (may be NULL) counts the labelled points that are not: they
 * contribute to no row.  n_nodes is the number of distinct nodes (voxels / supervoxels) among the row's points.  A label no point carries:
 * n_points 0, n_nodes 0, bbox6 = (+inf, +inf, +inf, -inf, -inf, -inf), zero centroid, covariance and eigenvalues, identity eigenvectors,
 * the eigen features of zeros.
 * vgs_point_label_boxes: the fields and the frame rule of vgs_get_segment_boxes, the frames made from the descriptor rows of THIS
 * labelling (computed first, by the call); a label no point carries gives lo = hi = half = 0 and center3 = its centroid3.
 * Both run the device code of the node tables -- the same chunk sums, folds, per-segment algebra and frame rule -- over the points sorted
 * by label (csrc/pointseg.hip): no float atomics, every sum of a fixed shape, bit-identical from call to call and engine to engine; and
 * handed the context's own point labels with K = counts[VGS_N_KEPT] they return the tables of vgs_get_segment_descriptors and
 * vgs_get_segment_boxes byte for byte.  Computed on every call, nothing cached; scratch of their own, about 16 bytes per finite point plus
 * the sort's storage.  No side effects: labels, refined labels, every cached table and the last comparison stay as they are.
 * vgs_compare_point_labels: the tables of vgs_compare_labels with L[i] = seg_labels[i] if it lies in 0 .. K-1 and -1 if it is negative.
 * Purely index-wise: a non-finite point takes part with the label the caller gave it.  Like vgs_compare_labels it makes its tables the
 * context's last comparison: vgs_get_label_comparison[_device] serve them, K rows in the segment table.
 * VGS_E_STATE before the context is segmented and for a tile context; VGS_E_ARG for a wrong n, a NULL labelling with n > 0, K out of
 * range, a label >= K and a bad frame. */
vgs_status vgs_point_label_descriptors(vgs_ctx* ctx, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_skipped, int64_t* n_points,
                                       int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3, double* evecs9,
                                       float* eigen8);
vgs_status vgs_point_label_descriptors_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_skipped,
                                              int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3,
                                              double* evecs9, float* eigen8);
vgs_status vgs_point_label_boxes(vgs_ctx* ctx, const int32_t* labels_host, int64_t n, int64_t K, int32_t frame, double* center3, double* half3,
                                 double* frame9, double* lo3, double* hi3);
vgs_status vgs_point_label_boxes_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t n, int64_t K, int32_t frame, double* center3,
                                        double* half3, double* frame9, double* lo3, double* hi3);
vgs_status vgs_compare_point_labels(vgs_ctx* ctx, const int32_t* seg_labels_host, int64_t K, const int32_t* ref_host, int64_t n, int64_t* n_cells,
                                    int64_t* n_refs, int64_t* summary /* 12 */);
vgs_status vgs_compare_point_labels_device(vgs_ctx* ctx, const int32_t* seg_labels_dev, int64_t K, const int32_t* ref_dev, int64_t n,
                                           int64_t* n_cells, int64_t* n_refs, int64_t* summary /* 12 */);
/* Field statistics and class histogram of ANY per-point labelling: the two attribute tables of vgs_segment_field_stats and
 * vgs_segment_class_histogram with K rows of the caller's labelling instead of the node labels -- mean intensity or colour, or the
 * majority class, of the refined segments, which the node pass cannot give (a boundary voxel may hold two or three labels).
 *   labels  the rules of vgs_point_label_descriptors: n int32 in input order, n == counts[VGS_N_POINTS]; label l is row l for 0 <= l < K,
 *           a negative label no row; a label >= K is VGS_E_ARG, the message naming the first offending index and its value (found on the
 *           device before anything is built); 0 <= K <= 2^31 - 1, K the caller's.
 *   field, n_channels, stride_bytes, cls, n_classes   exactly as vgs_segment_field_stats / vgs_segment_class_histogram: 1 .. 64 channels,
 *           the stride a multiple of 4 and at least 4 * n_channels, 1 .. 1024 classes; a finite value is valid, NaN and +-inf are skipped.
 * The host variants take BOTH arrays on the host and upload each once into buffers of the context; the _device variants read both in place
 * in HBM (the context's device; complete before the call).
 * Row k covers the points i with labels[i] == k that are in the octree -- the finite points, for SVGS those of a supervoxel: the set
 * vgs_point_label_descriptors counts in n_points.  *n_skipped (may be NULL) counts the labelled points that are not.  So n_valid[k, c] <=
 * n_points[k], and hist[k, :].sum() + n_outside[k] == n_points[k] of vgs_point_label_descriptors for the same labelling.
 * Field outputs, each K x n_channels, the definitions of vgs_segment_field_stats: n_valid; anchor[k, c] = the value of the label's first
 * point in the sorted order of csrc/pointseg.hip (octree positions sorted by label, positions ascending inside a label), 0.0 where that
 * value is not finite; mean = anchor + S1 / n, var = max(0, S2 / n - (S1 / n) * (S1 / n)), each one fp64 operation (no FMA); vmin, vmax
 * float.  A label no octree point carries: n_valid 0, anchor 0, mean, var, vmin and vmax NaN.
 * Histogram outputs, the definitions of vgs_segment_class_histogram: hist K x n_classes; n_outside, majority (the lowest class with the
 * largest count), majority_count K rows; majority -1 with count 0 for a row without counts, a label no point carries included.
 * VGS_E_UNSUPPORTED, with the numbers in the message, if K * n_channels or K * n_classes exceeds 2^27.  K = 0 writes nothing and returns
 * VGS_OK, but still validates and still counts *n_skipped.  Any output pointer may be NULL.
 * Two guarantees (csrc/pointfield.hip):
 *   1. bit-identical from call to call and from engine to engine: no float atomics, every sum of a fixed shape (the rule of
 *      vgs_segment_field_stats over the points sorted by label; the histogram adds integers);
 *   2. handed the context's own vgs_get_point_labels with K = counts[VGS_N_KEPT], the two calls return vgs_segment_field_stats and
 *      vgs_segment_class_histogram byte for byte, anchor included (the same device code over the same point sequence).
 * VGS_E_STATE before the context is segmented, and on a tile context: a rank holds only part of the cloud, and the tables over all ranks are
 * vgs_tiles_point_label_field_stats and vgs_tiles_point_label_class_histogram of the tiled driver (include/vgs_tiles.h), built from
 * vgs_own_point_label_field_moments and vgs_own_point_label_class_counts below.  VGS_E_ARG for a
 * wrong n, a NULL array with n > 0, bad channels, stride, classes or K, and a label >= K.  Computed on every call, nothing cached; no side
 * effects: labels, refined labels, every cached table and the context's last comparison stay as they are. */
vgs_status vgs_point_label_field_stats(vgs_ctx* ctx, const int32_t* labels_host, int64_t K, const float* field_host, int64_t n,
                                       int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor,
                                       double* mean, double* var, float* vmin, float* vmax);
vgs_status vgs_point_label_field_stats_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t K, const float* field_dev, int64_t n,
                                              int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor,
                                              double* mean, double* var, float* vmin, float* vmax);
vgs_status vgs_point_label_class_histogram(vgs_ctx* ctx, const int32_t* labels_host, int64_t K, const int32_t* cls_host, int64_t n,
                                           int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority,
                                           int64_t* majority_count);
vgs_status vgs_point_label_class_histogram_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t K, const int32_t* cls_dev, int64_t n,
                                                  int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority,
                                                  int64_t* majority_count);
/* Descriptors, boxes and scores of a point labelling for a tile context (the tiled driver, include/vgs_tiles.h: vgs_tiles_point_label_descriptors, _boxes and
 * vgs_tiles_compare_point_labels build the global tables from what these leave).  Tile contexts only: VGS_E_STATE before the context is
 * segmented and on a context that is not a tile context (the three entry points above keep refusing a tile context).  In all of them
 * `labels` holds one int32 per point of the rank's OWN load: labels[i] belongs to cloud point own_first + i of vgs_set_own_point_range and
 * n_own must equal that range's length.  Label l belongs to row l for 0 <= l < K, a negative label to no row; a label >= K is VGS_E_ARG,
 * the message naming the first offending own index and its value.  0 <= K <= 2^31 - 1.
 *
 * vgs_own_point_label_moments: one moment record per label with at least one own finite point, in ascending label order, with the fields of
 * vgs_get_own_segment_moments -- n_points the own finite points of the label, bbox6 their exact box, anchor3 the label's first own point
 * in the sorted order (positions ascending), s9 the fp64 sums about it -- the pipeline of vgs_point_label_descriptors restricted to the
 * own points.  *n_skipped counts the own points with a label >= 0 that lie outside the octree (not finite).
 *   n_nodes and the pair records.  A voxel of the shared grid can hold points that two or four ranks loaded.  A voxel is SHARED on a
 *   rank when its run of points in that context holds at least one own and at least one other point.  The first point of a voxel inside a
 *   label's run is counted into the record's n_nodes when the voxel is not shared; in a shared voxel it is NOT counted but written as a
 *   pair record (voxel code, label) of 16 bytes, in sorted order (label ascending, position ascending).  The driver counts the distinct
 *   pairs over all ranks and adds them to the folded n_nodes.  With points loaded by region (no point outside its rank's region) every
 *   rank that loaded a point of a straddling voxel sees the other ranks' points of it -- they lie within one voxel_size per axis, inside
 *   the halo of 2 graph_size + voxel_size -- so all of them classify it as shared and it is counted exactly once.  With points OUTSIDE a
 *   rank's region a straddling voxel may be counted twice in n_nodes; every other field stays exact.
 * The records stay in the context until the next call, a run of the stages or new labels; vgs_get_own_point_label_moments copies them out
 * (*n_records rows and *n_pairs pairs; any pointer may be NULL).  Bit-identical from call to call: no float atomics, no arrival order.
 *
 * vgs_get_own_point_label_extents: the contract of vgs_get_own_segment_extents over the own points of the caller's labelling.
 *
 * vgs_own_point_label_cells: the contract of vgs_own_label_cells with L[i] = seg_labels[i] (any negative label is the dropped row)
 * instead of the voxel label of own point i; purely index-wise, so a non-finite own point takes part.  vgs_get_own_label_cells serves the
 * cells. */
vgs_status vgs_own_point_label_moments(vgs_ctx* ctx, int64_t K, const int32_t* labels_host, int64_t n_own, int64_t* n_records, int64_t* n_pairs,
                                       int64_t* n_skipped);
vgs_status vgs_own_point_label_moments_device(vgs_ctx* ctx, int64_t K, const int32_t* labels_dev, int64_t n_own, int64_t* n_records,
                                              int64_t* n_pairs, int64_t* n_skipped);
vgs_status vgs_get_own_point_label_moments(vgs_ctx* ctx, int32_t* label, int64_t* n_points, int32_t* n_nodes, float* bbox6, float* anchor3,
                                           double* s9, uint64_t* pair_code, int32_t* pair_label);
vgs_status vgs_get_own_point_label_extents(vgs_ctx* ctx, int64_t K, int32_t frame, const int32_t* labels_host, int64_t n_own,
                                           const double* centroid3, const double* cov6, const double* evecs9, int64_t* n_records, int32_t* label,
                                           double* lo3, double* hi3);
vgs_status vgs_get_own_point_label_extents_device(vgs_ctx* ctx, int64_t K, int32_t frame, const int32_t* labels_dev, int64_t n_own,
                                                  const double* centroid3, const double* cov6, const double* evecs9, int64_t* n_records,
                                                  int32_t* label, double* lo3, double* hi3);
vgs_status vgs_own_point_label_cells(vgs_ctx* ctx, int64_t K, const int32_t* seg_labels_host, const int32_t* ref_host, int64_t n_own,
                                     int64_t* n_cells, int64_t* n_unannotated);
vgs_status vgs_own_point_label_cells_device(vgs_ctx* ctx, int64_t K, const int32_t* seg_labels_dev, const int32_t* ref_dev, int64_t n_own,
                                            int64_t* n_cells, int64_t* n_unannotated);
/* Attribute moments and class counts of a point labelling for a tile context (the tiled driver: vgs_tiles_point_label_field_stats and
 * vgs_tiles_point_label_class_histogram build the global tables from them).  Tile contexts only: VGS_E_STATE before the context is segmented
 * and on a context that is not a tile context (vgs_point_label_field_stats and vgs_point_label_class_histogram keep refusing a tile
 * context).  labels, field and cls hold one row per point of the rank's OWN load: row i belongs to cloud point own_first + i of
 * vgs_set_own_point_range and n_own must equal that range's length.  The label rules are those of vgs_own_point_label_moments: label l is
 * row l for 0 <= l < K, a negative label no row, a label >= K is VGS_E_ARG, the message naming the first offending own index and its value;
 * 0 <= K <= 2^31 - 1.  Channels, stride_bytes and classes as vgs_point_label_field_stats / vgs_point_label_class_histogram, the limit of
 * 2^27 entries (VGS_E_UNSUPPORTED) included.  The host variants take both arrays on the host, the _device variants read both in place.
 * One compact record per label with at least one own point in the octree, in ascending label order; *n_records of them, every array holds
 * up to min(K, n_own) records.  The record fields are exactly those of vgs_get_own_segment_field_moments and
 * vgs_get_own_segment_class_counts: anchor[k, c] = the value of the label's first own point in the sorted order of csrc/pointseg.hip
 * (pos_sorted[seg_start[k]] of the own points), 0.0 where it is not finite; s1, s2 the sums about it over the finite values in the fixed
 * shape of vgs_point_label_field_stats; vmin / vmax +inf / -inf for n_valid = 0.  *n_skipped counts the own points with a label >= 0 that
 * lie outside the octree.  Any output pointer may be NULL.  One sort per call whatever the channel count (csrc/pointfield.hip: the kernel
 * bodies of the single-context tables with own-row indexing); bit-identical from call to call.  Nothing is cached; no other table, no
 * labels, no own records of vgs_own_point_label_moments and no last comparison are touched. */
vgs_status vgs_own_point_label_field_moments(vgs_ctx* ctx, int64_t K, const int32_t* labels_host, const float* field_host, int64_t n_own,
                                             int32_t n_channels, int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped, int32_t* label,
                                             int64_t* n_valid, double* anchor, double* s1, double* s2, float* vmin, float* vmax);
vgs_status vgs_own_point_label_field_moments_device(vgs_ctx* ctx, int64_t K, const int32_t* labels_dev, const float* field_dev, int64_t n_own,
                                                    int32_t n_channels, int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped,
                                                    int32_t* label, int64_t* n_valid, double* anchor, double* s1, double* s2, float* vmin,
                                                    float* vmax);
vgs_status vgs_own_point_label_class_counts(vgs_ctx* ctx, int64_t K, const int32_t* labels_host, const int32_t* cls_host, int64_t n_own,
                                            int32_t n_classes, int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* hist,
                                            int64_t* n_outside);
vgs_status vgs_own_point_label_class_counts_device(vgs_ctx* ctx, int64_t K, const int32_t* labels_dev, const int32_t* cls_dev, int64_t n_own,
                                                   int32_t n_classes, int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* hist,
                                                   int64_t* n_outside);

/* Point-level label refinement at segment boundaries (no reference counterpart).  A point's label (vgs_get_point_labels) is the label of
 * its node -- a voxel for VGS, a supervoxel for SVGS -- so segment boundaries are staircases of whole nodes, and the points of voxels with
 * at most points_min points and of clusters with at most voxels_min voxels are -1 however close a kept segment lies.  This is a NEW output
 * next to the existing labels: one int32 per input point, from the rule below.  vgs_get_point_labels, the cluster lists, every
 * per-segment table and vgs_compare_labels keep reading the node labels.  All arithmetic is float32 in the written association with no
 * FMA (csrc/vgs_math.h: vm_refine_cost).
 *
 * Inputs
 * - A point p in node v.
 * - A = kept_label[v] if v is used, else -1.
 *
 * Candidates of v.  A node w is a candidate when all of these hold:
 * - w is v itself or is in v's adjacency list, as vgs_get_lists(which = 0) gives it,
 * - w is used,
 * - kept_label[w] >= 0,
 * - VGS_F_POS and VGS_F_NRM are both set in w's record.
 *
 * Cost of w for p, with c, n the centroid and normal of w:
 * - d = p - c
 * - h = (n0*d0 + n1*d1) + n2*d2
 * - q = (d0*d0 + d1*d1) + d2*d2
 * - t = vm_sqrt(max(q - h*h, 0))
 * - e = max(t - patch_radius, 0)
 * - cost = h*h + e*e
 * This is the squared distance to the node's planar patch of radius patch_radius.  A candidate whose cost is not finite is skipped (for
 * that point it is no candidate at all).
 *
 * Choice
 * - best is the candidate with the smallest (cost, node id), compared lexicographically.
 * - c_own is the smallest cost among candidates of label A.
 * - A >= 0 and a label-A candidate exists: the point takes label[best] only if cost_best < switch_ratio * c_own.  Otherwise it keeps A.
 * - A >= 0 and no label-A candidate exists: the point keeps A.
 * - A < 0 and fill != 0: the point takes label[best], or -1 when there is no candidate.
 * - A < 0 and fill == 0: the point keeps -1.
 * - A non-finite point keeps -1.
 * - A point that is in no node keeps -1.
 *
 * A consequence: a labelled node whose candidates all carry its own label is interior and its points keep their label without any
 * arithmetic.  Only the remaining nodes -- the WORKING nodes: labelled nodes with a candidate of another label and, with fill, unlabelled
 * nodes with a candidate -- are examined.  For SVGS an unused supervoxel has an empty list and so no candidate.
 *
 * vgs_refine_params_default: patch_radius = voxel_size for VGS and seed_size for SVGS, switch_ratio = 0.25, fill = 1.
 * vgs_refine_point_labels computes the labels on the device into a buffer of the context; counts (may be NULL): 0 working nodes, 1 points
 * examined (the points of the working nodes), 2 labelled points whose label changed, 3 unlabelled points filled.  No float atomics and
 * no dependence on the order of execution: the output is a function of the inputs, bit-identical from call to call.
 * vgs_get_refined_labels copies them (N int32, input order); vgs_get_refined_labels_device hands out the device pointer.  Both are valid
 * until the next run of the stages or the next refine, and answer VGS_E_STATE without a refine since the last run.
 * VGS_E_STATE before the context is segmented and, from vgs_refine_point_labels, for a tile context (vgs_refine_own_point_labels below
 * is its counterpart there); VGS_E_ARG for a negative or non-finite patch_radius and for a switch_ratio outside [0, 1] (NaN included). */
typedef struct { float patch_radius; float switch_ratio; int32_t fill; } vgs_refine_params;
vgs_status vgs_refine_params_default(vgs_ctx* ctx, vgs_refine_params* rp);
vgs_status vgs_refine_point_labels(vgs_ctx* ctx, const vgs_refine_params* rp, int64_t* counts /* 4 */);
vgs_status vgs_get_refined_labels(vgs_ctx* ctx, int32_t* labels /* N host */);
vgs_status vgs_get_refined_labels_device(vgs_ctx* ctx, const int32_t** labels_dev /* N */);
/* Refinement on a tile context (the tiled driver: vgs_tiles_refine_point_labels, include/vgs_tiles.h, states the rule over the ranks and
 * who refines what).  Three local calls, none of which needs K:
 * vgs_get_own_band_labels: (code, global label) of this rank's owned used voxels whose centre lies within reach + graph_size + 0.5
 * voxel_size of a border line of its region (reach = max(graph_size, 0.5001 voxel_size): how far outside its region a rank still refines
 * a node), in ascending voxel id (descending code), compacted on the device: what the other ranks need beyond the run's boundary records.  Two-call protocol: code == label == NULL computes and returns *n, the call with arrays copies those records.
 * vgs_set_refine_halo_labels: as vgs_set_halo_labels, into a table of the refinement's own, so that neither call invalidates the other:
 * label[k] (>= -1) is the global label of the voxel with code[k]; codes this context does not hold or owns itself are ignored; a voxel of
 * another rank without a record stays unknown.  One record per code (two records of one code with different labels would race).  Valid
 * until the next run of the stages or new labels of the tile.
 * vgs_refine_own_point_labels: this rank's share of the rule.  A node is refined here when it holds points of the rank's own load and its
 * centre lies at most reach outside the rank's region, per axis; own points elsewhere keep their point label; the points of other
 * ranks' strips are not evaluated (-1 in the buffer).  counts (may be NULL), all this rank's share: 0 owned working nodes, 1 own points
 * examined, 2 own labelled points changed, 3 own unlabelled points filled, 4 own points left unrefined beyond the strip.  A used
 * candidate of a node this rank refines or counts whose label is unknown fails the call with VGS_E_UNSUPPORTED, the count in the message.
 * vgs_get_refined_labels[_device] then serve the tile context, in the order of its whole cloud: the own points are [own_first, own_first
 * + n_own) of vgs_set_own_point_range.
 * VGS_E_STATE before the context is segmented, for a context that is not a tile context, and for vgs_refine_own_point_labels without
 * halo labels since the last labels of the tile; VGS_E_ARG for the parameters as vgs_refine_point_labels and for a label below -1. */
vgs_status vgs_get_own_band_labels(vgs_ctx* ctx, int64_t* n, uint64_t* code, int32_t* label);
vgs_status vgs_set_refine_halo_labels(vgs_ctx* ctx, const uint64_t* code, const int32_t* label, int64_t n);
vgs_status vgs_refine_own_point_labels(vgs_ctx* ctx, const vgs_refine_params* rp, int64_t* counts /* 5 */);

/* Connected parts of ANY per-point labelling of the cloud (no reference counterpart).  The tables above treat a label as a set of points;
 * this one says whether that set is one object or several, over the scene's own neighbourhood graph: the stranded islands a refinement
 * left per segment, the instances of a semantic class, whether a labelling is spatially coherent at graph_size.
 *
 * Input.  labels[i] for every input point i < N; negative = no label; 0 <= labels[i] < K, K the caller's choice: the contract of
 * vgs_point_label_descriptors, the first offending index of a label >= K reported as there (VGS_E_ARG).
 * Nodes.  Voxels for VGS, supervoxels for SVGS: what vgs_get_point_voxel returns.  A point with no node (a non-finite point, a point
 * outside the octree) is outside the whole pass: it gets part id -1 and counts in n_skipped if its label is >= 0.
 * Vertices.  The distinct pairs (label l, node v) with at least one point of v carrying l.
 * Edges.  (l, v) and (l, w) are joined when w is in the adjacency row of v OR v is in the row of w, the rows those of
 * vgs_get_lists(which = 0): every node, used or not, every neighbour.  (The hot path stores rows for used nodes only, and these may be
 * pruned to used neighbours; the rows of the other nodes that hold a labelled point are built on request.  An edge is honoured when
 * either endpoint's row has it.)
 * Part.  A connected component of that graph; all points of (l, v) belong to the part of (l, v).
 * Numbering.  Parts are numbered 0 .. C-1 in ascending (label, smallest node id of the part): the project's own cluster order inside
 * each label.  The parts of label k are the contiguous range label_first[k] .. label_first[k + 1] - 1.
 * Outputs:
 *   part_of_point    int32  [N]      part id of every point, input order; -1 as above and for an unlabelled point
 *   part_label       int32  [C]      label of the part
 *   part_points      int64  [C]      points in the part
 *   part_nodes       int32  [C]      nodes in the part
 *   part_first_node  int32  [C]      smallest node id of the part
 *   label_first      int64  [K + 1]  first part of each label (label_first[K] = C)
 *   label_largest    int32  [K]      part with the most points of each label, the lowest id on a tie; -1 for a label no point carries
 * Everything is integer: the tables are bit-identical from call to call and from engine to engine.  No point, no finite point, no node,
 * K = 0 or all labels negative: C = 0 and every part id -1.
 * vgs_point_label_components[_device] computes the result on the device into buffers of the context (the _device variant reads the
 * labels in place); n_parts = C and n_skipped may be NULL.  vgs_get_point_label_components copies the tables out, any pointer may be
 * NULL; vgs_get_point_label_components_device hands out the device pointers (NULL for a table without rows).  Both are valid until the
 * next vgs_point_label_components or the next run of the stages, and answer VGS_E_STATE without a result since the last run.
 * vgs_absorb_point_label_parts runs this pass in the same buffers every round: it discards the result (VGS_E_STATE from the getters
 * until the next vgs_point_label_components).
 * VGS_E_STATE before the context is segmented, and for a tile context: it holds part of the cloud and of the graph only, and parts
 * across the ranks of the tiled driver are not computed by this call (vgs_tiles_point_label_components, include/vgs_tiles.h, is).  VGS_E_ARG for n != N, a NULL labelling, K outside 0 .. 2^31 - 1. */
vgs_status vgs_point_label_components(vgs_ctx* ctx, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_skipped);
vgs_status vgs_point_label_components_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_skipped);
vgs_status vgs_get_point_label_components(vgs_ctx* ctx, int32_t* part_of_point, int32_t* part_label, int64_t* part_points, int32_t* part_nodes,
                                          int32_t* part_first_node, int64_t* label_first, int32_t* label_largest);
vgs_status vgs_get_point_label_components_device(vgs_ctx* ctx, const int32_t** part_of_point, const int32_t** part_label,
                                                 const int64_t** part_points, const int32_t** part_nodes, const int32_t** part_first_node,
                                                 const int64_t** label_first, const int32_t** label_largest);
/* Adjacency graph of ANY per-point labelling of the cloud (no reference counterpart): vgs_get_segment_graph for labels that need not be
 * constant on a node -- which refined segments, which parts of vgs_point_label_components, which instances or classes touch each other,
 * across how much boundary, and how strongly the local cut's weight links them there.
 *
 * Input, nodes, vertices and rows are exactly those of vgs_point_label_components: labels[i] per input point, negative = none,
 * 0 <= labels[i] < K, the first offending index of a label >= K reported with VGS_E_ARG; nodes are what vgs_get_point_voxel returns;
 * vertices are the distinct pairs (label, node) with a point; two nodes v, w are ADJACENT when w is in the row of v or v in the row of w,
 * the rows those of vgs_get_lists(which = 0) (the rows of unused voxels that hold a labelled point are built on request, VGS only); a
 * labelled point without a node counts in n_skipped.
 * Contact of labels a < b: an unordered pair of vertices {(a, v), (b, w)} with v != w and v, w adjacent.  Each contact is counted once,
 * whichever row holds the entry.
 * Shared node of a, b: a node v with both (a, v) and (b, v) as vertices.
 * Edge {a < b}: at least one contact or one shared node.  Edges are listed in ascending (a, b); E = their number.
 * With several labels per node one node pair can carry contacts of several edges, and two contacts of one edge: {(a, v), (b, w)} and
 * {(a, w), (b, v)} when both nodes carry both labels.
 * Per edge (E rows):
 *   seg_ab    int32 x2  a, b
 *   n_shared  int64     shared nodes
 *   n_pairs   int64     contacts
 *   n_finite  int64     contacts between two USED nodes whose weight is not NaN
 *   nodes_ab  int32 x2  the vertices of a that are in at least one contact of this edge, and those of b (a shared node alone does not count)
 *   w_sum     double    sum of the weights over those n_finite contacts
 *   w_min, w_max float  their extrema; NaN when n_finite == 0
 * The weight of a contact is vm_pair_weight(node[min(v, w)], node[max(v, w)], W), the lower node id first: the entry that
 * vgs_get_local_weights reports for that ordered pair.  A contact with an unused endpoint has no weight and counts in n_pairs only.
 * When every node carries one label and only used kept nodes are labelled -- vgs_get_point_labels with K = counts[VGS_N_KEPT] --
 * n_shared is 0 and every other field is the field of vgs_get_segment_graph.
 * The integer fields, w_min and w_max are functions of the contact set alone; w_sum is summed in fp64 in a fixed shape without float
 * atomics (csrc/labelgraph.hip): the table is bit-identical from call to call and from engine to engine.  E = 0 for K <= 1, no vertex,
 * or neither contact nor shared node.  VGS_E_UNSUPPORTED for more than 2^31 (vertex, other label) records.
 * vgs_point_label_graph[_device] computes the table on the device into buffers of the context (the _device variant reads the labels in
 * place); n_edges = E and n_skipped may be NULL.  vgs_get_point_label_graph copies it out, any pointer may be NULL;
 * vgs_get_point_label_graph_device hands out E and the device pointers (NULL for E = 0).  Both are valid until the next
 * vgs_point_label_graph or the next run of the stages, and answer VGS_E_STATE without a result since the last run.  No other table, no
 * labels and no result of vgs_point_label_components are touched.
 * vgs_absorb_point_label_parts runs this pass in the same buffers every round: it discards the table (VGS_E_STATE from the getters
 * until the next vgs_point_label_graph).
 * VGS_E_STATE before the context is segmented, and for a tile context: it holds part of the cloud and of the graph only, and the graph of a
 * labelling across the ranks of the tiled driver is not computed by this call (vgs_tiles_point_label_graph does).  VGS_E_ARG for n != N, a NULL labelling, K outside 0 .. 2^31 - 1. */
vgs_status vgs_point_label_graph(vgs_ctx* ctx, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped);
vgs_status vgs_point_label_graph_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped);
vgs_status vgs_get_point_label_graph(vgs_ctx* ctx, int32_t* seg_ab, int64_t* n_shared, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                     double* w_sum, float* w_min, float* w_max);
vgs_status vgs_get_point_label_graph_device(vgs_ctx* ctx, int64_t* n_edges, const int32_t** seg_ab, const int64_t** n_shared,
                                            const int64_t** n_pairs, const int64_t** n_finite, const int32_t** nodes_ab, const double** w_sum,
                                            const float** w_min, const float** w_max);
/* Absorb the stranded and the small connected parts of ANY per-point labelling of the cloud into the neighbour they touch most (no
 * reference counterpart): the clean-up every region-growing or graph segmenter ships, as one call that takes a labelling and returns one.
 *
 * Input.  The contract of vgs_point_label_components: labels[i] for every input point i < N; negative = no label; 0 <= labels[i] < K,
 * the first offending index of a label >= K reported with VGS_E_ARG.  The input is never written.
 * Parameters (vgs_absorb_params; vgs_absorb_params_default gives min_points = 0, island_points = 0, max_rounds = 8, drop = 0, which is
 * the identity):
 *   min_points     int64 >= 0   parts below it are candidates, the largest part of a label included
 *   island_points  int64 >= 0   parts below it that are NOT the largest part of their label are candidates
 *   max_rounds     int32 0..64  the cap on the applied rounds
 *   drop           int32        != 0: what is still a candidate at the end loses its label
 * EVALUATION of a labelling L:
 *   1. cmp = vgs_point_label_components(L, K): C parts, P = part_of_point.
 *   2. g = vgs_point_label_graph(P, C), the graph OF THE PARTS.  Parts of one label are never adjacent, so every edge joins two labels.
 *      Only seg_ab, n_shared and n_pairs are used.
 *   3. threshold(p) = min_points if p == label_largest[part_label[p]], else max(min_points, island_points).
 *   4. Part p is a CANDIDATE iff part_points[p] < threshold(p) -- strictly: a part of exactly the threshold stays.  Every other part is
 *      STABLE.
 *   5. A candidate p has a TARGET if it has at least one edge {p, q} with q stable: the q with the largest triple
 *      (n_shared + n_pairs, part_points[q], -q), compared lexicographically -- most boundary, then the bigger part, then the lower part
 *      id.  A candidate never targets a candidate, which rules out swaps and cycles.
 * ROUNDS.  For r = 0, 1, ...: evaluate L.  If r == max_rounds, or no candidate has a target, this is the FINAL evaluation: stop.
 * Otherwise every point of every candidate p with a target takes part_label[target(p)], all other points keep their label -- one APPLIED
 * round -- and the next round evaluates the new labelling.  An absorbed part touches its target through a contact or a shared node, so
 * it becomes connected to it: C falls by at least one per applied round and the loop ends without the cap, which only bounds the time.
 * After the final evaluation.  With drop != 0 every point of every candidate of the final evaluation, with or without a target, gets -1:
 * the output then has no candidate under the same parameters.  Without drop, when the loop ended before the cap, every remaining
 * candidate has no stable neighbour.
 * Points outside the pass.  A labelled point without a node (non-finite, or outside the octree) keeps its label under every parameter
 * and counts in n_skipped.  Unlabelled points stay as they are (a negative value is copied through): filling them is
 * vgs_refine_point_labels' job.
 * Outputs:
 *   labels_out  int32 [N]  input order; values in -1 .. K-1 for an input whose negative values are -1
 *   counts      int64 [8]  0 applied rounds, 1 parts absorbed and 2 points relabelled, both summed over the rounds, 3 candidates of the
 *                          final evaluation, 4 their points, 5 points dropped, 6 C of the final evaluation, 7 n_skipped
 * Everything is integer: the result is bit-identical from call to call and from engine to engine.  The score deliberately does not use
 * w_sum (DESIGN.md 8 says why).
 * vgs_absorb_point_label_parts[_device] computes the result on the device into a buffer of the context (the _device variant reads the
 * labels in place); counts may be NULL.  vgs_get_absorbed_point_labels copies it out, vgs_get_absorbed_point_labels_device hands out the
 * device pointer (NULL for N = 0).  Both are valid until the next absorb call or the next run of the stages and answer VGS_E_STATE
 * without a result since the last run.  The call OVERWRITES the context's results of vgs_point_label_components and
 * vgs_point_label_graph: their getters answer VGS_E_STATE afterwards until their own next compute call.  No other table and no label
 * buffer is touched: the point labels and the refined labels stay as they are.
 * VGS_E_STATE before the context is segmented, and for a tile context: it holds part of the cloud and of the graph only, and the call
 * across the ranks of the tiled driver does not exist yet.  VGS_E_ARG for n != N, a NULL labelling or NULL params, K outside
 * 0 .. 2^31 - 1, a negative threshold, max_rounds outside 0 .. 64.  VGS_E_UNSUPPORTED of an inner pass is passed on with its message. */
typedef struct { int64_t min_points; int64_t island_points; int32_t max_rounds; int32_t drop; } vgs_absorb_params;
vgs_status vgs_absorb_params_default(vgs_absorb_params* ap);
vgs_status vgs_absorb_point_label_parts(vgs_ctx* ctx, const int32_t* labels_host, int64_t n, int64_t K, const vgs_absorb_params* ap,
                                        int64_t* counts /* 8, may be NULL */);
vgs_status vgs_absorb_point_label_parts_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t n, int64_t K, const vgs_absorb_params* ap,
                                               int64_t* counts /* 8, may be NULL */);
vgs_status vgs_get_absorbed_point_labels(vgs_ctx* ctx, int32_t* out /* N */);
vgs_status vgs_get_absorbed_point_labels_device(vgs_ctx* ctx, const int32_t** out);
/* Tile contexts (vgs_set_owned_region and vgs_set_own_point_range; VGS only): a rank's share of the connected parts of a labelling over
 * all ranks of the tiled driver.  include/vgs_tiles.h (vgs_tiles_point_label_components) states the definition and the protocol these
 * four steps serve; csrc/labelcc_tiles.hip has the kernels.  Every call answers VGS_E_STATE on a plain context and before a run.
 * vgs_own_point_label_parts[_device]: `labels` holds one int32 per point of the rank's OWN load (labels[i] belongs to cloud point
 * own_first + i, n must equal the own range's length; label rules as vgs_own_point_label_moments).  The pass of
 * vgs_point_label_components over the own points alone: the LOCAL parts, numbered in ascending (label, smallest local node id), and
 * the BAND records -- (voxel code, label, local part) of every own vertex whose node centre lies within graph_size + voxel_size of a
 * border line of the owned region (an infinite border never matches), in ascending (label, node) order.  n_parts, n_band, n_skipped may
 * be NULL.  The rows of an own vertex's node are complete on the rank when its points were loaded by region (include/vgs_tiles.h).
 * vgs_get_own_point_label_parts copies out, per local part, label, points, nodes and the shared-grid code of its first node, and the
 * band records; any pointer may be NULL.
 * vgs_link_point_label_parts: the OTHER ranks' band records (code, label, rank, part; host arrays of n entries, any order).  A code this
 * context does not hold drops out.  For every own band vertex (l, v) and every neighbour w != v in v's adjacency row (stored, or built
 * on request for an unused voxel) every record (code of w, l, s, p) gives the triple (own local part, s, p).  The triples are sorted and
 * unique; vgs_get_point_label_part_links copies them out (*n_links entries each).  The equal key itself (w = v, a voxel with points of
 * two ranks) is not a link: the driver's fold unites equal (code, label) keys.
 * vgs_apply_point_label_part_ids: `map` gives the global part of every local part (n = the own call's *n_parts); one gather writes the
 * part id of every own point, in the order of the rank's load, -1 for a point without a part.  vgs_get_point_label_part_ids copies
 * them out (n = the own range's length), the _device variant hands out the device pointer (NULL without own points).
 * All results stay until the next vgs_own_point_label_parts or the next run of the stages. */
vgs_status vgs_own_point_label_parts(vgs_ctx* ctx, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_band, int64_t* n_skipped);
vgs_status vgs_own_point_label_parts_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_band,
                                            int64_t* n_skipped);
vgs_status vgs_get_own_point_label_parts(vgs_ctx* ctx, int32_t* part_label, int64_t* part_points, int32_t* part_nodes, uint64_t* part_first_code,
                                         uint64_t* band_code, int32_t* band_label, int32_t* band_part);
vgs_status vgs_link_point_label_parts(vgs_ctx* ctx, const uint64_t* code, const int32_t* label, const int32_t* rank, const int32_t* part, int64_t n,
                                      int64_t* n_links);
vgs_status vgs_get_point_label_part_links(vgs_ctx* ctx, int32_t* own_part, int32_t* rank, int32_t* part);
vgs_status vgs_apply_point_label_part_ids(vgs_ctx* ctx, const int32_t* map, int64_t n);
vgs_status vgs_get_point_label_part_ids(vgs_ctx* ctx, int32_t* part_of_point, int64_t n);
vgs_status vgs_get_point_label_part_ids_device(vgs_ctx* ctx, const int32_t** part_of_point);
/* Tile contexts: a rank's share of the adjacency graph of a labelling over all ranks of the tiled driver.  include/vgs_tiles.h
 * (vgs_tiles_point_label_graph) states the counting rule and the protocol these steps serve; csrc/labelgraph_tiles.hip has the kernels.
 * Every call answers VGS_E_STATE on a plain context and before a run.
 * vgs_own_point_label_band[_device]: `labels` as in vgs_own_point_label_parts.  The (label, node) vertices of the own points, without
 * the union-find of the parts pass, and the BAND records -- (voxel code, label) of every own vertex whose node centre lies within
 * graph_size + voxel_size of a border line of the owned region, in ascending (label, node) order; none for K <= 1.  n_band and n_skipped
 * may be NULL.  vgs_get_own_point_label_band copies the records out; either pointer may be NULL.  The pass overwrites the vertex arrays
 * of vgs_own_point_label_parts (whose later steps then answer VGS_E_STATE until the next own parts), and the reverse.
 * vgs_own_point_label_graph: the OTHER ranks' band records (code, label; host arrays of n_foreign entries, any order).  A code this
 * context does not hold and a label outside 0 .. K-1 drop out; the rest is merged with the own vertices, a vertex two ranks publish
 * being one vertex.  The walk of vgs_point_label_graph then runs over the merged list under the rule of include/vgs_tiles.h: vertices at
 * owned nodes walk in full, vertices at non-owned unused nodes only speak for owned vertices when the stored rows are pruned, every
 * other vertex is left to its owner.  *n_edges = the rows of this rank's PARTIAL table, in ascending (a, b).
 * vgs_get_own_point_label_graph copies the partial table out (fields and types of vgs_get_point_label_graph; any pointer may be
 * NULL); the sum of the ranks' partial tables is the table of the whole scene (vgs_tiles_fold_label_edges).
 * vgs_get_own_point_label_graph_counts (for the driver's payload figures): band records of the last own pass, foreign records whose code
 * was found in the local grid -- counted before the label check, so a record dropped for a label outside 0 .. K-1 is among them --,
 * partial edges.
 * All results stay until the next vgs_own_point_label_band, the next vgs_own_point_label_parts or the next run of the stages. */
vgs_status vgs_own_point_label_band(vgs_ctx* ctx, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_band, int64_t* n_skipped);
vgs_status vgs_own_point_label_band_device(vgs_ctx* ctx, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_band, int64_t* n_skipped);
vgs_status vgs_get_own_point_label_band(vgs_ctx* ctx, uint64_t* code, int32_t* label);
vgs_status vgs_own_point_label_graph(vgs_ctx* ctx, const uint64_t* code, const int32_t* label, int64_t n_foreign, int64_t* n_edges);
vgs_status vgs_get_own_point_label_graph(vgs_ctx* ctx, int32_t* seg_ab, int64_t* n_shared, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                         double* w_sum, float* w_min, float* w_max);
vgs_status vgs_get_own_point_label_graph_counts(vgs_ctx* ctx, int64_t* n_band, int64_t* n_hits, int64_t* n_edges);

/* ---- multi-GPU support (spatial tiles) -------------------------------------- */
/* The reference is single-process; these entry points are what a tiled driver needs around the same stages.
 * One context per GPU holds one tile plus a halo of raw points (2*graph_size + voxel_size wide).
 * Shared grid: the octree growth state (PCL OctreePointCloud box) is chained rank to rank. */
typedef struct { double min[3]; uint64_t shift[3]; int32_t depth; int32_t defined; } vgs_grid_state;
vgs_status vgs_grid_state_init(vgs_grid_state* g);
/* advance g over this context's points in index order (what inserting them after all earlier ranks' points does
 * to the octree box); call on rank r after receiving g from rank r-1 */
vgs_status vgs_grid_advance(vgs_ctx* ctx, vgs_grid_state* g);
/* shortcut of the chain: bounding box (min x, y, z, max x, y, z) and number of the finite points of this context's cloud,
 * and the replay of the growth over a cloud of which only that box is known (host arithmetic, no context).  The replay
 * advances g while the growth step is the same for every point outside the box and sets *need_scan when it is not (or
 * when g is still undefined): then vgs_grid_advance on the owner of the cloud continues from the state reached. */
vgs_status vgs_points_bbox(vgs_ctx* ctx, float* bbox6, int64_t* n_finite);
vgs_status vgs_grid_advance_bbox(vgs_grid_state* g, double voxel_size, const float* bbox6, int32_t* need_scan);
/* pin the final grid before vgs_voxelize: every rank bins with the state left by the last rank */
vgs_status vgs_set_grid(vgs_ctx* ctx, const vgs_grid_state* g);
/* the same from a caller that has replayed the growth over THIS context's cloud itself (vgs_grid_advance on it, or
 * vgs_grid_advance_bbox over its bounding box, as the tiled driver does for every rank): the voxelize stage then takes the grid
 * as final without scanning the points for one outside it (0.2 ms of a 10 M-point tile's step).  A point outside such a grid
 * is the caller's error and is binned with a wrapped key; vgs_set_grid keeps the check.  Reset by the next vgs_set_points. */
vgs_status vgs_set_grid_covering(vgs_ctx* ctx, const vgs_grid_state* g);
/* this rank owns the voxels whose centre lies in [lo, hi) in x and y; others are halo (computed redundantly,
 * their own connections are not trusted).  Components are then built from the connections that have an owned
 * endpoint, cluster sizes count owned voxels, and point labels wait for vgs_apply_root_labels. */
vgs_status vgs_set_owned_region(vgs_ctx* ctx, const double* lo_xy, const double* hi_xy);
/* A rank's cloud = the points it loaded itself + the border strips of the other ranks, assembled IN RANK ORDER: strips of lower
 * ranks, own points, strips of higher ranks -- the order in which a single process would have inserted them, because a voxel's
 * attributes depend on the order of its points (sequential float sums, the normal's flip looks at the voxel's first point, VS:1364,
 * 1394).  Points [first, first + n_own) are the rank's own load.  A voxel that holds points of both kinds (an object that reaches over
 * a tile's edge) becomes a boundary voxel on the rank that owns it and on the rank that loaded the foreign points, so the latter
 * learns the label of those points from the owner's record.  Call after vgs_set_points*; n_own = -1 switches it off. */
vgs_status vgs_set_own_point_range(vgs_ctx* ctx, int64_t first, int64_t n_own);
/* after vgs_segment: (global voxel code, local component root) records of the boundary voxels -- both endpoints of
 * every connection that crosses the ownership border, and every owned voxel with a halo voxel in its neighbourhood
 * (a possible closestCheck target of the neighbouring rank); duplicates possible.  Records of all ranks that share
 * a code name the same segment.  Two-call protocol: code == NULL returns the count. */
vgs_status vgs_get_boundary(vgs_ctx* ctx, int64_t* n_records, uint64_t* code, int32_t* root);
/* local component roots that contain owned voxels, with the number of owned voxels (two-call protocol) */
vgs_status vgs_get_owned_roots(vgs_ctx* ctx, int64_t* n_roots, int32_t* root, int32_t* owned_voxels);
/* final labels: label[k] for local root root[k] (-1 = dropped); points of halo voxels and of unlisted roots get -1 */
vgs_status vgs_apply_root_labels(vgs_ctx* ctx, const int32_t* root, const int32_t* label, int64_t n_roots);
/* Compact form of the two calls above, everything but the border stays on the GPU: the boundary records without
 * duplicates (one per boundary voxel: code, local root, number of owned voxels of that root), and the number of
 * local components that touch no boundary record and pass the `> voxels_min` filter on their own (their labels are
 * local_base + rank in ascending root order).  Two-call protocol: code == NULL computes and returns the counts. */
vgs_status vgs_get_boundary_roots(vgs_ctx* ctx, int64_t* n_records, uint64_t* code, int32_t* root, int32_t* owned_voxels,
                                  int64_t* n_kept_local);
/* final labels of a tile: label[k] for boundary root root[k] (-1 = dropped), local_base + rank for the kept
 * components without boundary records, -1 for everything else and for the points of halo voxels */
vgs_status vgs_apply_tile_labels(vgs_ctx* ctx, int32_t local_base, const int32_t* root, const int32_t* label, int64_t n_roots);

#ifdef __cplusplus
}
#endif
#endif /* VGS_H_ */
