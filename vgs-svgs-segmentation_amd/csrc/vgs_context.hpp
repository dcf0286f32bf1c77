// vgs_context.hpp -- internal state of one engine context (device buffers, stream, stage state).
// Data model in HBM (SoA, grow-only buffers reused across runs; sized for 288 GB):
//   points      xyz_in (caller stride) -> sort keys code[N] (u64), perm[N] (u32)        voxelize
//   voxels      vox_code[V] (u64 Morton, x-major), vox_start[V+1], node[V] (64 B record) features
//   hash        hkey[H] (u64), hval[H] (u32), H = pow2 >= 2V                             adjacency
//   adjacency   adj_key[U * stride] (u64: float bits of d2 << 32 | voxel id), adj_cnt[U] adjacency
//   connect     conn[U * stride] (u8 bit0 = in L0(i), bit1 = mutual)                     local cut / merge
//   components  parent[V], vox_label[V], point label[N]                                  merge / labels
#ifndef VGS_CONTEXT_HPP_
#define VGS_CONTEXT_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/vgs.h"
#include "vgs_math.h"
#include "counter_words.hpp"
#include "pairlist.hpp"

typedef VgsNode NodeRec;
static_assert(sizeof(NodeRec) == 64, "NodeRec must be 64 bytes");

// One-workgroup-per-item kernels: workgroup b runs on XCD b % 8 (observed dispatch order; used for speed only), so
// item = (b % 8) * ceil(n/8) + b / 8 hands every XCD one contiguous eighth of the Morton-ordered item list and
// spatial neighbours share an L2.  Launch vgs_xcd_grid(n) workgroups and drop items >= n.
#ifdef __HIPCC__
__device__ __forceinline__ int64_t vgs_xcd_item(unsigned int b, int64_t n) {
  const int64_t per = (n + 7) >> 3;
  return (int64_t)(b & 7u) * per + (int64_t)(b >> 3);
}
#endif
static inline unsigned int vgs_xcd_grid(int64_t n) { return (unsigned int)(((n + 7) >> 3) << 3); }

// grow-only device buffer; it owns its memory (freed with the buffer: a context's members by `delete`, a local on every return path)
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }   // (std::swap of two label buffers: merge.hip)
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    size_t want = n + n / 8 + 64;
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e != hipSuccess) return e;
    cap = want;
    return hipSuccess;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// PCL OctreePointCloud bounding-box growth: product-side restatement used by the host
// part of the voxelize stage (the oracle has its own copy; the two never share code).
struct OctreeBox {
  double min[3] = {0, 0, 0}, max[3] = {0, 0, 0};
  double res = 0;
  int depth = 0;
  bool defined = false;
  uint64_t shift[3] = {0, 0, 0};
  bool contains(const float* p) const;
  void adopt(const float* p);  // grows until p fits
};

struct Epoch {  // keys of points with index >= first use this box
  int64_t first;
  double min[3];
  uint64_t shift[3];
};

#define VGS_MAX_EPOCHS 96

// segment graph (seggraph.hip): one record per (used node u, neighbour label B != u's label A) -- over u's neighbours v > u of label B --
// and one partial per chunk of an edge's sorted records
struct SgRec {
  double w_sum;
  uint32_t cnt_lt, n_finite;
  int32_t a, b;   // A, B
  float w_min, w_max;
};
struct SgPart {
  double w_sum;
  int64_t n_pairs, n_finite;
  int32_t nodes_a, nodes_b;
  float w_min, w_max;
};

// graph of a point labelling (labelgraph.hip): one record per (vertex (A, u), other label B) as the vertex's own row walk sees it, and one
// proxy record per contact that the other endpoint's row lacks (a = the other vertex's label, b = the walker's); one partial per chunk
struct LgRec {
  double w_sum;
  uint32_t cnt, n_finite;   // contacts counted from this side, and those with a finite weight
  int32_t a, b;             // the label of the record's vertex, the other label
  float w_min, w_max;
  uint32_t t;               // the record's vertex: its position in (node, label) order
  uint32_t flags;           // LG_CONTACT: the vertex is in a contact of {a, b}; LG_SHARED: its node carries b too
};
struct LgPart {
  double w_sum;
  int64_t n_pairs, n_finite, n_shared;
  int32_t nodes_a, nodes_b;
  float w_min, w_max;
};

enum Stage { ST_NONE = 0, ST_POINTS = 1, ST_VOXELS = 2, ST_FEATURES = 3, ST_ADJACENCY = 4, ST_SEGMENTED = 5 };

// Diagnostics / schedule-tuning knobs (none changes a result).  Read from the environment ONCE, when the context is created
// (vgs_read_env_knobs): a stage never calls getenv, so a host that changes its environment between two calls cannot make the
// two halves of a stage disagree.
struct VgsKnobs {
  int a1_max = 4;            // VGS_A1MAX: own near-list length up to which a class-A voxel goes first
  float shell0 = 8.0f;       // VGS_SHELL0
  float cap_frac = 0.7f;     // VGS_CAPFRAC
  int dbg_stop = 0;          // VGS_DBG_STOP
  int max_rounds = 6;        // VGS_ROUNDS
  int dbg_max_m = 0;         // VGS_DBG_MAXM
  int dbg_xl_from = 0;       // VGS_DBG_XL_FROM: tests -- the 2048-vertex general kernel passes neighbourhoods above N on to the extra-large one
  int near_min_own = 7;      // VGS_NEARMINOWN
  int fv_blocks = 512;       // VGS_FV_BLOCKS
  int only_class = -1;       // VGS_ONLY_CLASS (-DVGS_PROF builds)
  bool no_dense = false;     // VGS_NO_DENSE
  bool no_overlap = false;   // VGS_NO_OVERLAP
  bool no_near = false;      // VGS_NO_NEAR
  bool no_adjmasks = false;  // VGS_NO_ADJMASKS
  int vote_period = 64;          // VGS_VOTE_PERIOD (power of two): one voxel in so many of the one-wavefront classes runs as a sample
  int cross_lds_kb = 0;          // VGS_CROSS_LDS: KB of (unused) LDS per wavefront of crossValidation's FIRST pass and its unions -- caps how many
                                 // of them a CU holds beside the hand-over kernel's workgroups, which need four wave slots at once
  bool no_sort32 = false;        // VGS_NO_SORT32: the one-wavefront classes of the local cut keep the 64-bit sort network (A/B twin of round 6's one-word keys)
  bool no_pg_xl = false;         // VGS_NO_PG_XL: no extra-large pair-list instantiation (neighbourhoods above 1024 voxels take the hand-over path)
  bool no_connbits = false;  // VGS_NO_CONNBITS: crossValidation searches the neighbour's row (the path of rounds 1-3)
  bool no_pairlists = false; // VGS_NO_PAIRLISTS: no pair lists (pairlist.hpp); hand-overs and wide classes take the kernels of round 4
  bool no_vote = false;      // VGS_NO_VOTE: every one-wavefront voxel tries the lazy schedule (LwParams::vote off)
  int ho_grid = -1;          // VGS_HO_GRID: workgroups of the hand-over kernels of the one-wavefront classes (-1: as many as the device holds at once; 0: one per row up to 16384)
  int pg_min_frac = 8;       // VGS_PG_MINFRAC: hand-overs go through the pair lists when they are more than 1/N of the used voxels (0: never)
  int pg_wide = 1;           // VGS_PG_WIDE: neighbourhoods above 128 voxels are cut from the pair lists (0: the multi-wavefront shell classes)
  int pg_wide_frac = 8;      // VGS_PG_WIDEFRAC: ... when they are more than 1/N of the used voxels
  bool debug = false;        // VGS_DEBUG
};

struct vgs_ctx {
  vgs_params P;
  VgsKnobs K;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // side streams: the heavy local-cut classes overlap the light one
  hipStream_t stream3 = nullptr;
  hipStream_t stream4 = nullptr;
  std::string err;
  int stage = ST_NONE;
  void* pin = nullptr;   // VGS_PIN_BYTES of pinned host memory: small read-backs land here (a pageable destination makes the copy blocking and slower)

  // input
  const float* xyz = nullptr;  // device pointer (one of xyz_buf or the caller's)
  // two input buffers: while the stages run on one cloud, vgs_stage_points copies the next one into the other on the
  // upload stream (a sequence of clouds; the points are read by the voxelize stage only)
  DevBuf<float> xyz_buf[2];
  int xyz_cur = 0;
  hipStream_t s_h2d = nullptr, s_d2h = nullptr;   // copy streams: uploads of the next cloud, downloads of the last labels
  hipEvent_t ev_h2d = nullptr, ev_d2h = nullptr;
  hipEvent_t ev_rb = nullptr;    // split read-backs (vgs_readback_begin / _end)
  bool gathered = false;         // voxelize: the leaf-order gather was queued behind the count read-back
  bool bricks_ready = false;     // the features stage has already queued the brick table of this voxel table (behind its read-back)
  // front fork (vgs_run, VGS route): the gather of the points and k_features run on stream2 beside the voxel table, the used flags, the
  // brick table and the adjacency rows on the main stream
  bool ff_want = false;          // vgs_run asks the voxelize stage to leave the gather to the fork
  bool ff_pending = false;       // ... which it did: the features stage forks behind the brick table (vgs_front_fork)
  bool ff_open = false;          // stream2 carries work of this run that the main stream has not joined yet (vgs_front_join)
  hipEvent_t ev_ff_fork = nullptr, ev_ff_join = nullptr;   // the brick table's kernels queued on the main stream / side chain done
  bool staged = false;         // a cloud is on its way into xyz_buf[1 - xyz_cur]
  int64_t staged_n = 0;
  int staged_stride = 12;
  bool pt_labels_pending = false;    // a tile's merge stage did not scatter the per-point labels (vgs_ensure_point_labels does, on request)
  bool labels_event_valid = false;   // EV_LABELS_END has been recorded behind the last kernel that wrote pt_label
  bool d2h_open = false;       // vgs_get_point_labels_async has a copy in flight ...
  const int32_t* d2h_src = nullptr;   // ... out of this buffer
  int64_t N = 0;
  int stride_f = 3;

  // octree
  OctreeBox box;
  bool grid_pinned = false;
  bool grid_covers = false;   // ... and the caller vouches that it covers every finite point of the current cloud (vgs_set_grid_covering): no scan
  int n_epochs = 0;   // growth epochs of the last voxelize (the epochs themselves stay in grow_state on the device)

  // voxelize
  DevBuf<uint64_t> code_a, code_b;
  DevBuf<uint32_t> perm_a, perm_b;
  DevBuf<uint8_t> sort_tmp;
  DevBuf<uint64_t> grow_state;         // GrowState of the box growth (voxelize.hip)
  DevBuf<uint32_t> pt_vox;             // per sorted position
  DevBuf<uint32_t> vox_tile;           // per tile of the sorted keys: run heads (then heads in front of the tile), valid keys
  DevBuf<uint32_t> head_flag;          // flags in front of a scan: scratch of the later stages (features, merge, supervoxels, boundary records)
  DevBuf<uint64_t> vox_code;
  DevBuf<uint32_t> vox_start;
  DevBuf<float> xs, ys, zs;  // points in sorted order (SoA)
  int64_t Nf = 0;            // finite points
  int64_t V = 0;
  int code_bits = 0;

  // features
  DevBuf<NodeRec> node;
  DevBuf<uint32_t> used_ids, used_rank;
  int64_t U = 0;

  // adjacency
  DevBuf<uint64_t> hkey;
  DevBuf<uint32_t> hval;
  uint32_t hbits = 0;
  DevBuf<int32_t> offsets;  // packed dx,dy,dz
  DevBuf<uint64_t> adj_masks;  // ball cells per (voxel position in its brick, brick offset): k_adjacency_masks
  int adj_mask_nb = 0;         // bricks per axis the ball can touch (0 = no mask table)
  bool adj_tab_valid = false;  // offsets / masks / length tables are on the device for (adj_tab_graph, adj_tab_voxel)
  float adj_tab_graph = 0.f, adj_tab_voxel = 0.f;
  // per adjacency row: start position of every group of equal integer offset length (crossValidation searches only
  // inside the group of the wanted distance); adj_nvals = the distinct lengths, adj_nrank[length] = its index
  DevBuf<uint16_t> adj_gtab;
  DevBuf<int32_t> adj_nvals;
  DevBuf<uint8_t> adj_nrank;
  int adj_ngroups = 0, adj_gstride = 0;
  bool adj_have_gtab = false;
  int n_off = 0;
  int adj_R = 0;   // largest |offset| per axis of the ball table
  int adj_stride = 0;
  DevBuf<uint64_t> adj_key;
  DevBuf<uint16_t> adj_off;   // per row entry: packed lattice offset from the row's voxel, (dx+16) | (dy+16) << 5 | (dz+16) << 10; row[0] = 0xffff: none
  bool adj_have_off = false;
  // crossValidation through the lattice (round 4): every cut also leaves its connect list as a BIT per lattice offset (conn_bits: U
  // rows of cb_words words; bit = vgs_cb_index(offset) in the cube of side 2 cb_R + 1 around the voxel, cb_R = the ball's largest
  // offset per axis; the centre bit -- the voxel itself, always a member -- says "this row has bits"), so "is i in L0(k)?" is one
  // bit of k's row, at the index of the negated offset = cube size - 1 - index, instead of a search in k's 8-byte keys.
  DevBuf<uint32_t> conn_bits;
  int cb_words = 0, cb_R = 0;
  bool cb_enabled = false;     // the cuts of this run wrote conn_bits
  DevBuf<uint32_t> adj_cnt, adj_mused;  // per used voxel: stored row length, number of ALL neighbours
  bool adj_pruned = false;              // rows hold used neighbours only
  float adj_r2 = 0.f;

  // near-pair lists (nearlist.hip): per voxel id, the heavy pairs with a used voxel at most two lattice steps away
  DevBuf<uint8_t> nl_cnt;
  DevBuf<uint32_t> nl_tot;
  DevBuf<float4> nl_ent;
  bool nl_enabled = false;
  int nl_reach_steps = 0;     // lattice steps up to which the lists are complete (nearlist.hip)
  bool nl_direct = false;     // the ball fits the direct offset map of the one-wavefront classes

  // pair lists (pairlist.hip): every heavy pair inside a voxel's ball, built on demand for the rows k_localcut_pg reads
  DevBuf<uint8_t> pl_state;    // [V] index (uint2: first entry, count) | [V] wanted marks | [V] "part of a heavy pair" flags: one fill resets all three
  DevBuf<float4> pl_ent;       // the pool of entries
  DevBuf<uint32_t> pl_work;    // work list of rows, redo list
  bool pl_enabled = false;
  bool pl_enabled_at_launch = false;   // this run queued the pair-list chain for its hand-overs (stream4 joins stream3 before the stage's last event)
  hipEvent_t ev_ho = nullptr;    // local cut: the hand-over lists are built and LcGate's word is written; stream3 (behind k_ho_lists); stream4 waits (the pair-list chain)
  hipEvent_t ev_ho2 = nullptr;   // local cut, two meanings by path: pair-list path of the wide classes -- their rows are built; stream2; stream4 waits.  Hand-overs through
                                 // the pair lists -- the pair-list chain is done; stream4; stream3 waits before EV_LC_HO_DONE.  (The first wait is queued before the second record.)
  hipEvent_t ev_fork = nullptr;  // merge stage, two meanings in turn: crossValidation's first pass done; main stream; stream3 waits (the side chain).  Then, its wait queued: the
                                 // second pass over the rows put off done; side stream; the main stream waits (their unions)
  hipEvent_t ev_join = nullptr;  // merge stage: the side chain is done (closestCheck; or, many hand-overs, the finish alone); side stream; the main stream waits
  float pl_w_ring = 0.0f;      // PairLists::w_ring of this run

  // local cut / merge
  DevBuf<uint8_t> conn;
  DevBuf<uint32_t> evals;      // per used voxel: pair evaluations of its local cut (diagnostics, summed on request)
  // hand-overs of the local cut run on a side stream while the merge stage already cross-validates the rows they cannot
  // touch: per used voxel "handed over, connect row not final yet", the rows put off, and what vgs_localcut_finish needs
  DevBuf<uint8_t> lc_pending;
  DevBuf<uint8_t> lc_defer_flag;   // per row: the first pass of crossValidation put it off (written by every row of that pass)
  DevBuf<uint32_t> lc_defer;
  // what the launch half of the local cut (vgs_stage_localcut) leaves for its finish (vgs_localcut_finish) and for the merge stage
  struct LcTail {
    bool open = false;           // the hand-over kernels of a run may still be on the side streams: nobody has collected them yet
    bool dense = true;           // the hand-overs went to the dense / pair-list kernels (false: VGS_NO_DENSE, the general kernel's fixed grids)
    bool gated = false;          // merge's first pass looks at LcGate's word ...
    bool many = false;           // ... and the finish found LC_MANY in it
    unsigned int grid_f = 0;     // workgroups of the one-wavefront classes' hand-over launch
    unsigned int grid_g = 0;     // ... of the wide classes' (the general kernel's fixed grid)
    unsigned int nabc[5] = {0, 0, 0, 0, 0};   // class sizes A, B, C + C0, D, A1 as the host knew them at the launch
    float tail_ms = 0.f;         // EV_LC_MAIN_END -> EV_LC_END of the last finish
    bool pg_xl_queued = false;   // class D's pair-list kernel queued for the extra-large one, which was launched
    bool rb_queued = false;      // vgs_localcut_finish_queue has queued the finish's read-back
  } lc_tail;
  int64_t lc_diag[16] = {0};   // vgs_get_schedule_counters[_ex]
#ifdef VGS_PROF
  DevBuf<uint32_t> lc_dbg;     // per-voxel cycle / round counters of the diagnostics build (localcut.hip)
#endif
  DevBuf<float> lc_ctab;      // screening table of the dense hand-over kernels (localcut.hip: lc_screen_table)
  float lc_ctab_key[8] = {0}, lc_ctab_scale = 0.0f;
  bool lc_ctab_valid = false;
  DevBuf<uint32_t> csize;      // per voxel: list length after crossValidation (0 for unused)
  DevBuf<int32_t> attach;      // per voxel: closestCheck target or -1
  DevBuf<uint8_t> cc_flags;    // per voxel: bit0 candidate, bit1 success
  DevBuf<uint32_t> parent;
  DevBuf<uint32_t> csz, kept_rank;
  DevBuf<int32_t> vox_label;
  DevBuf<int32_t> pt_label;      // labels of the current cloud
  DevBuf<int32_t> pt_label_alt;  // the buffer the next run writes while an asynchronous download still reads pt_label
  // getClusterIdx on the device (clusters.hip): offsets and point indices of the kept clusters, default order; rebuilt after a run on request
  DevBuf<int64_t> cl_off;
  DevBuf<int32_t> cl_idx;
  bool cl_valid = false;
  // per-segment descriptors (segdesc.hip): the table of the kept segments, computed on request, valid until the next run (sd_valid); the
  // sort, scans and partial records of that computation use their own scratch (no getter reads it)
  DevBuf<uint32_t> sd_key, sd_ids, sd_vp, sd_seg;
  DevBuf<uint8_t> sd_tmp;
  DevBuf<double> sd_part;
  DevBuf<int64_t> sd_npts;
  DevBuf<int32_t> sd_nnodes;
  DevBuf<float> sd_bbox, sd_eig8;
  DevBuf<double> sd_cen, sd_cov, sd_eval, sd_evec;
  bool sd_valid = false;
  // oriented boxes of the kept segments (segbox.hip), one table per frame (VGS_BOX_PRINCIPAL, VGS_BOX_UPRIGHT): computed on request, valid
  // until the next run (sb_valid[frame]); the frame the extents were taken in is the table's own copy, and the chunk partials its own scratch
  DevBuf<double> sb_part;
  DevBuf<double> sb_frame[2], sb_lo[2], sb_hi[2], sb_half[2], sb_center[2];
  bool sb_valid[2] = {false, false};
  // tile contexts (vgs_get_own_segment_extents / vgs_segment_boxes_from_extents): the descriptor rows handed in (centroid3 | cov6 | evecs9),
  // the frames made from them, the rows that come out (lo3 | hi3 | half3 | center3), one chunk per segment; nothing a cached table reads
  DevBuf<double> sbt_in, sbt_frame, sbt_out;
  DevBuf<uint32_t> sbt_idx;
  // per-segment statistics of a caller's point attributes (segfield.hip): computed on every call, nothing cached.  The host variants' upload
  // (sf_in, sf_cls), the chunk partials of one channel group, and the tables the rows are copied out of: K x n_channels for the field
  // statistics; K x n_classes counts, then n_outside and majority_count (K each) in sf_hist, majority in sf_maj.  Tile contexts
// (vgs_get_own_segment_field_moments, vgs_segment_field_stats_from_moments): a rank's S1 and S2 leave through sf_mean and sf_var; the
// folded moments come in as one partial per (segment, channel) in sf_part, one chunk per segment (sf_idx)
  DevBuf<float> sf_in, sf_min, sf_max;
  DevBuf<int32_t> sf_cls, sf_maj;
  DevBuf<double> sf_part, sf_anchor, sf_mean, sf_var;
  DevBuf<int64_t> sf_nvalid, sf_hist;
  DevBuf<uint32_t> sf_idx;
  // tile contexts (vgs_get_own_segment_moments / vgs_segment_descriptors_from_moments): first own point per segment, moment records
  DevBuf<uint32_t> sd_apos;
  DevBuf<double> sd_mom;
  // segment adjacency graph (seggraph.hip): the edge table of the kept segments, computed on request, valid until the next run (sg_valid);
  // its effective labels, per-row records, sort, scans and partials use their own scratch (no getter reads it)
  DevBuf<int32_t> sg_lab;
  DevBuf<uint32_t> sg_nrec, sg_ridx, sg_ework, sg_meta;
  DevBuf<uint64_t> sg_roff, sg_rkey;
  DevBuf<SgRec> sg_rec;
  DevBuf<SgPart> sg_part;
  DevBuf<uint8_t> sg_tmp;
  DevBuf<int32_t> sg_ab, sg_nodes;
  DevBuf<int64_t> sg_npairs, sg_nfin;
  DevBuf<double> sg_wsum;
  DevBuf<float> sg_wmin, sg_wmax;
  int64_t sg_E = 0;
  bool sg_valid = false;
  // tile contexts (vgs_set_halo_labels / vgs_get_own_segment_graph): the global label of every voxel this rank does not own (SG_UNKNOWN
  // without a record), the (code, label) upload, per-row counts of unknown neighbours
  DevBuf<int32_t> sg_halo, sg_hlab;
  DevBuf<uint64_t> sg_hcode;
  DevBuf<uint32_t> sg_nunk;
  bool sg_halo_valid = false;
  int64_t sg_own_K = -1;   // the key space of the tile table the sg_* outputs hold (-1: none)
  // comparison with a caller's labelling (segcompare.hip): the cells, the reference table and the segment table of the last
  // vgs_compare_labels, valid until the next compare or the next run (cmp_valid).  cmp_ref the host variant's upload; keys, flags, scans,
  // sorts and run starts their own scratch.  Several arrays share a buffer: cell_seg | cell_ref at a stride of cmp_ann, ref_id |
  // ref_best_seg and ref_points | ref_dropped | ref_best_n at a stride of cmp_cells, seg_annotated | seg_best_n and seg_refs |
  // seg_best_ref at a stride of max(cmp_K, 1)
  DevBuf<int32_t> cmp_ref, cmp_cell_i32, cmp_ref_i32, cmp_seg_i32;
  DevBuf<int64_t> cmp_cell_n, cmp_ref_i64, cmp_seg_i64;
  DevBuf<double> cmp_ref_iou, cmp_seg_iou;
  DevBuf<uint64_t> cmp_key, cmp_meta;
  DevBuf<uint32_t> cmp_work, cmp_cstart, cmp_rowstart, cmp_rsort, cmp_rstart;
  DevBuf<uint8_t> cmp_tmp;
  int64_t cmp_ann = 0, cmp_cells = 0, cmp_refs = 0, cmp_K = 0, cmp_summary[12] = {0};
  bool cmp_valid = false;
  // tile contexts (vgs_own_label_cells): the cells over the own points wait in cmp_cell_i32 / cmp_cell_n at a stride of cmp_ann until
  // vgs_get_own_label_cells; -1: none.  vgs_label_comparison_from_cells stages its input in cmp_ref (seg | ref) and cmp_key (keys, counts)
  int64_t cmp_own_cells = -1;
  // point-level label refinement (refine.hip): the refined labels in input order, valid until the next run or the next refine (rf_valid).
  // Scratch of its own: per listed node the number of point batches and their scan, the ids of the unused voxels, and for a chunk of
  // those the adjacency rows that the hot path does not keep (keys, lengths, neighbour counts)
  DevBuf<int32_t> rf_label;
  DevBuf<uint32_t> rf_batches, rf_start, rf_ids, rf_cnt, rf_nall;
  DevBuf<uint64_t> rf_rows, rf_counts;
  bool rf_valid = false;
  // tile contexts (vgs_set_refine_halo_labels / vgs_get_own_band_labels / vgs_refine_own_point_labels): the global label of every voxel this
  // rank does not own (RF_UNKNOWN without a record) -- a table of the refinement's own, beside sg_halo -- and its (code, label) upload;
  // per voxel the effective label and the mask (bit 0 refinable, bit 1 owned); the band records (code, label) of the owned used voxels
  // near a border line, rf_band_n of them (-1: not computed)
  DevBuf<int32_t> rf_halo, rf_hlab, rf_eff, rf_blab;
  DevBuf<uint64_t> rf_hcode, rf_bcode;
  DevBuf<uint8_t> rf_mask;
  bool rf_halo_valid = false;
  int64_t rf_band_n = -1;
  // descriptors and boxes of a caller's per-point labelling (pointseg.hip): computed on every call, nothing cached.  The host variants'
  // upload (ps_in, which vgs_compare_point_labels shares), keys in | out and sorted positions in | out (Nf words each half), label starts |
  // chunk counts | first chunks (K + 1 words each), rocprim's storage, the chunk partials and head-flag counts, the two counters of the
  // key pass, and the K rows the caller's arrays are copied out of: bbox6 | eigen8 in ps_f; centroid3 | cov6 | evals3 | evecs9 | frame9 |
  // lo3 | hi3 | half3 | center3 in ps_d
  DevBuf<int32_t> ps_in, ps_nnodes;
  DevBuf<uint32_t> ps_key, ps_val, ps_seg, ps_nn;
  DevBuf<uint8_t> ps_tmp;
  DevBuf<uint64_t> ps_meta;
  DevBuf<double> ps_part, ps_d;
  DevBuf<float> ps_f;
  DevBuf<int64_t> ps_npts;
  // tile contexts (vgs_own_point_label_moments): the shared-voxel flags (V bytes), pair flags | their scan (Nf words each), the compacted
  // pair records; the moment records use ps_d.  The compact records wait on the host until vgs_get_own_point_label_moments: pso_K rows
  // were asked for (-1: none; a run of the stages or new labels discard them)
  DevBuf<uint8_t> ps_shared;
  DevBuf<uint32_t> ps_flag;
  DevBuf<uint64_t> ps_pcode;
  DevBuf<int32_t> ps_plab;
  std::vector<int32_t> pso_label, pso_nnodes, pso_plab;
  std::vector<int64_t> pso_npts;
  std::vector<float> pso_bbox, pso_anchor;
  std::vector<double> pso_s9;
  std::vector<uint64_t> pso_pcode;
  int64_t pso_K = -1;
  // connected parts of a caller's per-point labelling (labelcc.hip): the result of the last vgs_point_label_components, valid until the
  // next one or the next run of the stages (lcc_valid) -- part of every point (N), label, points, nodes and first node of every part
  // (lcc_C rows), first part (lcc_K + 1) and largest part (lcc_K) of every label.  Scratch of its own: head flags and their scan (Nf + 1
  // words each), the vertex arrays node | label | first point | parent | root | part (vertices + 1 words each) and the scan over them,
  // the lowest | highest vertex of every node (V words each), the first vertex (K + 1) and the fold word (K) of every label, the list
  // (vertex | node) of the vertices of unused voxels.  The sort is
  // pointseg.hip's (ps_*), the rows built for unused voxels sit in refine.hip's chunk (rf_rows, rf_cnt, rf_nall).  (lc_* is the local cut's.)
  DevBuf<int32_t> lcc_pop, lcc_plabel, lcc_pnodes, lcc_pfirst, lcc_llargest;
  DevBuf<int64_t> lcc_ppoints, lcc_lfirst;
  DevBuf<uint32_t> lcc_flag, lcc_vex, lcc_vtx, lcc_vscan, lcc_vfirst, lcc_uv, lcc_nidx;
  DevBuf<uint64_t> lcc_lmax;
  int64_t lcc_C = 0, lcc_K = 0;
  uint32_t lcc_nv = 0;   // vertices of the last pass (the arrays of lcc_vtx hold lcc_nv + 1 words each)
  bool lcc_valid = false;
  // adjacency graph of a caller's per-point labelling (labelgraph.hip): the table of the last vgs_point_label_graph (lg_E rows), valid
  // until the next one or the next run of the stages (lg_valid).  Scratch of its own: per vertex the record count and first record, per
  // record the record, two sort keys and two indices twice, the edge work words, the chunk partials; the vertex arrays are labelcc.hip's
  // (lcc_vtx and the rest of its scratch), the sort pointseg.hip's (ps_*), the rows built for unused voxels refine.hip's chunk.
  DevBuf<uint32_t> lg_nrec, lg_ridx, lg_tkey, lg_ework, lg_meta;
  DevBuf<uint64_t> lg_roff, lg_rkey;
  DevBuf<LgRec> lg_rec;
  DevBuf<LgPart> lg_part;
  DevBuf<uint8_t> lg_tmp;
  DevBuf<int32_t> lg_ab, lg_nodes;
  DevBuf<int64_t> lg_nshared, lg_npairs, lg_nfin;
  DevBuf<double> lg_wsum;
  DevBuf<float> lg_wmin, lg_wmax;
  int64_t lg_E = 0;
  bool lg_valid = false;
  // absorbing the small parts of a caller's per-point labelling (labelabsorb.hip): the labelling of the last vgs_absorb_point_label_parts
  // (la_out, N words), valid until the next one or the next run of the stages (la_valid), and the second labelling the rounds alternate
  // with (la_alt, N words).  Scratch of its own: per part the candidate flag, the target and the run begin | end of its records, per edge
  // of the graph of the parts the sort's keys in | out and values in | out, rocprim's storage, the counter words.  Every round runs
  // labelcc.hip and labelgraph.hip in their own buffers: lcc_valid and lg_valid are false behind the call.
  DevBuf<int32_t> la_out, la_alt, la_target;
  DevBuf<uint8_t> la_cand, la_tmp;
  DevBuf<uint32_t> la_key, la_val, la_run;
  DevBuf<uint64_t> la_cnt;
  bool la_valid = false;
  // a tile context's share of the label graph across the ranks of the tiled driver (labelgraph_tiles.hip; include/vgs.h,
  // vgs_own_point_label_band): the own vertices of the last own pass stay in lcc_vtx (lgt_nv of them) and its band records in lct_bcode /
  // lct_blabel (lgt_band rows) until vgs_own_point_label_graph merges them with the other ranks' records -- the merged vertex arrays node |
  // label | iota, labels | nodes sorted | vertices sorted (merged + 1 words each), the unused flags and their scan (merged + 1 words
  // each); the keys of the merge use lct_key / lct_key2 / lct_val, the partial table is in lg_ab ... lg_wmax (lg_E rows).  lgt_own: an
  // own pass waits for its records; lgt_valid: the partial table is there.  Both are dropped by the next run of the stages.
  DevBuf<uint32_t> lgt_vtx, lgt_flag, lgt_scan;
  uint32_t lgt_nv = 0;
  int64_t lgt_K = 0, lgt_band = 0, lgt_hits = 0;
  bool lgt_own = false, lgt_valid = false;
  // the parts of a labelling across the ranks of the tiled driver (labelcc_tiles.hip; include/vgs.h, vgs_own_point_label_parts): the band
  // records of the last own pass (lct_band rows: code, label, local part, vertex), the code of every local part's first node, the other
  // ranks' records as looked up and sorted (key = label << 32 | local node, value = index of the record), the link triples, the map from
  // local to global part and the own points' global part ids (n_own words).  lct_own / lct_linked / lct_applied: how far the last call got.
  DevBuf<uint64_t> lct_bcode, lct_pcode, lct_fcode, lct_key, lct_key2;
  DevBuf<int32_t> lct_blabel, lct_bpart, lct_flabel, lct_frank, lct_fpart, lct_map, lct_ids;
  DevBuf<uint32_t> lct_bvtx, lct_flag, lct_scan, lct_val, lct_val2, lct_list, lct_count;
  DevBuf<uint32_t> lct_link, lct_link2;   // four words a triple: own part, rank, part, 0
  int64_t lct_band = 0, lct_links = 0, lct_K = 0;
  bool lct_own = false, lct_linked = false, lct_applied = false;
  DevBuf<uint64_t> counters;  // device-side counters (pairs, flags)
  DevBuf<uint32_t> work_ids;   // scratch index lists

  int64_t counts[VGS_N_COUNTS] = {0};
  double times[VGS_T_COUNT] = {0};
  hipEvent_t ev[EV_COUNT] = {nullptr};   // indexed by VgsEvent (counter_words.hpp), which says who records and who waits
  hipEvent_t tev[VGS_T_COUNT][2] = {{nullptr}};   // stage timers: begin / end of every stage, read lazily (capi.hip: timed)
  bool tev_pending[VGS_T_COUNT] = {false};

  // SVGS
  DevBuf<int32_t> sv_label;     // per point: supervoxel label (0 = unassigned), what getLabeledCloud returns (SS:283)
  int32_t sv_max_label = 0;
  bool sv_have_labels = false;
  bool sv_labels_external = false;  // supplied through svgs_set_supervoxel_labels (independent of the VCCS parameters)
  int64_t sv_label_n = -1;          // number of points the labelling was made for
  DevBuf<uint32_t> sv_key_a, sv_key_b;
  DevBuf<uint64_t> cell_code_a, cell_code_b;
  DevBuf<uint32_t> cell_id_a, cell_id_b, cell_start;
  // VCCS-style supervoxel stage
  DevBuf<float> vc_cen, vc_nrm, vc_dist, vc_state;
  DevBuf<int32_t> vc_label;
  DevBuf<uint32_t> vc_tile_start;   // expansion over tiles (vccs.hip): start of every 8^3 tile's run of voxels
  DevBuf<uint32_t> vc_tile_of, vc_tchg;        // vccs_mode 1: tile of every voxel; per tile "a live flag changed in that sweep" (two sweeps' worth)
  DevBuf<int32_t> vc_nbr_tiles;                // vccs_mode 1: the tiles on the 26 sides of a tile ([NT][27], -1: none)
  DevBuf<int32_t> vc_plive;                    // vccs_mode 1: owner << 1 | live of every voxel, swept in place
  DevBuf<uint16_t> vc_cell;                    // a voxel's cell in its tile's 10^3 label array
  DevBuf<unsigned int> vc_ring;   // (vccs_mode 1) the sweeps' change counters of a pass
  DevBuf<unsigned int> vc_dbg;    // (vccs_mode 1, VGS_DEBUG) lanes that moved a voxel, per pass and round
  DevBuf<uint64_t> vc_halo, vc_tile_meta, vc_pool;   // (voxel, cell) of the voxels in the tiles' shells; (offset, length) per tile; entries handed out
  DevBuf<uint64_t> vc_seedkey;
  DevBuf<long long> vc_sums;
  DevBuf<uint32_t> vc_count;
  DevBuf<float> vc_accu;        // vccs_mode 1: 1-ring covariance accumulators (10 floats per voxel)
  DevBuf<uint8_t> vc_alive;   // vccs_mode 1: supervoxel still exists

  // multi-GPU
  bool have_region = false;
  double own_lo[2] = {0, 0}, own_hi[2] = {0, 0};
  DevBuf<uint8_t> owned;        // per voxel: 1 = centre inside this rank's region
  int64_t own_first = 0, n_own = -1;   // points [own_first, own_first + n_own) of the cloud were loaded by this rank itself, the rest came with other ranks' strips (-1: not told)
  DevBuf<uint8_t> mixsrc;       // per voxel: holds own-loaded points / holds points from other ranks' strips
  DevBuf<uint8_t> straddle;     // per voxel: 1 = its cube crosses the border of the region (it may hold points of two ranks)
  DevBuf<uint64_t> bnd_code;    // boundary records
  DevBuf<int32_t> bnd_root;
  DevBuf<int32_t> root_label;   // per voxel id: label of the component rooted there
  DevBuf<uint64_t> bnd_code2;   // compact protocol: unique boundary voxels (code, root, owned count of the root)
  DevBuf<int32_t> bnd_root2, bnd_cnt;
  DevBuf<uint8_t> broot;        // per voxel id: 1 = root named by a boundary record
  int64_t bnd_unique = -1, bnd_kept_local = 0;  // results of the last vgs_get_boundary_roots (-1 = not computed)
};

#define VGS_HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) {                                                                          \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                                \
      if (_e == hipErrorOutOfMemory) { (void)hipGetLastError(); return VGS_E_NOMEM; }                \
      return VGS_E_HIP;                                                                              \
    }                                                                                                \
  } while (0)

// small device -> host read-back through the context's pinned scratch, followed by a wait for the stream
static inline vgs_status vgs_readback(vgs_ctx* c, void* dst, const void* src_dev, size_t bytes) {
  if (bytes > VGS_PIN_BYTES || !c->pin) {
    VGS_HIP_TRY(c, hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VGS_OK;
  }
  VGS_HIP_TRY(c, hipMemcpyAsync(c->pin, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(dst, c->pin, bytes);
  return VGS_OK;
}
// The same on a stream of the caller's choice: only that stream is waited for, whatever else is queued on the others (the merge stage
// reads closestCheck's counters on a side stream while the main stream runs the first unions).  Lower half of the pinned scratch only:
// the upper half may hold a split read-back (below) that has not been collected yet.
static inline vgs_status vgs_readback_on(vgs_ctx* c, hipStream_t s, void* dst, const void* src_dev, size_t bytes) {
  if (bytes > VGS_PIN_SPLIT || !c->pin) {
    VGS_HIP_TRY(c, hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, s));
    VGS_HIP_TRY(c, hipStreamSynchronize(s));
    return VGS_OK;
  }
  VGS_HIP_TRY(c, hipMemcpyAsync(c->pin, src_dev, bytes, hipMemcpyDeviceToHost, s));
  VGS_HIP_TRY(c, hipStreamSynchronize(s));
  memcpy(dst, c->pin, bytes);
  return VGS_OK;
}
// Optional outputs of a getter: one column is the host destination (NULL: not wanted), its rows in HBM and the bytes of a row.
// vgs_copy_rows copies n_rows rows of every wanted column and waits for the stream once.
struct RowCol { void* dst; const void* src; size_t row_bytes; };
static inline vgs_status vgs_copy_rows(vgs_ctx* c, size_t n_rows, const RowCol* col, int n_col) {
  for (int i = 0; i < n_col; ++i)
    if (col[i].dst) VGS_HIP_TRY(c, hipMemcpyAsync(col[i].dst, col[i].src, n_rows * col[i].row_bytes, hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGS_OK;
}
// Longest row of connect bits the kernels hold in LDS: 624 words = a cube of 27 cells a side = balls of up to 13 voxels (the edge list of
// the smallest one-wavefront class, 312 keys of 8 bytes, is where its row is put together).  Wider balls (up to the engine's own limit
// of graph_size / voxel_size = 12 ... 15 by rounding) keep crossValidation's search in the neighbour's row.  (Round 4: 256 words, 9 voxels --
// config 2's ball of ten fell back silently.)
#define VGS_CB_MAX_WORDS 624
// bit of the lattice offset p (packed (dx+16) | (dy+16) << 5 | (dz+16) << 10, as the rows' adj_off holds it) in a row of connect bits
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t vgs_cb_index(uint32_t p, int R) {
  const int D = 2 * R + 1;
  const int dx = (int)(p & 31u) - 16 + R, dy = (int)((p >> 5) & 31u) - 16 + R, dz = (int)((p >> 10) & 31u) - 16 + R;
  return (uint32_t)((dz * D + dy) * D + dx);
}
#endif
#define VGS_READBACK(ctx, dst, src, bytes) do { vgs_status _s = vgs_readback((ctx), (dst), (src), (bytes)); if (_s != VGS_OK) return _s; } while (0)
#define VGS_READBACK_ON(ctx, s, dst, src, bytes) do { vgs_status _s = vgs_readback_on((ctx), (s), (dst), (src), (bytes)); if (_s != VGS_OK) return _s; } while (0)

// The same in two halves (round 4): the copy is queued NOW, the host collects it LATER.  Kernels launched in between that do not need
// the number run while the host makes its round trip (20-30 us of an idle GPU per read-back otherwise: profiles/r04_step_timeline.txt).
// Uses the upper half of the pinned scratch, so that a plain vgs_readback in between does not overwrite it.
static inline vgs_status vgs_readback_begin(vgs_ctx* c, const void* src_dev, size_t bytes) {
  if (bytes > VGS_PIN_BYTES - VGS_PIN_SPLIT || !c->pin || !c->ev_rb) return VGS_E_ARG;
  VGS_HIP_TRY(c, hipMemcpyAsync((char*)c->pin + VGS_PIN_SPLIT, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipEventRecord(c->ev_rb, c->stream));
  return VGS_OK;
}
static inline vgs_status vgs_readback_end(vgs_ctx* c, void* dst, size_t bytes) {
  VGS_HIP_TRY(c, hipEventSynchronize(c->ev_rb));
  memcpy(dst, (char*)c->pin + VGS_PIN_SPLIT, bytes);
  return VGS_OK;
}
static inline bool vgs_can_split_readback(const vgs_ctx* c) { return c->pin != nullptr && c->ev_rb != nullptr; }

// Front fork: the main stream waits for what stream2 carries (the gather, k_features); nothing is queued on stream2 behind it until the
// local cut.  vgs_front_abandon is the same for a stage sequence that is cut short (an error, an early return): the host waits, so that
// the next cloud cannot overwrite perm_b, xs/ys/zs or node under a running kernel.
static inline vgs_status vgs_front_join(vgs_ctx* c) {
  if (!c->ff_open) return VGS_OK;
  VGS_HIP_TRY(c, hipEventRecord(c->ev_ff_join, c->stream2));   // (on an error ff_open stays set: the caller abandons)
  VGS_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_ff_join, 0));
  c->ff_open = false;
  return VGS_OK;
}
static inline void vgs_front_abandon(vgs_ctx* c) {
  if (!c->ff_open) return;
  c->ff_open = false;
  (void)hipStreamSynchronize(c->stream2);
}

// The decomposition of the per-segment passes (segdesc.hip, segbox.hip, segfield.hip): chunks of SD_CHUNK virtual points that never cross a segment.
// sd_prepare (segdesc.hip) runs steps 1-2 of segdesc.hip's header for labels 0 .. K-1 -- sorted node ids, virtual positions, per segment
// its first sorted node and first chunk, pointers into the sd_* scratch -- and gives the grid bound of the chunk kernels.
#define SD_TB 256                   // threads of a chunk workgroup
#define SD_PPT 8                    // points per thread of a chunk
#define SD_CHUNK (SD_TB * SD_PPT)   // virtual points per chunk
struct SdPrep { uint32_t *ids, *vp, *seg_node, *seg_chunk; int64_t n_chunks_max; };
vgs_status sd_prepare(vgs_ctx* c, int64_t K, SdPrep& o);
// tile contexts: the first own point of every label of that decomposition, in the chunks' order, into sd_apos (segdesc.hip: k_sd_own_anchor)
vgs_status sd_own_anchor(vgs_ctx* c, int64_t K, const SdPrep& P);
// a tile context (the tiled driver, include/vgs_tiles.h) holds only part of its segments: the per-segment getters of one context refuse it
static inline bool vgs_is_tile(const vgs_ctx* c) { return c->have_region || c->n_own >= 0; }
#ifdef __HIPCC__
// position of the voxel with code q in vox_code (sorted, descending); V when the context does not hold it
__device__ __forceinline__ int64_t vgs_find_voxel(const uint64_t* __restrict__ vox_code, int64_t V, uint64_t q) {
  int64_t lo = 0, hi = V;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (vox_code[mid] > q) lo = mid + 1; else hi = mid; }
  return (lo < V && vox_code[lo] == q) ? lo : V;
}
// The walk of a chunk workgroup (blockIdx.x) from chunk to segment to nodes, one copy for segdesc.hip, segbox.hip and segfield.hip: the
// segment k of the chunk, its virtual range [a, b) and its m nodes staged in s_vp (virtual start of each node) and s_dl (sorted position -
// virtual position, mod 2^32), two LDS arrays of SD_CHUNK words.  False, with nothing staged, for a workgroup past the real number of
// chunks (k = 0xffffffff: nothing to write) and for an empty chunk (cannot happen for a kept segment; the caller writes an empty record so
// that the fold stays well defined).  The caller's __syncthreads follows; then sd_pos gives the sorted position of a virtual point.
struct SdChunk { uint32_t k, n0, a, b, m; };
__device__ __forceinline__ bool sd_walk(const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ vp,
                                        const uint32_t* __restrict__ seg_node, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                        uint32_t* __restrict__ s_vp, uint32_t* __restrict__ s_dl, SdChunk& o) {
  const uint32_t c = blockIdx.x;
  o.k = 0xffffffffu;
  if (c >= seg_chunk[K]) return false;
  // segment of chunk c: the last k with seg_chunk[k] <= c (every segment has at least one chunk)
  uint32_t lo = 0, hi = K - 1;
  while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (seg_chunk[mid] <= c) lo = mid; else hi = mid - 1; }
  const uint32_t k = lo;
  o.k = k;
  const uint32_t n0 = seg_node[k], n1 = seg_node[k + 1];
  const uint32_t a = vp[n0] + (c - seg_chunk[k]) * SD_CHUNK;
  const uint32_t b = min(a + SD_CHUNK, vp[n1]);
  if (n1 <= n0 || a >= b) return false;
  // nodes that overlap [a, b): the last node starting at or before a ... the last node starting before b.  Every node of a kept segment
  // holds a point, so vp rises strictly inside the segment and they are at most b - a <= SD_CHUNK nodes.
  uint32_t i0 = n0, i1 = n1 - 1;
  while (i0 < i1) { const uint32_t mid = (i0 + i1 + 1) >> 1; if (vp[mid] <= a) i0 = mid; else i1 = mid - 1; }
  uint32_t j0 = i0 + 1, j1 = n1;
  while (j0 < j1) { const uint32_t mid = (j0 + j1) >> 1; if (vp[mid] < b) j0 = mid + 1; else j1 = mid; }
  const uint32_t m = min(j0 - i0, (uint32_t)SD_CHUNK);   // (the bound above; the clamp only guards the LDS arrays)
  for (uint32_t t = threadIdx.x; t < m; t += SD_TB) {
    const uint32_t i = i0 + t, q = vp[i];
    s_vp[t] = q;
    s_dl[t] = vox_start[ids[i]] - q;
  }
  o.n0 = n0; o.a = a; o.b = b; o.m = m;
  return true;
}
// sorted position of the virtual point q of the chunk: the last staged node that starts at or before q
__device__ __forceinline__ uint32_t sd_pos(const uint32_t* __restrict__ s_vp, const uint32_t* __restrict__ s_dl, uint32_t m, uint32_t q) {
  uint32_t l = 0, h = m - 1;
  while (l < h) { const uint32_t mid = (l + h + 1) >> 1; if (s_vp[mid] <= q) l = mid; else h = mid - 1; }
  return q + s_dl[l];
}
#endif

vgs_status vgs_cut_order(vgs_ctx* c, std::vector<uint16_t>& ord_host, std::vector<uint32_t>& k_host, bool want_lists = false,
                         const uint8_t* list_flag = nullptr, std::vector<uint32_t>* list_cnt = nullptr, std::vector<int32_t>* list_ids = nullptr);   // cutorder.hip
void vgs_read_env_knobs(vgs_ctx* c);   // capi.hip; called by vgs_create only

// stage implementations (one .hip file each)
vgs_status vgs_stage_voxelize(vgs_ctx* c);
vgs_status vgs_front_fork(vgs_ctx* c);   // voxelize.hip: the gather of the points goes to stream2 (vgs_run's front fork)
vgs_status vgs_stage_features(vgs_ctx* c);
vgs_status vgs_stage_adjacency(vgs_ctx* c);
vgs_status vgs_run_adjacency(vgs_ctx* c, bool full, uint64_t* out_key, uint32_t* out_cnt, uint32_t* out_nall, float r2, const uint32_t* ids = nullptr,
                             int64_t n_ids = 0);
bool vgs_unused_are_inert(const vgs_params& p);
vgs_status vgs_stage_nearlists(vgs_ctx* c);   // part of the local-cut stage
vgs_status vgs_pairlists_begin(vgs_ctx* c, hipStream_t strm);   // pairlist.hip, part of the local-cut stage
vgs_status vgs_pairlists_build(vgs_ctx* c, hipStream_t strm, const uint32_t* const* ids, const unsigned int* const* n_dev, const unsigned int* n_host,
                               int n_lists, bool all_rows, const float* ctab, float ctab_scale, float d2_stop, int slot, const LcGate& gate,
                               bool big_rows_too);
vgs_status vgs_stage_localcut(vgs_ctx* c);   // launches everything; its hand-over kernels may still run when it returns
vgs_status vgs_ensure_point_labels(vgs_ctx* c);   // merge.hip
vgs_status vgs_localcut_finish_queue(vgs_ctx* c, hipStream_t s);  // queues the finish's waits and read-back on stream s without waiting (optional; the finish collects it)
vgs_status vgs_localcut_finish(vgs_ctx* c, hipStream_t s, unsigned int* n_deferred);  // waits for them on stream s, checks the stage's flags (called by the merge stage)
vgs_status vgs_stage_merge(vgs_ctx* c);
vgs_status vgs_clusters_on_device(vgs_ctx* c);   // clusters.hip
vgs_status vgs_segdesc_on_device(vgs_ctx* c);    // segdesc.hip
vgs_status vgs_segbox_on_device(vgs_ctx* c, int frame);   // segbox.hip
// k_sb_frames over K rows of evecs9 / cov6 in HBM, left on the context's stream: the frame rule's one launch site (segbox.hip)
void sb_launch_frames(vgs_ctx* c, const double* evec, const double* cov, int64_t K, int frame, double* out);
// tile contexts (segbox.hip; pointseg.hip runs them over a caller's labelling): K rows of the global descriptor table from the host into
// sbt_in and their frames into sbt_frame; k_sb_final over chunk partials into sbt_out (lo3 | hi3 | half3 | center3)
vgs_status sbt_upload_frames(vgs_ctx* c, int64_t K, int32_t frame, const double* centroid3, const double* cov6, const double* evecs9);
void sbt_launch_final(vgs_ctx* c, int64_t K, const uint32_t* seg_chunk, const double* part, uint32_t n_part);
// a caller's per-point labelling (pointseg.hip): VGS_E_ARG, the message naming the first index and its value, if a label is not below K
// (one pass on the device); and the host variants' upload into ps_in (*labels_dev = nullptr for n = 0)
vgs_status vgs_check_label_range(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t n, int64_t K);
vgs_status vgs_upload_point_labels(vgs_ctx* c, const int32_t* labels_host, int64_t n, const int32_t** labels_dev);
// steps 1-3 of pointseg.hip's header: the octree points that carry a label 0 .. K-1 sorted by label (pos: sorted positions, a label's run ascending), per label the start of its
// run (seg_start, K + 1 words) and its first chunk (seg_chunk, K + 1 words), in the ps_* scratch and left on the stream; the grid bound of
// the chunk kernels.  sorted = false (nothing queued behind the range check) for K = 0.  pointfield.hip runs its kernels over the same sort
struct PsSort { bool sorted; uint32_t *key, *pos, *seg_start, *seg_chunk; int64_t n_chunks_max; };
vgs_status ps_sort_points(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t own_first, int64_t n_lab, int64_t K, size_t tmp_extra,
                          int64_t* n_skipped, PsSort& S);
// the folds of segfield.hip for pointfield.hip: k_sf_final over the chunk partials of one channel group (seg_chunk: K + 1 first chunks),
// k_sf_own_records over the same for a tile context (raw n, S1, S2, min, max), k_sf_majority over a K x n_classes table; left on the
// context's stream
void sf_launch_own_records(vgs_ctx* c, const uint32_t* seg_chunk, const double* part, uint32_t n_part, int64_t K, uint32_t C, uint32_t c0, uint32_t ng,
                           int64_t* o_n, double* o_s1, double* o_s2, float* o_min, float* o_max);
void sf_launch_final(vgs_ctx* c, const uint32_t* seg_chunk, const double* part, uint32_t n_part, int64_t K, uint32_t C, uint32_t c0, uint32_t ng,
                     const double* anchor, int64_t* o_n, double* o_mean, double* o_var, float* o_min, float* o_max);
void sf_launch_majority(vgs_ctx* c, const int64_t* hist, int32_t n_classes, int64_t K, int32_t* majority, int64_t* majority_count);
// labelcc.hip's pass over the points own_first .. own_first + n_lab - 1 (labelcc_tiles.hip runs it over a tile context's own points)
vgs_status vgs_label_parts_on_device(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t own_first, int64_t n_lab, int64_t K, int64_t* n_parts,
                                     int64_t* n_skipped);
// its steps 1 and 2, shared with labelgraph.hip: the sort and the vertex arrays (nv + 1 words each, in lcc_vtx), in (label, node) order
struct LcVtx { uint32_t *node, *label, *q, *parent, *root, *part; };
vgs_status vgs_label_vertices_on_device(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t own_first, int64_t n_lab, int64_t K,
                                        int64_t* n_skipped, PsSort& S, uint32_t* n_vertices, LcVtx& X);
// labelgraph.hip behind the vertex list, for labelgraph_tiles.hip: what the row kernels need besides the rows, and where the records go;
// step 2 (the vertices X by node: fills G); steps 3 to 6 behind a walk of the caller's -- walk(write = false) counts the records of
// every vertex into lg_nrec, walk(write = true) writes them -- into lg_ab ... lg_wmax, lg_E rows, the stream waited for
struct LgWalk {
  uint32_t nv, K, R;
  const uint32_t *snode, *slab, *nbeg, *nend;
  VgsWeightParams W;
  uint64_t* rkey;
  uint32_t *tkey, *ridx;
};
typedef vgs_status (*LgWalkFn)(vgs_ctx* c, const LgWalk& G, bool write, void* arg);
vgs_status vgs_lg_vertices_by_node(vgs_ctx* c, const LcVtx& X, uint32_t nv, int64_t K, LgWalk& G);
vgs_status vgs_lg_table_from_walk(vgs_ctx* c, const char* fn, LgWalk& G, LgWalkFn walk, void* arg);
// labelcc_tiles.hip's band and lookup steps, for labelgraph_tiles.hip: the band records of nv vertices (code, label, vpart[vertex],
// vertex) into lct_bcode / lct_blabel / lct_bpart / lct_bvtx (vpart == nullptr: the first two only), the stream waited for; n records (code, label) in HBM looked up in the
// local grid, key[k] = label << 32 | node or all ones, val[k] = k, counts[0] += hits, left on the stream
vgs_status vgs_lt_band_on_device(vgs_ctx* c, const uint32_t* vnode, const uint32_t* vlabel, const uint32_t* vpart, uint32_t nv, uint32_t* n_band);
vgs_status vgs_lt_find_on_device(vgs_ctx* c, const uint64_t* code_dev, const int32_t* label_dev, int64_t n, uint64_t* key, uint32_t* val,
                                 unsigned long long* counts);
vgs_status vgs_seggraph_on_device(vgs_ctx* c);   // seggraph.hip
// tile contexts: halo[v] = label[k] for the voxel v of code[k] that this context holds and does not own, queued on the context's stream
// (code, label: n entries in HBM; halo: V entries).  One kernel for the graph's table and the refinement's (seggraph.hip)
vgs_status vgs_halo_find(vgs_ctx* c, const uint64_t* code_dev, const int32_t* label_dev, int64_t n, int32_t* halo_dev);
vgs_status vgs_refine_on_device(vgs_ctx* c, const vgs_refine_params& rp, int64_t* counts4);   // refine.hip
vgs_status vgs_refine_own_on_device(vgs_ctx* c, const vgs_refine_params& rp, int64_t* counts5);   // refine.hip, tile contexts
vgs_status vgs_stage_vccs(vgs_ctx* c);
vgs_status vgs_stage_svgs_group(vgs_ctx* c);
vgs_status vgs_stage_svgs_neighbours(vgs_ctx* c);
vgs_status vgs_grow_box_from(vgs_ctx* c, OctreeBox& box, bool record_epochs);
vgs_status vgs_compute_owned(vgs_ctx* c);

#endif
