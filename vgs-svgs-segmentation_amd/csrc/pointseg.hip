// pointseg.hip -- descriptors and oriented boxes of a per-POINT labelling of the context's cloud that the CALLER supplies (include/vgs.h:
// vgs_point_label_descriptors, vgs_point_label_boxes): the refined labels, ground-truth instances, anything made from the engine's output.
// The passes of segdesc.hip / segbox.hip sort V nodes by label and walk each node's run of points, so they can only describe a labelling
// that is constant on a node; here the points themselves are sorted.  Row k covers the points i with labels[i] == k that xs/ys/zs hold
// (the finite points, the ones in the octree); the row fields, the algebra and the frame rule are those of the two node passes.
//
// Data flow (the points sit in HBM in leaf order, perm_b gives the input index of a sorted position, pt_vox its node):
//   1. k_ps_keys      for every sorted position pos < N: l = labels[perm[pos]]; pos < Nf: key = l if 0 <= l < K, else K, value = pos;
//                     pos >= Nf (a point outside the octree) with l >= 0: counted as skipped; l >= K anywhere: the smallest such input
//                     index is kept (one atomicMax of N - i per workgroup that saw one)                                 -> read-back
//   2. one STABLE rocprim::radix_sort_pairs over the bits of K -> pos_sorted: a label's points are one run, positions ascending inside it
//   3. k_ps_segments  one lower bound per k: the run's start; ceil(points / SD_CHUNK) chunks, none for a label without a point; exclusive
//                     scan -> the first chunk of every label.  The chunk grid is the bound Nf / SD_CHUNK + min(K, Nf) + 1 (only a label
//                     with a point has a ragged last chunk), launched without reading the real number back
//   4. k_ps_chunks    one workgroup per chunk: the point of a lane is pos_sorted[a + it * SD_TB + tid], the anchor the label's first point
//                     in that order, the partial record sd_chunk_sums' (segpass.hpp, the body k_sd_chunks runs); and the number of head
//                     flags pt_vox[pos_sorted[q]] != pt_vox[pos_sorted[q - 1]] of the chunk, whose sum over a label is its n_nodes
//   5. k_ps_final     one wavefront per label: sd_fold_partials, the head flags added, sd_segment_algebra -- the one copy of the algebra
//   6. boxes: k_sb_frames (segbox.hip) over the rows of step 5, k_ps_box_chunks with sb_chunk_extents over the same pos_sorted,
//      k_ps_box_final with the fold and the row of k_sb_final
// A label no point carries: no chunk, so the folds are empty: n_points = n_nodes = 0, bbox6 = (+inf x3, -inf x3), a zero anchor and zero
// sums (zero centroid, covariance and eigenvalues, identity eigenvectors, the features of zeros); its box is lo = hi = half = 0 and
// center = centroid, the rule of vgs_segment_boxes_from_extents.
// Why a sort and not atomics: fp64 sums by atomics depend on the order of arrival.  Sorted, every sum has a fixed shape -- which point a
// lane reads depends on (chunk, lane, step) only -- so the tables are bit-identical from call to call and engine to engine.  And for a
// labelling that is constant on nodes, a stable sort of the positions by label gives the very point sequence sd_prepare's virtual order
// gives (nodes in ascending id, each node's run in order), hence the same chunks and the same anchor: handed the engine's own point
// labels, this pass reproduces the cached tables of segdesc.hip and segbox.hip byte for byte.
// Scratch, all in buffers of its own (ps_*; nothing a getter or a cached table reads): two key and two value arrays of Nf words = 16 B
// per finite point, rocprim's sort storage, 3 (K + 1) words of label starts and chunk counts, one partial record and one word per chunk,
// the K output rows, and N words for the labels of the host variants.  Nothing is cached: the input is the caller's.
// Tile contexts (the tiled driver, include/vgs_tiles.h; the entry points at the end of this file): the same steps over the rank's OWN
// points only -- step 1 gives every other position the key K -- with the moment record of k_sd_own_records in place of the row
// (k_ps_own_records), and the head flags of voxels that hold another rank's points too (k_ps_shared) sent as pair records (k_ps_pairs)
// instead of counted (k_ps_own_chunks), so that the driver counts such a voxel once over all ranks.
#include <string.h>

#include <algorithm>
#include <string>

#include <rocprim/rocprim.hpp>

#include "segpass.hpp"

typedef unsigned long long ps_u64;
enum { PM_SKIPPED = 0, PM_BAD = 1, PM_SLOTS = 2 };   // slots of ps_meta
#define PS_TB 256

// Step 1.  perm == nullptr: the identity (a cloud without a finite point has no order).  key == nullptr: the range check alone.
// labels holds n_lab entries, labels[j] for the input index own_first + j (one context: own_first = 0, n_lab = N; a tile context: its own
// point range).  An input index outside that range has no label: its position gets the key K and counts nowhere.
__global__ __launch_bounds__(PS_TB) void k_ps_keys(const int32_t* __restrict__ labels, const uint32_t* __restrict__ perm, int64_t N, int64_t nf,
                                                   int64_t own_first, int64_t n_lab, uint32_t K, uint32_t* __restrict__ key,
                                                   uint32_t* __restrict__ val, ps_u64* __restrict__ meta) {
  __shared__ ps_u64 s_sk[PS_TB / 64], s_bad[PS_TB / 64];
  const int64_t pos = (int64_t)blockIdx.x * PS_TB + threadIdx.x;
  ps_u64 sk = 0, bad = 0;
  if (pos < N) {
    const int64_t j = (perm ? (int64_t)perm[pos] : pos) - own_first;
    const int32_t l = (j >= 0 && j < n_lab) ? labels[j] : -1;
    const bool over = l >= 0 && (uint32_t)l >= K;
    if (over) bad = (ps_u64)(n_lab - j);   // (the largest n_lab - j is the first offending index)
    if (pos < nf) {
      if (key) { key[pos] = (l < 0 || over) ? K : (uint32_t)l; val[pos] = (uint32_t)pos; }
    } else if (l >= 0) {
      sk = 1;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sk += __shfl_xor(sk, m, 64);
    const ps_u64 o = __shfl_xor(bad, m, 64); bad = o > bad ? o : bad;
  }
  if ((threadIdx.x & 63) == 0) { s_sk[threadIdx.x >> 6] = sk; s_bad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x != 0) return;   // at most two atomics per workgroup
  for (int w = 1; w < PS_TB / 64; ++w) { sk += s_sk[w]; bad = s_bad[w] > bad ? s_bad[w] : bad; }
  if (sk) atomicAdd(&meta[PM_SKIPPED], sk);
  if (bad) atomicMax(&meta[PM_BAD], bad);
}

// Step 3.  Per label k < K: the start of its run in the sorted keys (seg_start[K] = the end of the labelled points) and its number of
// chunks, 0 for a label without a point (nchunk[K] = 0).
__global__ __launch_bounds__(PS_TB) void k_ps_segments(const uint32_t* __restrict__ key, uint32_t n, uint32_t K, uint32_t* __restrict__ seg_start,
                                                       uint32_t* __restrict__ nchunk) {
  const uint64_t k64 = (uint64_t)blockIdx.x * PS_TB + threadIdx.x;
  if (k64 > (uint64_t)K) return;
  const uint32_t k = (uint32_t)k64;
  const uint32_t n0 = sd_lower_bound(key, n, k);
  seg_start[k] = n0;
  if (k == K) { nchunk[k] = 0; return; }
  const uint32_t n1 = sd_lower_bound(key, n, k + 1);
  nchunk[k] = (n1 - n0 + SD_CHUNK - 1) / SD_CHUNK;
}

// Step 4.  Grid: the bound of the header; workgroups past the real number of chunks leave at once (whole workgroups, before any barrier).
// TILE (k_ps_own_chunks, tile contexts): pos_sorted holds the rank's own labelled points only.  A head flag in a voxel that other ranks'
// points share (shared[v], k_ps_shared) is not counted: it is written to flag[q] and leaves as a pair record (k_ps_pairs), so that the
// driver counts the voxel once over all ranks.  flag[q] is written for every point of every chunk.
template <bool TILE>
__device__ __forceinline__ void ps_chunk_body(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                              const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ pt_vox,
                                              const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                              double* __restrict__ part, uint32_t* __restrict__ nn_part, const uint8_t* __restrict__ shared,
                                              uint32_t* __restrict__ flag) {
  __shared__ uint32_t s_nn[SD_TB / 64];
  PsChunk wk;
  if (!ps_walk(seg_start, seg_chunk, K, wk)) return;
  const uint32_t c = blockIdx.x;
  // the anchor: the label's first point in the sorted order, the same for every chunk of the label
  const uint32_t pa = pos_sorted[wk.s0];
  const double ax = (double)xs[pa], ay = (double)ys[pa], az = (double)zs[pa];
  sd_chunk_sums<false>(xs, ys, zs, wk.a, wk.b, ax, ay, az, [&](uint32_t q) { return pos_sorted[q]; }, part + (size_t)c * SD_REC, nullptr, 0, 0);
  // distinct nodes: inside a label the positions ascend, so a node's points are adjacent and its first one carries the flag
  uint32_t heads = 0;
#pragma unroll 2
  for (int it = 0; it < SD_PPT; ++it) {
    const uint32_t q = wk.a + (uint32_t)it * SD_TB + threadIdx.x;
    if (q < wk.b) {
      const uint32_t v = pt_vox[pos_sorted[q]];
      const bool head = q == wk.s0 || v != pt_vox[pos_sorted[q - 1]];
      if (TILE) {
        const bool sh = head && shared[v] != 0;
        flag[q] = sh ? 1u : 0u;
        heads += (head && !sh) ? 1u : 0u;
      } else {
        heads += head ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) heads += __shfl_xor(heads, m, 64);
  if ((threadIdx.x & 63) == 0) s_nn[threadIdx.x >> 6] = heads;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t v = s_nn[0];
    for (int u = 1; u < SD_TB / 64; ++u) v += s_nn[u];
    nn_part[c] = v;
  }
}

__global__ __launch_bounds__(SD_TB) void k_ps_chunks(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                     const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ pt_vox,
                                                     const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                                     double* __restrict__ part, uint32_t* __restrict__ nn_part) {
  ps_chunk_body<false>(xs, ys, zs, pos_sorted, pt_vox, seg_start, seg_chunk, K, part, nn_part, nullptr, nullptr);
}

__global__ __launch_bounds__(SD_TB) void k_ps_own_chunks(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                         const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ pt_vox,
                                                         const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                                         double* __restrict__ part, uint32_t* __restrict__ nn_part,
                                                         const uint8_t* __restrict__ shared, uint32_t* __restrict__ flag) {
  ps_chunk_body<true>(xs, ys, zs, pos_sorted, pt_vox, seg_start, seg_chunk, K, part, nn_part, shared, flag);
}

// Tile contexts.  shared[v] = 1 for a voxel whose run of points in this context holds at least one own point and at least one point of
// another rank: such a run has two neighbours of different kind, and the later one of every such pair stores the flag -- plain stores of 1
// into a zeroed table, no atomics.
__global__ __launch_bounds__(PS_TB) void k_ps_shared(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pt_vox, int64_t nf,
                                                     int64_t own_first, int64_t own_end, uint8_t* __restrict__ shared) {
  const int64_t pos = (int64_t)blockIdx.x * PS_TB + threadIdx.x;
  if (pos < 1 || pos >= nf) return;
  const uint32_t v = pt_vox[pos];
  if (pt_vox[pos - 1] != v) return;
  const int64_t a = (int64_t)perm[pos], b = (int64_t)perm[pos - 1];
  if ((a >= own_first && a < own_end) != (b >= own_first && b < own_end)) shared[v] = 1;
}

// Tile contexts.  The pair records in sorted order: the flagged point q (flag, its inclusive scan inc) writes record inc[q] - 1 -- the code
// of its voxel and its label.  The order is that of the sort (label ascending, position ascending), never that of arrival.
__global__ __launch_bounds__(PS_TB) void k_ps_pairs(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ inc, const uint32_t* __restrict__ key,
                                                    const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ pt_vox,
                                                    const uint64_t* __restrict__ vox_code, int64_t n, uint64_t* __restrict__ pair_code,
                                                    int32_t* __restrict__ pair_label) {
  const int64_t q = (int64_t)blockIdx.x * PS_TB + threadIdx.x;
  if (q >= n || !flag[q]) return;
  const uint32_t o = inc[q] - 1;
  pair_code[o] = vox_code[pt_vox[pos_sorted[q]]];
  pair_label[o] = (int32_t)key[q];
}

// Step 5.  One wavefront per label: fold its partials (lane stride, then butterfly), then everything per label on lane 0.  REC
// (k_ps_own_records, tile contexts): the folded moments leave as the label's record of SD_MREC doubles, the layout of k_sd_own_records --
// points, unshared head flags, min[3], max[3], anchor[3] (0 without a point), sum d[3], sum d d^T[6] -- instead of a row of the table.
template <bool REC>
__device__ __forceinline__ void ps_final_body(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                              const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ seg_start,
                                              const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part,
                                              const uint32_t* __restrict__ nn_part, uint32_t n_part, uint32_t K, int svgs,
                                              int64_t* __restrict__ o_npts, int32_t* __restrict__ o_nnodes, float* __restrict__ o_bbox,
                                              double* __restrict__ o_cen, double* __restrict__ o_cov, double* __restrict__ o_eval,
                                              double* __restrict__ o_evec, float* __restrict__ o_eig8, double* __restrict__ mom) {
  const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= K) return;   // (whole wavefronts; no barrier follows)
  const uint32_t c0 = seg_chunk[k], c1 = min(seg_chunk[k + 1], n_part);   // (the bound only guards the records: the chunks fit, see the launch)
  // the head flags first; their sum waits in LDS, one word per wavefront, so that the fold below keeps k_sd_final's register budget
  __shared__ uint32_t s_nn[4];
  uint32_t nn = 0;
  for (uint32_t c = c0 + lane; c < c1; c += 64) nn += nn_part[c];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) nn += __shfl_xor(nn, m, 64);
  if (lane == 0) s_nn[threadIdx.x >> 6] = nn;
  double s[9], mn[3], mx[3], cnt;
  sd_fold_partials<false>(part, c0, c1, lane, s, mn, mx, cnt);
  if (lane != 0) return;
  nn = s_nn[threadIdx.x >> 6];   // (written by this lane: no barrier)
  const uint32_t s0 = seg_start[k], n = seg_start[k + 1] - s0;
  double anc[3] = {0.0, 0.0, 0.0};   // (a label without a point: a zero anchor)
  if (n > 0) {
    const uint32_t pa = pos_sorted[s0];
    anc[0] = (double)xs[pa]; anc[1] = (double)ys[pa]; anc[2] = (double)zs[pa];
  }
  if (REC) {
    double* r = mom + (size_t)k * SD_MREC;
    r[0] = (double)n;
    r[1] = (double)nn;
#pragma unroll
    for (int f = 0; f < 3; ++f) { r[2 + f] = mn[f]; r[5 + f] = mx[f]; r[8 + f] = anc[f]; }
#pragma unroll
    for (int f = 0; f < 9; ++f) r[11 + f] = s[f];
  } else {
    sd_segment_algebra(k, (int64_t)n, (int32_t)nn, mn, mx, anc, s, svgs, o_npts, o_nnodes, o_bbox, o_cen, o_cov, o_eval, o_evec, o_eig8);
  }
}

__global__ __launch_bounds__(256) void k_ps_final(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                  const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ seg_start,
                                                  const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part,
                                                  const uint32_t* __restrict__ nn_part, uint32_t n_part, uint32_t K, int svgs,
                                                  int64_t* __restrict__ o_npts, int32_t* __restrict__ o_nnodes, float* __restrict__ o_bbox,
                                                  double* __restrict__ o_cen, double* __restrict__ o_cov, double* __restrict__ o_eval,
                                                  double* __restrict__ o_evec, float* __restrict__ o_eig8) {
  ps_final_body<false>(xs, ys, zs, pos_sorted, seg_start, seg_chunk, part, nn_part, n_part, K, svgs, o_npts, o_nnodes, o_bbox, o_cen, o_cov, o_eval,
                       o_evec, o_eig8, nullptr);
}

__global__ __launch_bounds__(256) void k_ps_own_records(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                        const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ seg_start,
                                                        const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part,
                                                        const uint32_t* __restrict__ nn_part, uint32_t n_part, uint32_t K,
                                                        double* __restrict__ mom) {
  ps_final_body<true>(xs, ys, zs, pos_sorted, seg_start, seg_chunk, part, nn_part, n_part, K, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr, mom);
}

// Step 6.  The chunks of step 4 once more, projected onto the frame of their label about its centroid.
__global__ __launch_bounds__(SD_TB) void k_ps_box_chunks(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                         const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ seg_start,
                                                         const uint32_t* __restrict__ seg_chunk, uint32_t K, const double* __restrict__ cen,
                                                         const double* __restrict__ frame, double* __restrict__ part) {
  PsChunk wk;
  if (!ps_walk(seg_start, seg_chunk, K, wk)) return;
  sb_chunk_extents<false>(xs, ys, zs, wk.a, wk.b, cen + (size_t)wk.k * 3, frame + (size_t)wk.k * 9, [&](uint32_t q) { return pos_sorted[q]; },
                          part + (size_t)blockIdx.x * SB_REC, nullptr, 0, 0);
}

__global__ __launch_bounds__(256) void k_ps_box_final(const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part, uint32_t n_part,
                                                      uint32_t K, const double* __restrict__ cen, const double* __restrict__ frame,
                                                      double* __restrict__ o_lo, double* __restrict__ o_hi, double* __restrict__ o_half,
                                                      double* __restrict__ o_center) {
  const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= K) return;   // (whole wavefronts; no barrier follows)
  const uint32_t c0 = seg_chunk[k], c1 = min(seg_chunk[k + 1], n_part);
  double mn[3], mx[3];
  sb_fold_partials(part, c0, c1, lane, mn, mx);
  if (lane != 0) return;
  if (c0 >= c1) {   // a label without a point: lo = hi = 0, so half = 0 and center = centroid plus a zero
#pragma unroll
    for (int f = 0; f < 3; ++f) { mn[f] = 0.0; mx[f] = 0.0; }
  }
  sb_box_row(k, mn, mx, cen, frame, o_lo, o_hi, o_half, o_center);
}

// ---------------------------------------------------------------------------------------------------------------------- host
// Step 1 alone or with the keys: the first input index whose label is not below K fails the call, the message naming it and its value.
// labels_dev: n_lab entries for the input indices own_first .. own_first + n_lab - 1 (k_ps_keys); the index of the message is the caller's.
static vgs_status ps_scan_labels(vgs_ctx* c, const char* fn, const int32_t* labels_dev, const uint32_t* perm, int64_t N, int64_t nf, int64_t own_first,
                                 int64_t n_lab, int64_t K, uint32_t* key, uint32_t* val, int64_t* n_skipped) {
  if (n_skipped) *n_skipped = 0;
  if (N == 0) return VGS_OK;
  VGS_HIP_TRY(c, c->ps_meta.ensure(PM_SLOTS));
  ps_u64* meta = (ps_u64*)c->ps_meta.p;
  VGS_HIP_TRY(c, hipMemsetAsync(meta, 0, PM_SLOTS * sizeof(uint64_t), c->stream));
  hipLaunchKernelGGL(k_ps_keys, dim3((unsigned)((N + PS_TB - 1) / PS_TB)), dim3(PS_TB), 0, c->stream, labels_dev, perm, N, nf, own_first, n_lab, (uint32_t)K,
                     key, val, meta);
  VGS_HIP_TRY(c, hipGetLastError());
  uint64_t m[PM_SLOTS];
  VGS_READBACK(c, m, meta, PM_SLOTS * sizeof(uint64_t));
  if (m[PM_BAD] != 0) {
    const int64_t i = n_lab - (int64_t)m[PM_BAD];
    int32_t v = 0;
    VGS_READBACK(c, &v, labels_dev + i, sizeof(int32_t));
    c->err = std::string(fn) + ": labels[" + std::to_string(i) + "] = " + std::to_string(v) + " is not below K = " + std::to_string(K) +
             " (a label must be negative or in 0 .. K-1)";
    return VGS_E_ARG;
  }
  if (n_skipped) *n_skipped = (int64_t)m[PM_SKIPPED];
  return VGS_OK;
}

vgs_status vgs_check_label_range(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t n, int64_t K) {
  return ps_scan_labels(c, fn, labels_dev, nullptr, n, n, 0, n, K, nullptr, nullptr, nullptr);
}

static vgs_status ps_check(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t n, int64_t K) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of the cloud; the tables of a point labelling need the whole cloud in one context";
    return VGS_E_STATE;
  }
  if (n != c->N) {
    c->err = std::string(fn) + ": n = " + std::to_string(n) + " must equal the number of points of the cloud, " + std::to_string(c->N);
    return VGS_E_ARG;
  }
  if (!labels && n > 0) { c->err = std::string(fn) + ": labels is NULL"; return VGS_E_ARG; }
  if (K < 0 || K > (int64_t)0x7fffffff) { c->err = std::string(fn) + ": K = " + std::to_string(K) + " is out of range"; return VGS_E_ARG; }
  return VGS_OK;
}

// the K rows in HBM (ps_npts, ps_nnodes, ps_f, ps_d)
struct PsTable {
  int64_t* npts; int32_t* nnodes; float *bbox, *eig8;
  double *cen, *cov, *eval, *evec;           // descriptors
  double *frame, *lo, *hi, *half, *center;   // boxes
};

// Steps 1-3: the finite points that carry a label 0 .. K-1, sorted by label, and the chunks of every label.  labels_dev holds n_lab entries
// for the input indices own_first .. (one context: 0 and N; a tile context: its own point range, so that only own points are sorted).
// Left on the stream; sorted = false (nothing queued behind the range check) for K = 0.  tmp_extra: bytes of ps_tmp the caller needs later.
// (PsSort: vgs_context.hpp; pointfield.hip runs the attribute tables over the same sort.)
vgs_status ps_sort_points(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t own_first, int64_t n_lab, int64_t K, size_t tmp_extra,
                                 int64_t* n_skipped, PsSort& S) {
  const int64_t N = c->N, nf = c->Nf;
  S.sorted = false;
  VGS_HIP_TRY(c, c->ps_key.ensure(2 * (size_t)nf + 1)); VGS_HIP_TRY(c, c->ps_val.ensure(2 * (size_t)nf + 1));
  uint32_t *key_in = c->ps_key.p, *key_out = key_in + nf, *val_in = c->ps_val.p, *val_out = val_in + nf;
  vgs_status s = ps_scan_labels(c, fn, labels_dev, nf > 0 ? c->perm_b.p : nullptr, N, nf, own_first, n_lab, K, key_in, val_in, n_skipped);
  if (s != VGS_OK) return s;
  if (K == 0) return VGS_OK;
  // only a label with a point has a ragged last chunk: sum over the labels of ceil(n_k / SD_CHUNK) <= floor(Nf / SD_CHUNK) + min(K, Nf)
  const int64_t n_chunks_max = nf / SD_CHUNK + std::min(K, nf) + 1;
  if (n_chunks_max * SD_TB >= ((int64_t)1 << 32)) {
    c->err = std::string(fn) + ": " + std::to_string(nf) + " points under " + std::to_string(K) + " labels need up to " + std::to_string(n_chunks_max) +
             " chunk workgroups, above the limit of one launch";
    return VGS_E_UNSUPPORTED;
  }
  const size_t k = (size_t)K;
  VGS_HIP_TRY(c, c->ps_seg.ensure(3 * (k + 1)));
  uint32_t *seg_start = c->ps_seg.p, *nchunk = seg_start + k + 1, *seg_chunk = nchunk + k + 1;
  unsigned bits = 1;
  while (bits < 32 && (1ull << bits) <= (unsigned long long)K) ++bits;   // keys 0 .. K
  size_t t_sort = 0, t_scan = 0;
  if (nf > 0) VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, key_in, key_out, val_in, val_out, (size_t)nf, 0, bits, c->stream));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_scan, nchunk, seg_chunk, 0u, k + 1, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, c->ps_tmp.ensure(std::max(std::max(t_sort, t_scan), tmp_extra)));
  if (nf > 0) VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->ps_tmp.p, t_sort, key_in, key_out, val_in, val_out, (size_t)nf, 0, bits, c->stream));
  hipLaunchKernelGGL(k_ps_segments, dim3((unsigned)((k + 1 + PS_TB - 1) / PS_TB)), dim3(PS_TB), 0, c->stream, key_out, (uint32_t)nf, (uint32_t)K, seg_start,
                     nchunk);
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->ps_tmp.p, t_scan, nchunk, seg_chunk, 0u, k + 1, rocprim::plus<uint32_t>(), c->stream));
  S.sorted = true; S.key = key_out; S.pos = val_out; S.seg_start = seg_start; S.seg_chunk = seg_chunk; S.n_chunks_max = n_chunks_max;
  return VGS_OK;
}

// Steps 1-5 over labels_dev, and step 6 when frame >= 0: the rows are left in the ps_* buffers (T), the stream is not waited for.
static vgs_status ps_tables_on_device(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, int frame, PsTable& T, int64_t* n_skipped) {
  const int64_t nf = c->Nf;
  PsSort S;
  vgs_status s = ps_sort_points(c, fn, labels_dev, 0, c->N, K, 0, n_skipped, S);
  if (s != VGS_OK) return s;
  if (!S.sorted) return VGS_OK;
  const size_t k = (size_t)K;
  const int64_t n_chunks_max = S.n_chunks_max;
  uint32_t *val_out = S.pos, *seg_start = S.seg_start, *seg_chunk = S.seg_chunk;
  VGS_HIP_TRY(c, c->ps_part.ensure((size_t)n_chunks_max * SD_REC)); VGS_HIP_TRY(c, c->ps_nn.ensure((size_t)n_chunks_max));
  VGS_HIP_TRY(c, c->ps_npts.ensure(k)); VGS_HIP_TRY(c, c->ps_nnodes.ensure(k)); VGS_HIP_TRY(c, c->ps_f.ensure(14 * k));
  VGS_HIP_TRY(c, c->ps_d.ensure(42 * k));
  T.npts = c->ps_npts.p; T.nnodes = c->ps_nnodes.p; T.bbox = c->ps_f.p; T.eig8 = T.bbox + 6 * k;
  T.cen = c->ps_d.p; T.cov = T.cen + 3 * k; T.eval = T.cov + 6 * k; T.evec = T.eval + 3 * k;
  T.frame = T.evec + 9 * k; T.lo = T.frame + 9 * k; T.hi = T.lo + 3 * k; T.half = T.hi + 3 * k; T.center = T.half + 3 * k;
  const unsigned waves_grid = (unsigned)((K + 3) / 4);
  if (nf > 0)
    hipLaunchKernelGGL(k_ps_chunks, dim3((unsigned)n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, val_out, c->pt_vox.p, seg_start,
                       seg_chunk, (uint32_t)K, c->ps_part.p, c->ps_nn.p);
  hipLaunchKernelGGL(k_ps_final, dim3(waves_grid), dim3(256), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, val_out, seg_start, seg_chunk, c->ps_part.p,
                     c->ps_nn.p, (uint32_t)n_chunks_max, (uint32_t)K, c->P.method == 3 ? 1 : 0, T.npts, T.nnodes, T.bbox, T.cen, T.cov, T.eval, T.evec, T.eig8);
  if (frame >= 0) {
    // (the descriptor partials are folded: the same buffer takes the shorter extent records)
    sb_launch_frames(c, T.evec, T.cov, K, frame, T.frame);
    if (nf > 0)
      hipLaunchKernelGGL(k_ps_box_chunks, dim3((unsigned)n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, val_out, seg_start, seg_chunk,
                         (uint32_t)K, T.cen, T.frame, c->ps_part.p);
    hipLaunchKernelGGL(k_ps_box_final, dim3(waves_grid), dim3(256), 0, c->stream, seg_chunk, c->ps_part.p, (uint32_t)n_chunks_max, (uint32_t)K, T.cen,
                       T.frame, T.lo, T.hi, T.half, T.center);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}

// the host variants' one upload into a buffer of the context
vgs_status vgs_upload_point_labels(vgs_ctx* c, const int32_t* labels_host, int64_t n, const int32_t** labels_dev) {
  *labels_dev = nullptr;
  if (n <= 0) return VGS_OK;
  VGS_HIP_TRY(c, c->ps_in.ensure((size_t)n));
  VGS_HIP_TRY(c, hipMemcpyAsync(c->ps_in.p, labels_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
  *labels_dev = c->ps_in.p;
  return VGS_OK;
}

#define PS_COPY(dst, src, count) \
  if (dst) VGS_HIP_TRY(c, hipMemcpyAsync((dst), (src), (count) * sizeof(*(dst)), hipMemcpyDeviceToHost, c->stream))

static vgs_status ps_descriptors(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t n, int64_t K, int64_t* n_skipped,
                                 int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3, double* evecs9,
                                 float* eigen8) {
  if (!c) return VGS_E_ARG;
  vgs_status s = ps_check(c, fn, labels, n, K);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device && (s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK) return s;
  PsTable T;
  if ((s = ps_tables_on_device(c, fn, labels, K, -1, T, n_skipped)) != VGS_OK) return s;
  const size_t k = (size_t)K;
  if (k > 0) {
    PS_COPY(n_points, T.npts, k); PS_COPY(n_nodes, T.nnodes, k); PS_COPY(bbox6, T.bbox, 6 * k); PS_COPY(centroid3, T.cen, 3 * k);
    PS_COPY(cov6, T.cov, 6 * k); PS_COPY(evals3, T.eval, 3 * k); PS_COPY(evecs9, T.evec, 9 * k); PS_COPY(eigen8, T.eig8, 8 * k);
  }
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the rows have arrived, and a labelling read in place is the caller's again
  return VGS_OK;
}

static vgs_status ps_boxes(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t n, int64_t K, int32_t frame, double* center3,
                           double* half3, double* frame9, double* lo3, double* hi3) {
  if (!c) return VGS_E_ARG;
  if (frame != VGS_BOX_PRINCIPAL && frame != VGS_BOX_UPRIGHT) {
    c->err = std::string(fn) + ": frame must be VGS_BOX_PRINCIPAL (0) or VGS_BOX_UPRIGHT (1)";
    return VGS_E_ARG;
  }
  vgs_status s = ps_check(c, fn, labels, n, K);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device && (s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK) return s;
  PsTable T;
  if ((s = ps_tables_on_device(c, fn, labels, K, frame, T, nullptr)) != VGS_OK) return s;
  const size_t k = (size_t)K;
  if (k > 0) {
    PS_COPY(center3, T.center, 3 * k); PS_COPY(half3, T.half, 3 * k); PS_COPY(frame9, T.frame, 9 * k); PS_COPY(lo3, T.lo, 3 * k); PS_COPY(hi3, T.hi, 3 * k);
  }
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGS_OK;
}

extern "C" vgs_status vgs_point_label_descriptors(vgs_ctx* c, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_skipped, int64_t* n_points,
                                                  int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3, double* evecs9,
                                                  float* eigen8) {
  return ps_descriptors(c, "vgs_point_label_descriptors", labels_host, false, n, K, n_skipped, n_points, n_nodes, bbox6, centroid3, cov6, evals3, evecs9,
                        eigen8);
}

extern "C" vgs_status vgs_point_label_descriptors_device(vgs_ctx* c, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_skipped,
                                                         int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6,
                                                         double* evals3, double* evecs9, float* eigen8) {
  return ps_descriptors(c, "vgs_point_label_descriptors_device", labels_dev, true, n, K, n_skipped, n_points, n_nodes, bbox6, centroid3, cov6, evals3,
                        evecs9, eigen8);
}

extern "C" vgs_status vgs_point_label_boxes(vgs_ctx* c, const int32_t* labels_host, int64_t n, int64_t K, int32_t frame, double* center3, double* half3,
                                            double* frame9, double* lo3, double* hi3) {
  return ps_boxes(c, "vgs_point_label_boxes", labels_host, false, n, K, frame, center3, half3, frame9, lo3, hi3);
}

extern "C" vgs_status vgs_point_label_boxes_device(vgs_ctx* c, const int32_t* labels_dev, int64_t n, int64_t K, int32_t frame, double* center3,
                                                   double* half3, double* frame9, double* lo3, double* hi3) {
  return ps_boxes(c, "vgs_point_label_boxes_device", labels_dev, true, n, K, frame, center3, half3, frame9, lo3, hi3);
}

// ------------------------------------------------------------------------------------------------ tile contexts (include/vgs_tiles.h)
// A rank hands in one label per point of its OWN load (own point i = cloud point own_first + i) and only per-label records travel.  The
// pipeline above runs over the own points alone: k_ps_keys gives every other position the key K, so the sort, the chunks, the anchor and
// the folds see own points only.  n_nodes over all ranks counted once: a head flag in a voxel that holds points of another rank too
// (k_ps_shared) is not counted here but leaves as a pair record (voxel code, label); the driver counts the distinct pairs of all ranks
// (vgs_tiles_fold_label_pairs).  The records wait in host arrays of the context (pso_*) until vgs_get_own_point_label_moments.
static vgs_status ps_own_check(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t n_own, int64_t K) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (!c->have_region || c->n_own < 0) {
    c->err = std::string(fn) + ": a tile context (vgs_set_owned_region and vgs_set_own_point_range) only";
    return VGS_E_STATE;
  }
  if (K < 0 || K > (int64_t)0x7fffffff) { c->err = std::string(fn) + ": K = " + std::to_string(K) + " is out of range"; return VGS_E_ARG; }
  if (n_own != c->n_own) {
    c->err = std::string(fn) + ": n_own = " + std::to_string(n_own) + " must equal the number of own points of the context, " + std::to_string(c->n_own);
    return VGS_E_ARG;
  }
  if (!labels && n_own > 0) { c->err = std::string(fn) + ": labels is NULL"; return VGS_E_ARG; }
  if (c->own_first < 0 || c->own_first + n_own > c->N) {
    c->err = std::string(fn) + ": the own point range ends at " + std::to_string(c->own_first + n_own) + ", the cloud holds " + std::to_string(c->N) + " points";
    return VGS_E_ARG;
  }
  return VGS_OK;
}

static vgs_status ps_own_moments(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t K, int64_t n_own, int64_t* n_records,
                                 int64_t* n_pairs, int64_t* n_skipped) {
  if (!c) return VGS_E_ARG;
  vgs_status s = ps_own_check(c, fn, labels, n_own, K);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  c->pso_K = -1;
  if (n_records) *n_records = 0;
  if (n_pairs) *n_pairs = 0;
  if (!on_device && (s = vgs_upload_point_labels(c, labels, n_own, &labels)) != VGS_OK) return s;
  const int64_t nf = c->Nf, V = c->V;
  size_t t_inc = 0;
  if (nf > 0 && K > 0) {
    VGS_HIP_TRY(c, c->ps_flag.ensure(2 * (size_t)nf));
    VGS_HIP_TRY(c, rocprim::inclusive_scan(nullptr, t_inc, c->ps_flag.p, c->ps_flag.p + nf, (size_t)nf, rocprim::plus<uint32_t>(), c->stream));
  }
  PsSort S;
  if ((s = ps_sort_points(c, fn, labels, c->own_first, n_own, K, t_inc, n_skipped, S)) != VGS_OK) return s;
  c->pso_label.clear(); c->pso_npts.clear(); c->pso_nnodes.clear(); c->pso_bbox.clear(); c->pso_anchor.clear(); c->pso_s9.clear();
  c->pso_pcode.clear(); c->pso_plab.clear();
  if (!S.sorted || nf == 0 || V == 0) { c->pso_K = K; return VGS_OK; }
  const size_t k = (size_t)K;
  VGS_HIP_TRY(c, c->ps_part.ensure((size_t)S.n_chunks_max * SD_REC)); VGS_HIP_TRY(c, c->ps_nn.ensure((size_t)S.n_chunks_max));
  VGS_HIP_TRY(c, c->ps_d.ensure(k * SD_MREC)); VGS_HIP_TRY(c, c->ps_shared.ensure((size_t)V));
  uint32_t *flag = c->ps_flag.p, *inc = flag + nf;
  VGS_HIP_TRY(c, hipMemsetAsync(c->ps_shared.p, 0, (size_t)V, c->stream));
  VGS_HIP_TRY(c, hipMemsetAsync(flag, 0, (size_t)nf * sizeof(uint32_t), c->stream));
  const unsigned pos_grid = (unsigned)((nf + PS_TB - 1) / PS_TB);
  hipLaunchKernelGGL(k_ps_shared, dim3(pos_grid), dim3(PS_TB), 0, c->stream, c->perm_b.p, c->pt_vox.p, nf, c->own_first, c->own_first + n_own, c->ps_shared.p);
  hipLaunchKernelGGL(k_ps_own_chunks, dim3((unsigned)S.n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, S.pos, c->pt_vox.p, S.seg_start,
                     S.seg_chunk, (uint32_t)K, c->ps_part.p, c->ps_nn.p, c->ps_shared.p, flag);
  hipLaunchKernelGGL(k_ps_own_records, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, S.pos, S.seg_start, S.seg_chunk,
                     c->ps_part.p, c->ps_nn.p, (uint32_t)S.n_chunks_max, (uint32_t)K, c->ps_d.p);
  VGS_HIP_TRY(c, rocprim::inclusive_scan(c->ps_tmp.p, t_inc, flag, inc, (size_t)nf, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, hipGetLastError());
  uint32_t np = 0;
  std::vector<double> m(k * SD_MREC);
  VGS_HIP_TRY(c, hipMemcpyAsync(&np, inc + nf - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipMemcpyAsync(m.data(), c->ps_d.p, m.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (np > 0) {
    VGS_HIP_TRY(c, c->ps_pcode.ensure((size_t)np)); VGS_HIP_TRY(c, c->ps_plab.ensure((size_t)np));
    hipLaunchKernelGGL(k_ps_pairs, dim3(pos_grid), dim3(PS_TB), 0, c->stream, flag, inc, S.key, S.pos, c->pt_vox.p, c->vox_code.p, nf, c->ps_pcode.p,
                       c->ps_plab.p);
    VGS_HIP_TRY(c, hipGetLastError());
    c->pso_pcode.resize(np); c->pso_plab.resize(np);
    VGS_HIP_TRY(c, hipMemcpyAsync(c->pso_pcode.data(), c->ps_pcode.p, (size_t)np * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->pso_plab.data(), c->ps_plab.p, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  for (size_t i = 0; i < k; ++i) {
    const double* r = m.data() + i * SD_MREC;
    if (r[0] == 0.0) continue;   // no own finite point of this label here
    c->pso_label.push_back((int32_t)i); c->pso_npts.push_back((int64_t)r[0]); c->pso_nnodes.push_back((int32_t)r[1]);
    for (int f = 0; f < 6; ++f) c->pso_bbox.push_back((float)r[2 + f]);
    for (int f = 0; f < 3; ++f) c->pso_anchor.push_back((float)r[8 + f]);
    for (int f = 0; f < 9; ++f) c->pso_s9.push_back(r[11 + f]);
  }
  c->pso_K = K;
  if (n_records) *n_records = (int64_t)c->pso_label.size();
  if (n_pairs) *n_pairs = (int64_t)np;
  return VGS_OK;
}

extern "C" vgs_status vgs_own_point_label_moments(vgs_ctx* c, int64_t K, const int32_t* labels_host, int64_t n_own, int64_t* n_records, int64_t* n_pairs,
                                                  int64_t* n_skipped) {
  return ps_own_moments(c, "vgs_own_point_label_moments", labels_host, false, K, n_own, n_records, n_pairs, n_skipped);
}

extern "C" vgs_status vgs_own_point_label_moments_device(vgs_ctx* c, int64_t K, const int32_t* labels_dev, int64_t n_own, int64_t* n_records,
                                                         int64_t* n_pairs, int64_t* n_skipped) {
  return ps_own_moments(c, "vgs_own_point_label_moments_device", labels_dev, true, K, n_own, n_records, n_pairs, n_skipped);
}

extern "C" vgs_status vgs_get_own_point_label_moments(vgs_ctx* c, int32_t* label, int64_t* n_points, int32_t* n_nodes, float* bbox6, float* anchor3,
                                                      double* s9, uint64_t* pair_code, int32_t* pair_label) {
  if (!c) return VGS_E_ARG;
  if (c->stage < ST_SEGMENTED || c->pso_K < 0) {
    c->err = "vgs_get_own_point_label_moments: no own records (vgs_own_point_label_moments first; a run of the stages or new labels discard them)";
    return VGS_E_STATE;
  }
  if (label) std::copy(c->pso_label.begin(), c->pso_label.end(), label);
  if (n_points) std::copy(c->pso_npts.begin(), c->pso_npts.end(), n_points);
  if (n_nodes) std::copy(c->pso_nnodes.begin(), c->pso_nnodes.end(), n_nodes);
  if (bbox6) std::copy(c->pso_bbox.begin(), c->pso_bbox.end(), bbox6);
  if (anchor3) std::copy(c->pso_anchor.begin(), c->pso_anchor.end(), anchor3);
  if (s9) std::copy(c->pso_s9.begin(), c->pso_s9.end(), s9);
  if (pair_code) std::copy(c->pso_pcode.begin(), c->pso_pcode.end(), pair_code);
  if (pair_label) std::copy(c->pso_plab.begin(), c->pso_plab.end(), pair_label);
  return VGS_OK;
}

// The contract of vgs_get_own_segment_extents over the own points sorted by label: the rows handed in make the frames (k_sb_frames), then
// k_ps_box_chunks over the own pos_sorted and the fold of k_sb_final; a label without an own point keeps the empty record and is left out.
static vgs_status ps_own_extents(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t K, int32_t frame, int64_t n_own,
                                 const double* centroid3, const double* cov6, const double* evecs9, int64_t* n_records, int32_t* label, double* lo3,
                                 double* hi3) {
  if (!c || !n_records) return VGS_E_ARG;
  *n_records = 0;
  if (frame != VGS_BOX_PRINCIPAL && frame != VGS_BOX_UPRIGHT) {
    c->err = std::string(fn) + ": frame must be VGS_BOX_PRINCIPAL (0) or VGS_BOX_UPRIGHT (1)";
    return VGS_E_ARG;
  }
  vgs_status s = ps_own_check(c, fn, labels, n_own, K);
  if (s != VGS_OK) return s;
  if (K > 0 && (!centroid3 || !cov6 || !evecs9)) { c->err = std::string(fn) + ": centroid3, cov6 and evecs9 are required"; return VGS_E_ARG; }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device && (s = vgs_upload_point_labels(c, labels, n_own, &labels)) != VGS_OK) return s;
  PsSort S;
  if ((s = ps_sort_points(c, fn, labels, c->own_first, n_own, K, 0, nullptr, S)) != VGS_OK) return s;
  if (!S.sorted || c->Nf == 0) return VGS_OK;
  VGS_HIP_TRY(c, c->ps_part.ensure((size_t)S.n_chunks_max * SD_REC));
  if ((s = sbt_upload_frames(c, K, frame, centroid3, cov6, evecs9)) != VGS_OK) return s;
  hipLaunchKernelGGL(k_ps_box_chunks, dim3((unsigned)S.n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, S.pos, S.seg_start, S.seg_chunk,
                     (uint32_t)K, c->sbt_in.p, c->sbt_frame.p, c->ps_part.p);
  sbt_launch_final(c, K, S.seg_chunk, c->ps_part.p, (uint32_t)S.n_chunks_max);
  VGS_HIP_TRY(c, hipGetLastError());
  std::vector<double> e(6 * (size_t)K);   // lo3 | hi3
  VGS_HIP_TRY(c, hipMemcpyAsync(e.data(), c->sbt_out.p, e.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double* lo = e.data();
  const double* hi = lo + 3 * (size_t)K;
  int64_t n = 0;
  for (int64_t k = 0; k < K; ++k) {
    if (lo[3 * k] > hi[3 * k]) continue;   // the empty record: no own point of this label here
    if (label) label[n] = (int32_t)k;
    if (lo3) for (int f = 0; f < 3; ++f) lo3[3 * n + f] = lo[3 * k + f];
    if (hi3) for (int f = 0; f < 3; ++f) hi3[3 * n + f] = hi[3 * k + f];
    ++n;
  }
  *n_records = n;
  return VGS_OK;
}

extern "C" vgs_status vgs_get_own_point_label_extents(vgs_ctx* c, int64_t K, int32_t frame, const int32_t* labels_host, int64_t n_own,
                                                      const double* centroid3, const double* cov6, const double* evecs9, int64_t* n_records,
                                                      int32_t* label, double* lo3, double* hi3) {
  return ps_own_extents(c, "vgs_get_own_point_label_extents", labels_host, false, K, frame, n_own, centroid3, cov6, evecs9, n_records, label, lo3, hi3);
}

extern "C" vgs_status vgs_get_own_point_label_extents_device(vgs_ctx* c, int64_t K, int32_t frame, const int32_t* labels_dev, int64_t n_own,
                                                             const double* centroid3, const double* cov6, const double* evecs9, int64_t* n_records,
                                                             int32_t* label, double* lo3, double* hi3) {
  return ps_own_extents(c, "vgs_get_own_point_label_extents_device", labels_dev, true, K, frame, n_own, centroid3, cov6, evecs9, n_records, label, lo3,
                        hi3);
}
