// segdesc.hip -- per-segment geometric descriptors of the kept segments (no reference counterpart: what a caller of getClusterIdx
// computes next).  Descriptor k covers exactly the points whose label (vgs_get_point_labels) is k: point count, node count, exact
// float bounding box, fp64 centroid and population covariance, a double-precision Jacobi eigensolve, and vm_eigen_features.
//
// Data flow (everything already sits in HBM in the right order: xs/ys/zs hold the points sorted by node, vox_start gives each node's
// run, vox_label its kept label):
//   1. one stable radix sort of the node ids by label (V keys, not N points): the nodes of segment k are one run of the sorted list
//   2. per sorted node its run length, exclusive scan -> vp: the "virtual" position of the node's first point in the concatenation of all
//      segments' points in label order; per segment its node run (a binary search in the sorted keys) and ceil(points / SD_CHUNK) chunks,
//      exclusive scan -> the first chunk of every segment
//   3. k_sd_chunks: one workgroup per chunk of <= SD_CHUNK virtual points (a chunk never crosses a segment, it may split a node); it reads
//      its nodes' runs of xs/ys/zs and writes one partial record: sums of d = p - a and of d d^T in fp64, min and max, where the anchor a
//      is the segment's first point (its first node's first point) -- the same anchor in every chunk of the segment, so the partials add
//   4. k_sd_final: one wavefront per segment folds its partials, then computes centroid, covariance, eigen decomposition and features
// Determinism: every sum has a fixed shape -- which point a lane reads depends on (chunk, lane, step) only, the lanes fold by a fixed
// butterfly, the waves in index order, the partials of a segment by lane stride then butterfly.  No atomics.  Balance: a segment of
// millions of points is spread over its chunks like any other; a segment of a few hundred points costs one workgroup.
// Scratch: own buffers only (sd_*), nothing another getter reads.  Computed on request and cached until the next run (sd_valid).
// Tile contexts (the tiled driver, include/vgs_tiles.h): the same steps over global labels with own points only (k_sd_own_anchor,
// k_sd_chunks_own, k_sd_own_records) give this rank's moment records; the driver folds all ranks' records on the host and
// k_sd_algebra turns them into the table with the per-segment algebra k_sd_final runs (sd_segment_algebra, one copy).
#include <cstring>
#include <string.h>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "segpass.hpp"

// SD_TB threads of a chunk workgroup, SD_PPT points per thread, SD_CHUNK = SD_TB * SD_PPT virtual points per chunk: vgs_context.hpp;
// SD_REC doubles per partial record and the bodies shared with segbox.hip and pointseg.hip: segpass.hpp

// key of node v: its kept label, K for the nodes of dropped clusters (they sort behind every kept segment; so would a label >= K)
__global__ void k_sd_keys(const int32_t* __restrict__ vox_label, int64_t V, uint32_t K, uint32_t* __restrict__ key, uint32_t* __restrict__ ids) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int32_t l = vox_label[v];
  key[v] = (l < 0 || (uint32_t)l >= K) ? K : (uint32_t)l;
  ids[v] = (uint32_t)v;
}

// run length of the node at sorted position i (0 for dropped nodes and for the sentinel i = V)
__global__ void k_sd_runlen(const uint32_t* __restrict__ key, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ vox_start, int64_t V,
                            uint32_t K, uint32_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > V) return;
  uint32_t n = 0;
  if (i < V && key[i] < K) { const uint32_t v = ids[i]; n = vox_start[v + 1] - vox_start[v]; }
  len[i] = n;
}

// per segment k < K: first sorted node (seg_node[k], seg_node[K] = end of the kept nodes) and number of chunks (nchunk[K] = 0)
__global__ void k_sd_segments(const uint32_t* __restrict__ key, uint32_t V, uint32_t K, const uint32_t* __restrict__ vp,
                              uint32_t* __restrict__ seg_node, uint32_t* __restrict__ nchunk) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > K) return;
  const uint32_t n0 = sd_lower_bound(key, V, k);
  seg_node[k] = n0;
  if (k == K) { nchunk[k] = 0; return; }
  const uint32_t n1 = sd_lower_bound(key, V, k + 1);
  const uint32_t pts = vp[n1] - vp[n0];
  const uint32_t ch = (pts + SD_CHUNK - 1) / SD_CHUNK;
  nchunk[k] = ch > 0 ? ch : 1u;   // (a kept segment holds at least one point; the guard keeps the chunk -> segment search well defined)
}

// One workgroup per chunk of SD_CHUNK virtual points of one segment.  Grid: an upper bound of the number of chunks (floor(Nf / SD_CHUNK) +
// K + 1); workgroups past the real number leave at once.  OWN (tile contexts, k_sd_chunks_own): only the points whose input index
// perm[pos] lies in [own_first, own_end) count -- in the sums, the min / max and the point count (field 15) -- and the anchor is the
// segment's first own point (anchor_pos[k], from k_sd_own_anchor); a segment without own points writes an empty record.
template <bool OWN>
__device__ __forceinline__ void sd_chunk_body(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                              const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                              const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                              const uint32_t* __restrict__ seg_chunk, uint32_t K, double* __restrict__ part,
                                              const uint32_t* __restrict__ perm, int64_t own_first, int64_t own_end,
                                              const uint32_t* __restrict__ anchor_pos) {
  __shared__ uint32_t s_vp[SD_CHUNK];    // virtual start of the chunk's nodes
  __shared__ uint32_t s_dl[SD_CHUNK];    // sorted position - virtual position of the same (mod 2^32)
  const uint32_t c = blockIdx.x;
  SdChunk wk;
  if (!sd_walk(vox_start, ids, vp, seg_node, seg_chunk, K, s_vp, s_dl, wk)) {
    if (wk.k != 0xffffffffu) sd_empty_record(part + (size_t)c * SD_REC);   // (an empty record keeps the fold well defined)
    return;
  }
  const uint32_t k = wk.k, a = wk.a, b = wk.b, m = wk.m;
  // the anchor: the segment's first point (OWN: its first own point), the same for every chunk of the segment
  const uint32_t pa = OWN ? anchor_pos[k] : vox_start[ids[wk.n0]];
  if (OWN && pa == 0xffffffffu) {   // no own point in this segment: nothing counts
    sd_empty_record(part + (size_t)c * SD_REC);
    return;
  }
  const double ax = (double)xs[pa], ay = (double)ys[pa], az = (double)zs[pa];
  // the sums, the butterflies and the waves in index order: segpass.hpp (its first barrier closes the staging above)
  sd_chunk_sums<OWN>(xs, ys, zs, a, b, ax, ay, az, [&](uint32_t q) { return sd_pos(s_vp, s_dl, m, q); }, part + (size_t)c * SD_REC, perm, own_first,
                     own_end);
}

__global__ __launch_bounds__(SD_TB) void k_sd_chunks(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                     const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                     const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                                     const uint32_t* __restrict__ seg_chunk, uint32_t K, double* __restrict__ part) {
  sd_chunk_body<false>(xs, ys, zs, vox_start, ids, vp, seg_node, seg_chunk, K, part, nullptr, 0, 0, nullptr);
}

__global__ __launch_bounds__(SD_TB) void k_sd_chunks_own(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                         const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                         const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                                         const uint32_t* __restrict__ seg_chunk, uint32_t K, double* __restrict__ part,
                                                         const uint32_t* __restrict__ perm, int64_t own_first, int64_t own_end,
                                                         const uint32_t* __restrict__ anchor_pos) {
  sd_chunk_body<true>(xs, ys, zs, vox_start, ids, vp, seg_node, seg_chunk, K, part, perm, own_first, own_end, anchor_pos);
}

// Tile contexts: one wavefront per segment finds its first own point in the chunks' order (sorted nodes, each node's run in order):
// 64 nodes at a time, each lane scans its node's run, the lowest lane that found one wins.  anchor_pos[k] = its sorted position, or
// 0xffffffff when the segment holds no own point here.
__global__ __launch_bounds__(256) void k_sd_own_anchor(const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                       const uint32_t* __restrict__ seg_node, const uint32_t* __restrict__ perm,
                                                       int64_t own_first, int64_t own_end, uint32_t K, uint32_t* __restrict__ anchor_pos) {
  const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= K) return;   // (whole wavefronts; no barrier follows)
  const uint32_t n0 = seg_node[k], n1 = seg_node[k + 1];
  uint32_t found = 0xffffffffu;
  for (uint32_t base = n0; base < n1; base += 64) {
    const uint32_t i = base + lane;
    uint32_t p = 0xffffffffu;
    if (i < n1) {
      const uint32_t v = ids[i], e = vox_start[v + 1];
      for (uint32_t j = vox_start[v]; j < e; ++j) {
        const int64_t o = (int64_t)perm[j];
        if (o >= own_first && o < own_end) { p = j; break; }
      }
    }
    const uint64_t hit = __ballot(p != 0xffffffffu);
    if (hit) { found = __shfl(p, __ffsll((unsigned long long)hit) - 1, 64); break; }
  }
  if (lane == 0) anchor_pos[k] = found;
}

// sd_fold_partials and sd_segment_algebra (the one copy of the per-segment algebra, with its Jacobi rotations): segpass.hpp

// one wavefront per segment: fold its partials (lane stride, then butterfly), then everything per segment on lane 0
__global__ __launch_bounds__(256) void k_sd_final(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                  const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                  const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                                  const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part, uint32_t n_part, uint32_t K, int svgs,
                                                  int64_t* __restrict__ o_npts, int32_t* __restrict__ o_nnodes, float* __restrict__ o_bbox,
                                                  double* __restrict__ o_cen, double* __restrict__ o_cov, double* __restrict__ o_eval,
                                                  double* __restrict__ o_evec, float* __restrict__ o_eig8) {
  const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= K) return;   // (whole wavefronts; no barrier follows)
  const uint32_t c0 = seg_chunk[k], c1 = min(seg_chunk[k + 1], n_part);   // (the bound only guards the records: the chunks fit, see the launch)
  double s[9], mn[3], mx[3], cnt;
  sd_fold_partials<false>(part, c0, c1, lane, s, mn, mx, cnt);
  if (lane != 0) return;
  const uint32_t n0 = seg_node[k], n1 = seg_node[k + 1];
  const uint32_t n = vp[n1] - vp[n0];
  const uint32_t pa = vox_start[ids[n0]];
  const double anc[3] = {(double)xs[pa], (double)ys[pa], (double)zs[pa]};
  sd_segment_algebra(k, (int64_t)n, (int32_t)(n1 - n0), mn, mx, anc, s, svgs, o_npts, o_nnodes, o_bbox, o_cen, o_cov, o_eval, o_evec, o_eig8);
}

// Tile contexts: one wavefront per segment folds the partials of k_sd_chunks_own exactly as k_sd_final does, counts the segment's
// owned voxels (lane stride, then butterfly) and writes its moment record: SD_MREC doubles = own points, owned voxels, min[3], max[3]
// (float values), anchor[3] (the first own point's floats; 0 without one), sum d[3], sum d d^T[6].
__global__ __launch_bounds__(256) void k_sd_own_records(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                        const uint32_t* __restrict__ ids, const uint32_t* __restrict__ seg_node,
                                                        const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part, uint32_t n_part,
                                                        const uint32_t* __restrict__ anchor_pos, const uint8_t* __restrict__ owned, uint32_t K,
                                                        double* __restrict__ mom) {
  const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= K) return;   // (whole wavefronts; no barrier follows)
  const uint32_t c0 = seg_chunk[k], c1 = min(seg_chunk[k + 1], n_part);
  double s[9], mn[3], mx[3], cnt;
  sd_fold_partials<true>(part, c0, c1, lane, s, mn, mx, cnt);
  const uint32_t n0 = seg_node[k], n1 = seg_node[k + 1];
  uint32_t no = 0;
  for (uint32_t i = n0 + lane; i < n1; i += 64) no += owned[ids[i]] ? 1u : 0u;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) no += __shfl_xor(no, m, 64);
  if (lane != 0) return;
  const uint32_t pa = anchor_pos[k];
  double* r = mom + (size_t)k * SD_MREC;
  r[0] = cnt;
  r[1] = (double)no;
#pragma unroll
  for (int f = 0; f < 3; ++f) { r[2 + f] = mn[f]; r[5 + f] = mx[f]; }
  r[8] = pa != 0xffffffffu ? (double)xs[pa] : 0.0;
  r[9] = pa != 0xffffffffu ? (double)ys[pa] : 0.0;
  r[10] = pa != 0xffffffffu ? (double)zs[pa] : 0.0;
#pragma unroll
  for (int f = 0; f < 9; ++f) r[11 + f] = s[f];
}

// Moments folded over the ranks (same record layout as k_sd_own_records) -> the table: one thread per segment, sd_segment_algebra
__global__ __launch_bounds__(256) void k_sd_algebra(const double* __restrict__ mom, uint32_t K, int svgs, int64_t* __restrict__ o_npts,
                                                    int32_t* __restrict__ o_nnodes, float* __restrict__ o_bbox, double* __restrict__ o_cen,
                                                    double* __restrict__ o_cov, double* __restrict__ o_eval, double* __restrict__ o_evec,
                                                    float* __restrict__ o_eig8) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const double* r = mom + (size_t)k * SD_MREC;
  const double mn[3] = {r[2], r[3], r[4]}, mx[3] = {r[5], r[6], r[7]}, anc[3] = {r[8], r[9], r[10]};
  const double s[9] = {r[11], r[12], r[13], r[14], r[15], r[16], r[17], r[18], r[19]};
  sd_segment_algebra(k, (int64_t)r[0], (int32_t)r[1], mn, mx, anc, s, svgs, o_npts, o_nnodes, o_bbox, o_cen, o_cov, o_eval, o_evec, o_eig8);
}


// Steps 1-2 for labels 0 .. K-1 and the launch of step 3's grid bound: sorted node ids, virtual positions, per segment its first sorted
// node and first chunk.  Pointers into the sd_* scratch.  (SdPrep: vgs_context.hpp; segbox.hip runs the same steps.)
vgs_status sd_prepare(vgs_ctx* c, int64_t K, SdPrep& o) {
  const int64_t V = c->V, nf = c->Nf;
  VGS_HIP_TRY(c, c->sd_key.ensure(2 * (size_t)V)); VGS_HIP_TRY(c, c->sd_ids.ensure(2 * (size_t)V));
  VGS_HIP_TRY(c, c->sd_vp.ensure(2 * ((size_t)V + 1)));
  VGS_HIP_TRY(c, c->sd_seg.ensure(3 * ((size_t)K + 1)));
  uint32_t *key_in = c->sd_key.p, *key_out = key_in + V, *ids_in = c->sd_ids.p, *ids_out = ids_in + V;
  uint32_t *len = c->sd_vp.p, *vp = len + V + 1;
  uint32_t *seg_node = c->sd_seg.p, *nchunk = seg_node + K + 1, *seg_chunk = nchunk + K + 1;
  const int TB = 256;
  hipLaunchKernelGGL(k_sd_keys, dim3((unsigned)((V + TB - 1) / TB)), dim3(TB), 0, c->stream, c->vox_label.p, V, (uint32_t)K, key_in, ids_in);
  unsigned bits = 1;
  while (bits < 32 && (1ull << bits) <= (unsigned long long)K) ++bits;   // keys 0 .. K
  size_t t_sort = 0, t_scan1 = 0, t_scan2 = 0;
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, key_in, key_out, ids_in, ids_out, (size_t)V, 0, bits, c->stream));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_scan1, len, vp, 0u, (size_t)V + 1, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_scan2, nchunk, seg_chunk, 0u, (size_t)K + 1, rocprim::plus<uint32_t>(), c->stream));
  size_t t_max = t_sort > t_scan1 ? t_sort : t_scan1;
  if (t_scan2 > t_max) t_max = t_scan2;
  VGS_HIP_TRY(c, c->sd_tmp.ensure(t_max));
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->sd_tmp.p, t_sort, key_in, key_out, ids_in, ids_out, (size_t)V, 0, bits, c->stream));
  hipLaunchKernelGGL(k_sd_runlen, dim3((unsigned)((V + 1 + TB - 1) / TB)), dim3(TB), 0, c->stream, key_out, ids_out, c->vox_start.p, V,
                     (uint32_t)K, len);
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sd_tmp.p, t_scan1, len, vp, 0u, (size_t)V + 1, rocprim::plus<uint32_t>(), c->stream));
  hipLaunchKernelGGL(k_sd_segments, dim3((unsigned)((K + 1 + TB - 1) / TB)), dim3(TB), 0, c->stream, key_out, (uint32_t)V, (uint32_t)K, vp,
                     seg_node, nchunk);
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sd_tmp.p, t_scan2, nchunk, seg_chunk, 0u, (size_t)K + 1, rocprim::plus<uint32_t>(), c->stream));
  // sum over segments of ceil(n_k / SD_CHUNK) <= floor(Nf / SD_CHUNK) + K: launched without reading the real number back
  o.n_chunks_max = nf / SD_CHUNK + K + 1;
  VGS_HIP_TRY(c, c->sd_part.ensure((size_t)o.n_chunks_max * SD_REC));
  o.ids = ids_out; o.vp = vp; o.seg_node = seg_node; o.seg_chunk = seg_chunk;
  return VGS_OK;
}

static vgs_status sd_ensure_table(vgs_ctx* c, size_t k1) {
  VGS_HIP_TRY(c, c->sd_npts.ensure(k1)); VGS_HIP_TRY(c, c->sd_nnodes.ensure(k1));
  VGS_HIP_TRY(c, c->sd_bbox.ensure(6 * k1)); VGS_HIP_TRY(c, c->sd_eig8.ensure(8 * k1));
  VGS_HIP_TRY(c, c->sd_cen.ensure(3 * k1)); VGS_HIP_TRY(c, c->sd_cov.ensure(6 * k1));
  VGS_HIP_TRY(c, c->sd_eval.ensure(3 * k1)); VGS_HIP_TRY(c, c->sd_evec.ensure(9 * k1));
  return VGS_OK;
}

// The table in HBM, K = counts[VGS_N_KEPT] rows; valid until the next run of the stages.
vgs_status vgs_segdesc_on_device(vgs_ctx* c) {
  if (c->sd_valid) return VGS_OK;
  const int64_t K = c->counts[VGS_N_KEPT], V = c->V, nf = c->Nf;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  vgs_status s = sd_ensure_table(c, (size_t)(K > 0 ? K : 1));
  if (s != VGS_OK) return s;
  if (K == 0 || V == 0 || nf == 0) { c->sd_valid = true; return VGS_OK; }
  SdPrep P;
  if ((s = sd_prepare(c, K, P)) != VGS_OK) return s;
  hipLaunchKernelGGL(k_sd_chunks, dim3((unsigned)P.n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, c->vox_start.p, P.ids, P.vp,
                     P.seg_node, P.seg_chunk, (uint32_t)K, c->sd_part.p);
  hipLaunchKernelGGL(k_sd_final, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, c->vox_start.p, P.ids, P.vp,
                     P.seg_node, P.seg_chunk, c->sd_part.p, (uint32_t)P.n_chunks_max, (uint32_t)K, c->P.method == 3 ? 1 : 0, c->sd_npts.p, c->sd_nnodes.p, c->sd_bbox.p,
                     c->sd_cen.p, c->sd_cov.p, c->sd_eval.p, c->sd_evec.p, c->sd_eig8.p);
  VGS_HIP_TRY(c, hipGetLastError());
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->sd_valid = true;
  return VGS_OK;
}

static vgs_status sd_check(vgs_ctx* c, const char* fn) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of its segments; descriptors need the whole cloud in one context";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

extern "C" vgs_status vgs_get_segment_descriptors(vgs_ctx* c, int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6,
                                                  double* evals3, double* evecs9, float* eigen8) {
  if (!c) return VGS_E_ARG;
  vgs_status s = sd_check(c, "vgs_get_segment_descriptors");
  if (s != VGS_OK) return s;
  const size_t K = (size_t)c->counts[VGS_N_KEPT];
  if (K == 0) return VGS_OK;
  if ((s = vgs_segdesc_on_device(c)) != VGS_OK) return s;
  if (n_points) VGS_HIP_TRY(c, hipMemcpy(n_points, c->sd_npts.p, K * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (n_nodes) VGS_HIP_TRY(c, hipMemcpy(n_nodes, c->sd_nnodes.p, K * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (bbox6) VGS_HIP_TRY(c, hipMemcpy(bbox6, c->sd_bbox.p, 6 * K * sizeof(float), hipMemcpyDeviceToHost));
  if (centroid3) VGS_HIP_TRY(c, hipMemcpy(centroid3, c->sd_cen.p, 3 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (cov6) VGS_HIP_TRY(c, hipMemcpy(cov6, c->sd_cov.p, 6 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (evals3) VGS_HIP_TRY(c, hipMemcpy(evals3, c->sd_eval.p, 3 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (evecs9) VGS_HIP_TRY(c, hipMemcpy(evecs9, c->sd_evec.p, 9 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (eigen8) VGS_HIP_TRY(c, hipMemcpy(eigen8, c->sd_eig8.p, 8 * K * sizeof(float), hipMemcpyDeviceToHost));
  return VGS_OK;
}

extern "C" vgs_status vgs_get_segment_descriptors_device(vgs_ctx* c, const int64_t** n_points, const int32_t** n_nodes, const float** bbox6,
                                                         const double** centroid3, const double** cov6, const double** evals3,
                                                         const double** evecs9, const float** eigen8) {
  if (!c) return VGS_E_ARG;
  vgs_status s = sd_check(c, "vgs_get_segment_descriptors_device");
  if (s != VGS_OK) return s;
  if ((s = vgs_segdesc_on_device(c)) != VGS_OK) return s;
  if (n_points) *n_points = c->sd_npts.p;
  if (n_nodes) *n_nodes = c->sd_nnodes.p;
  if (bbox6) *bbox6 = c->sd_bbox.p;
  if (centroid3) *centroid3 = c->sd_cen.p;
  if (cov6) *cov6 = c->sd_cov.p;
  if (evals3) *evals3 = c->sd_eval.p;
  if (evecs9) *evecs9 = c->sd_evec.p;
  if (eigen8) *eigen8 = c->sd_eig8.p;
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ tile contexts (include/vgs_tiles.h)
// The first own point of every label 0 .. K-1 of a prepared decomposition into sd_apos (k_sd_own_anchor; left on the stream).  One launch
// site for the descriptor moments here and the attribute moments of segfield.hip.
vgs_status sd_own_anchor(vgs_ctx* c, int64_t K, const SdPrep& P) {
  VGS_HIP_TRY(c, c->sd_apos.ensure((size_t)K));
  hipLaunchKernelGGL(k_sd_own_anchor, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, c->stream, c->vox_start.p, P.ids, P.seg_node, c->perm_b.p,
                     c->own_first, c->own_first + c->n_own, (uint32_t)K, c->sd_apos.p);
  return VGS_OK;
}

// This rank's moments of the global labels 0 .. K-1: the pipeline above over vox_label (global after vgs_apply_tile_labels), with the
// own-point chunks, the first own point as anchor, and the owned-voxel count.  Dense on the device (K records), compact on the host.
extern "C" vgs_status vgs_get_own_segment_moments(vgs_ctx* c, int64_t K, int64_t* n_records, int32_t* label, int64_t* n_points, int32_t* n_nodes,
                                                  float* bbox6, float* anchor3, double* s9) {
  if (!c || !n_records || K < 0 || K >= (int64_t)0xffffffffLL) return VGS_E_ARG;
  if (c->stage < ST_SEGMENTED) { c->err = "vgs_get_own_segment_moments: segment first"; return VGS_E_STATE; }
  if (!c->have_region || c->n_own < 0) {
    c->err = "vgs_get_own_segment_moments: a tile context (vgs_set_owned_region and vgs_set_own_point_range) only";
    return VGS_E_STATE;
  }
  *n_records = 0;
  const int64_t V = c->V, nf = c->Nf;
  if (K == 0 || V == 0 || nf == 0) return VGS_OK;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  SdPrep P;
  vgs_status s = sd_prepare(c, K, P);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, c->sd_mom.ensure((size_t)K * SD_MREC));
  const int64_t own_end = c->own_first + c->n_own;
  const unsigned waves_grid = (unsigned)((K + 3) / 4);
  if ((s = sd_own_anchor(c, K, P)) != VGS_OK) return s;
  hipLaunchKernelGGL(k_sd_chunks_own, dim3((unsigned)P.n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, c->vox_start.p, P.ids, P.vp,
                     P.seg_node, P.seg_chunk, (uint32_t)K, c->sd_part.p, c->perm_b.p, c->own_first, own_end, c->sd_apos.p);
  hipLaunchKernelGGL(k_sd_own_records, dim3(waves_grid), dim3(256), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, P.ids, P.seg_node, P.seg_chunk,
                     c->sd_part.p, (uint32_t)P.n_chunks_max, c->sd_apos.p, c->owned.p, (uint32_t)K, c->sd_mom.p);
  VGS_HIP_TRY(c, hipGetLastError());
  std::vector<double> m((size_t)K * SD_MREC);
  VGS_HIP_TRY(c, hipMemcpyAsync(m.data(), c->sd_mom.p, m.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  int64_t n = 0;
  for (int64_t k = 0; k < K; ++k) {
    const double* r = m.data() + (size_t)k * SD_MREC;
    if (r[0] == 0.0 && r[1] == 0.0) continue;   // neither an own point nor an owned voxel of this label here
    if (label) label[n] = (int32_t)k;
    if (n_points) n_points[n] = (int64_t)r[0];
    if (n_nodes) n_nodes[n] = (int32_t)r[1];
    if (bbox6) for (int f = 0; f < 6; ++f) bbox6[6 * n + f] = (float)r[2 + f];
    if (anchor3) for (int f = 0; f < 3; ++f) anchor3[3 * n + f] = (float)r[8 + f];
    if (s9) for (int f = 0; f < 9; ++f) s9[9 * n + f] = r[11 + f];
    ++n;
  }
  *n_records = n;
  return VGS_OK;
}

// The table from moments folded over the ranks: uploaded as SD_MREC records, k_sd_algebra, the caller's arrays written back.
extern "C" vgs_status vgs_segment_descriptors_from_moments(vgs_ctx* c, int64_t K, const int64_t* n_points, const int32_t* n_nodes, const float* bbox6,
                                                           const float* anchor3, const double* s9, int64_t* n_points_out, int32_t* n_nodes_out,
                                                           float* bbox6_out, double* centroid3, double* cov6, double* evals3, double* evecs9,
                                                           float* eigen8) {
  if (!c || K < 0 || K >= (int64_t)0xffffffffLL || (K > 0 && (!n_points || !n_nodes || !bbox6 || !anchor3 || !s9))) return VGS_E_ARG;
  if (K == 0) return VGS_OK;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  std::vector<double> m((size_t)K * SD_MREC);
  for (int64_t k = 0; k < K; ++k) {
    double* r = m.data() + (size_t)k * SD_MREC;
    r[0] = (double)n_points[k];
    r[1] = (double)n_nodes[k];
    for (int f = 0; f < 6; ++f) r[2 + f] = (double)bbox6[6 * k + f];
    for (int f = 0; f < 3; ++f) r[8 + f] = (double)anchor3[3 * k + f];
    for (int f = 0; f < 9; ++f) r[11 + f] = s9[9 * k + f];
  }
  c->sd_valid = false;   // (the table buffers now hold these rows)
  vgs_status s = sd_ensure_table(c, (size_t)K);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, c->sd_mom.ensure(m.size()));
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sd_mom.p, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_sd_algebra, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, c->sd_mom.p, (uint32_t)K, c->P.method == 3 ? 1 : 0,
                     c->sd_npts.p, c->sd_nnodes.p, c->sd_bbox.p, c->sd_cen.p, c->sd_cov.p, c->sd_eval.p, c->sd_evec.p, c->sd_eig8.p);
  VGS_HIP_TRY(c, hipGetLastError());
  const RowCol col[8] = {{n_points_out, c->sd_npts.p, sizeof(int64_t)}, {n_nodes_out, c->sd_nnodes.p, sizeof(int32_t)},
                          {bbox6_out, c->sd_bbox.p, 6 * sizeof(float)},  {centroid3, c->sd_cen.p, 3 * sizeof(double)},
                          {cov6, c->sd_cov.p, 6 * sizeof(double)},       {evals3, c->sd_eval.p, 3 * sizeof(double)},
                          {evecs9, c->sd_evec.p, 9 * sizeof(double)},    {eigen8, c->sd_eig8.p, 8 * sizeof(float)}};
  return vgs_copy_rows(c, (size_t)K, col, 8);
}
