// segfield.hip -- per-segment statistics of point attributes the CALLER supplies (no reference counterpart: the first thing a user of a
// segmentation does with intensity, colour, time, class scores or a ground-truth class).  Row k covers exactly the points whose label
// (vgs_get_point_labels) is k.  Two tables:
//   field statistics  per (segment, channel): number of finite values, an anchor, fp64 mean and population variance about it, float min / max
//   class histogram   per (segment, class): point counts; per segment the points whose class is out of range, the majority class and its count
// The input is in INPUT order (row i belongs to input point i), the engine's points are sorted by node: perm_b maps a sorted position to
// the point's input index, so the pass is the decomposition of segdesc.hip -- sd_prepare: nodes sorted by label, virtual positions, chunks
// of SD_CHUNK virtual points that never cross a segment and may split a node -- with a gather through perm_b.
// Data flow of the field statistics, per group of SF_G channels (one partial buffer of n_chunks_max x SF_G records, whatever n_channels):
//   k_sf_anchor  once, every channel: the value of the segment's first point in the chunk order (segdesc.hip's anchor) as a double, 0.0
//                where that value is not finite -- one point per segment, the same for every channel
//   k_sf_chunks  one workgroup per chunk: i = perm_b[pos], the group's channels of row i; per channel, over the finite values, S1 = sum d,
//                S2 = sum d d with d = (double)x - anchor, the count, min and max; wavefront butterfly, the waves through LDS in index order
//   k_sf_final   one wavefront per (segment, channel of the group) folds the partials (lane stride, then butterfly) and writes
//                mean = anchor + S1 / n and var = max(0, S2 / n - (S1 / n) (S1 / n)), each one fp64 operation in that association (the build
//                passes -ffp-contract=off: no FMA)
// Determinism: the rule of segdesc.hip -- which point a lane reads depends on (chunk, lane, step) only, every fold has a fixed shape, no
// float atomics -- so the table is bit-identical from call to call and engine to engine.
// The histogram (k_sf_hist, k_sf_majority) holds integer counts, for which every summation order gives the same bits, so integer atomics
// are acceptable: the chunk's workgroup counts in LDS (n_classes + 1 counters of 32 bits; a wavefront first folds the lanes that share
// its first lane's class, so a segment of one class costs one LDS add per wavefront and step) and adds only its non-zero counters to the
// zeroed K x n_classes table -- at most one global add per (chunk, class), never every point of the ground at one address.
// Nothing is cached and no getter's table is touched: scratch of sd_prepare (sd_*) and buffers of its own (sf_*).
// Tile contexts (the tiled driver, include/vgs_tiles.h): a rank hands in one row per point of its OWN load (own point i = cloud point
// own_first + i) and only per-segment records travel.  k_sd_own_anchor (segdesc.hip) gives every global label's first own point,
// k_sf_anchor_own its values, k_sf_chunks_own / k_sf_hist_own run the chunk bodies over the own points only, k_sf_own_records folds the
// partials as k_sf_final does and leaves n, S1, S2, min and max as they are (vgs_get_own_segment_field_moments,
// vgs_get_own_segment_class_counts); the driver folds all ranks' records on the host and k_sf_final itself, over one partial per
// (segment, channel), finishes the table (vgs_segment_field_stats_from_moments).
// Host side: the drivers, uploads, copy-out and argument rules are attrpass.hpp's, one copy shared with pointfield.hip.  This file gives
// them the source of the node labelling (sf_source: sd_prepare, for a tile context with the own range), its launch lines and record rule
// (the attr_* specialisations for SdPrep) and the order of the checks (sf_check, then the table's own rules); the eight entry
// points of a table go through one function with an on_device flag (sf_field_entry, sf_hist_entry), a record set selecting the tile
// context's calls.  The folds' launch sites (sf_launch_*) are exported for both files' passes.
#include <string.h>

#include <algorithm>
#include <string>

#include "attrpass.hpp"

// anchor[k, c] for every channel: the value of the segment's first point in the chunk order, 0.0 where it is not finite.  One thread per entry.
__global__ __launch_bounds__(256) void k_sf_anchor(const float* __restrict__ field, int64_t stride_f, uint32_t C, const uint32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                   const uint32_t* __restrict__ seg_node, uint32_t K, double* __restrict__ anchor) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)K * C) return;
  const uint32_t k = (uint32_t)(t / C), ch = (uint32_t)(t % C);
  const uint32_t n0 = seg_node[k], n1 = seg_node[k + 1];
  double v = 0.0;
  if (n1 > n0) {
    const float x = field[(size_t)perm[vox_start[ids[n0]]] * (size_t)stride_f + ch];
    if (sf_valid(x)) v = (double)x;
  }
  anchor[t] = v;
}

// One workgroup per chunk, channels c0 .. c0 + ng - 1 (ng <= SF_G): one partial record per (chunk, channel of the group).  Grid: the bound
// of sd_prepare; workgroups past the real number of chunks leave at once.  OWN (tile contexts, k_sf_chunks_own): only the points whose
// input index o = perm[pos] lies in [own_first, own_end) count -- the selection of segdesc.hip's k_sd_chunks_own -- and their row is
// field + (o - own_first) * stride; a segment without an own point (anchor_pos[k] = 0xffffffff, from k_sd_own_anchor) writes the empty record.
__device__ __forceinline__ void sf_empty_record(double* __restrict__ rec) {
  if (threadIdx.x < SF_G * SF_REC) {
    const int f = threadIdx.x % SF_REC;
    rec[threadIdx.x] = f < 3 ? 0.0 : (f == 3 ? __builtin_huge_val() : -__builtin_huge_val());
  }
}

template <bool OWN>
__device__ __forceinline__ void sf_chunk_body(const float* __restrict__ field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng,
                                              const uint32_t* __restrict__ perm, const uint32_t* __restrict__ vox_start,
                                              const uint32_t* __restrict__ ids, const uint32_t* __restrict__ vp,
                                              const uint32_t* __restrict__ seg_node, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                              const double* __restrict__ anchor, double* __restrict__ part, int64_t own_first, int64_t own_end,
                                              const uint32_t* __restrict__ anchor_pos) {
  __shared__ uint32_t s_vp[SD_CHUNK];    // virtual start of the chunk's nodes
  __shared__ uint32_t s_dl[SD_CHUNK];    // sorted position - virtual position of the same (mod 2^32)
  SdChunk w;
  double* rec = part + (size_t)blockIdx.x * (SF_G * SF_REC);
  if (!sd_walk(vox_start, ids, vp, seg_node, seg_chunk, K, s_vp, s_dl, w)) {
    if (w.k != 0xffffffffu) sf_empty_record(rec);   // an empty record keeps the fold well defined
    return;
  }
  if (OWN && anchor_pos[w.k] == 0xffffffffu) {   // no own point in this segment: nothing counts
    sf_empty_record(rec);
    return;
  }
  double an[SF_G];
#pragma unroll
  for (int g = 0; g < SF_G; ++g) an[g] = (uint32_t)g < ng ? anchor[(size_t)w.k * C + c0 + g] : 0.0;
  sf_chunk_sums<OWN>(field, stride_f, c0, ng, w.a, w.b, an, [&](uint32_t q) { return sd_pos(s_vp, s_dl, w.m, q); }, perm, own_first, own_end, rec);
}

__global__ __launch_bounds__(SD_TB) void k_sf_chunks(const float* __restrict__ field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng,
                                                     const uint32_t* __restrict__ perm, const uint32_t* __restrict__ vox_start,
                                                     const uint32_t* __restrict__ ids, const uint32_t* __restrict__ vp,
                                                     const uint32_t* __restrict__ seg_node, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                                     const double* __restrict__ anchor, double* __restrict__ part) {
  sf_chunk_body<false>(field, stride_f, C, c0, ng, perm, vox_start, ids, vp, seg_node, seg_chunk, K, anchor, part, 0, 0, nullptr);
}

__global__ __launch_bounds__(SD_TB) void k_sf_chunks_own(const float* __restrict__ field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng,
                                                         const uint32_t* __restrict__ perm, const uint32_t* __restrict__ vox_start,
                                                         const uint32_t* __restrict__ ids, const uint32_t* __restrict__ vp,
                                                         const uint32_t* __restrict__ seg_node, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                                         const double* __restrict__ anchor, double* __restrict__ part, int64_t own_first,
                                                         int64_t own_end, const uint32_t* __restrict__ anchor_pos) {
  sf_chunk_body<true>(field, stride_f, C, c0, ng, perm, vox_start, ids, vp, seg_node, seg_chunk, K, anchor, part, own_first, own_end, anchor_pos);
}

// Tile contexts: anchor[k, c] for every channel = the value of the segment's first own point in the chunk order (anchor_pos[k], from
// k_sd_own_anchor), 0.0 where that value is not finite and for a segment without an own point.  One thread per entry.
__global__ __launch_bounds__(256) void k_sf_anchor_own(const float* __restrict__ field, int64_t stride_f, uint32_t C, const uint32_t* __restrict__ perm,
                                                       const uint32_t* __restrict__ anchor_pos, int64_t own_first, int64_t own_end, uint32_t K,
                                                       double* __restrict__ anchor) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)K * C) return;
  const uint32_t k = (uint32_t)(t / C), ch = (uint32_t)(t % C);
  const uint32_t pa = anchor_pos[k];
  double v = 0.0;
  if (pa != 0xffffffffu) {
    const int64_t o = (int64_t)perm[pa];
    if (o >= own_first && o < own_end) {   // (k_sd_own_anchor's own selection: the test only guards the read)
      const float x = field[(size_t)(o - own_first) * (size_t)stride_f + ch];
      if (sf_valid(x)) v = (double)x;
    }
  }
  anchor[t] = v;
}

// the fold of one (segment, channel of the group) over its chunk partials, on one wavefront: lane stride, then butterfly
__device__ __forceinline__ void sf_fold_partials(const uint32_t* seg_chunk, const double* part, uint32_t n_part, uint32_t k,
                                                 uint32_t g, uint32_t lane, double& s1, double& s2, double& cn, double& mn, double& mx) {
  const uint32_t q0 = seg_chunk[k], q1 = min(seg_chunk[k + 1], n_part);   // (the bound only guards the records: the chunks fit, see the launch)
  s1 = 0.0; s2 = 0.0; cn = 0.0; mn = __builtin_huge_val(); mx = -__builtin_huge_val();
  for (uint32_t c = q0 + lane; c < q1; c += 64) {
    const double* r = part + ((size_t)c * SF_G + g) * SF_REC;
    s1 += r[0]; s2 += r[1]; cn += r[2];
    mn = fmin(mn, r[3]); mx = fmax(mx, r[4]);
  }
  s1 = sf_wave_sum(s1); s2 = sf_wave_sum(s2); cn = sf_wave_sum(cn);
  mn = sf_wave_min(mn); mx = sf_wave_max(mx);
}

// one wavefront per (segment, channel of the group): fold the partials (lane stride, then butterfly), then the row's entries on lane 0
__global__ __launch_bounds__(256) void k_sf_final(const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part, uint32_t n_part, uint32_t K,
                                                  uint32_t C, uint32_t c0, uint32_t ng, const double* __restrict__ anchor,
                                                  int64_t* __restrict__ o_n, double* __restrict__ o_mean, double* __restrict__ o_var,
                                                  float* __restrict__ o_min, float* __restrict__ o_max) {
  const uint64_t wi = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (wi >= (uint64_t)K * ng) return;   // (whole wavefronts; no barrier follows)
  const uint32_t k = (uint32_t)(wi / ng), g = (uint32_t)(wi % ng);
  double s1, s2, cn, mn, mx;
  sf_fold_partials(seg_chunk, part, n_part, k, g, lane, s1, s2, cn, mn, mx);
  if (lane != 0) return;
  const size_t o = (size_t)k * C + c0 + g;
  o_n[o] = (int64_t)cn;
  if (cn > 0.0) {
    const double m1 = s1 / cn;
    const double v = s2 / cn - m1 * m1;
    o_mean[o] = anchor[o] + m1;
    o_var[o] = v > 0.0 ? v : 0.0;
    o_min[o] = (float)mn;
    o_max[o] = (float)mx;
  } else {
    o_mean[o] = __builtin_nan(""); o_var[o] = __builtin_nan("");
    o_min[o] = __builtin_nanf(""); o_max[o] = __builtin_nanf("");
  }
}

// Tile contexts: the fold of k_sf_final over the partials of k_sf_chunks_own, the sums left as they are -- one wavefront per (segment,
// channel of the group) writes n, S1, S2, min and max of the rank's own points (0, 0, 0, +inf, -inf without a valid value).
__global__ __launch_bounds__(256) void k_sf_own_records(const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part, uint32_t n_part,
                                                        uint32_t K, uint32_t C, uint32_t c0, uint32_t ng, int64_t* __restrict__ o_n,
                                                        double* __restrict__ o_s1, double* __restrict__ o_s2, float* __restrict__ o_min,
                                                        float* __restrict__ o_max) {
  const uint64_t wi = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (wi >= (uint64_t)K * ng) return;   // (whole wavefronts; no barrier follows)
  const uint32_t k = (uint32_t)(wi / ng), g = (uint32_t)(wi % ng);
  double s1, s2, cn, mn, mx;
  sf_fold_partials(seg_chunk, part, n_part, k, g, lane, s1, s2, cn, mn, mx);
  if (lane != 0) return;
  const size_t o = (size_t)k * C + c0 + g;
  o_n[o] = (int64_t)cn; o_s1[o] = s1; o_s2[o] = s2;
  o_min[o] = (float)mn; o_max[o] = (float)mx;
}

// One workgroup per chunk: the classes of its points counted in LDS (slot n_classes: out of range), the non-zero counters added to the
// zeroed tables.  hist: K x n_classes, n_outside: K.  Integer atomics: the sums do not depend on the order.  OWN (tile contexts,
// k_sf_hist_own): only the points whose input index o = perm[pos] lies in [own_first, own_end) count, and their class is cls[o - own_first].
// the walk of sf_hist_chunk over the node labelling: sd_walk stages the chunk's nodes, sd_pos finds a virtual point
struct SfNodeWalk {
  const uint32_t *vox_start, *ids, *vp, *seg_node, *seg_chunk;
  uint32_t K;
  uint32_t *s_vp, *s_dl;
  SdChunk w;
  __device__ __forceinline__ bool begin(uint32_t& k, uint32_t& a, uint32_t& b) {
    if (!sd_walk(vox_start, ids, vp, seg_node, seg_chunk, K, s_vp, s_dl, w)) return false;
    k = w.k; a = w.a; b = w.b;
    return true;
  }
  __device__ __forceinline__ uint32_t pos(uint32_t q) const { return sd_pos(s_vp, s_dl, w.m, q); }
};
template <bool OWN>
__device__ __forceinline__ void sf_hist_body(const int32_t* __restrict__ cls, uint32_t n_classes, const uint32_t* __restrict__ perm,
                                             const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                             const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                             const uint32_t* __restrict__ seg_chunk, uint32_t K, unsigned long long* __restrict__ hist,
                                             unsigned long long* __restrict__ n_outside, int64_t own_first, int64_t own_end) {
  __shared__ uint32_t s_vp[SD_CHUNK];
  __shared__ uint32_t s_dl[SD_CHUNK];
  sf_hist_chunk<OWN>(cls, n_classes, perm, SfNodeWalk{vox_start, ids, vp, seg_node, seg_chunk, K, s_vp, s_dl, {}}, hist, n_outside, own_first, own_end);
}

__global__ __launch_bounds__(SD_TB) void k_sf_hist(const int32_t* __restrict__ cls, uint32_t n_classes, const uint32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                   const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                                   const uint32_t* __restrict__ seg_chunk, uint32_t K, unsigned long long* __restrict__ hist,
                                                   unsigned long long* __restrict__ n_outside) {
  sf_hist_body<false>(cls, n_classes, perm, vox_start, ids, vp, seg_node, seg_chunk, K, hist, n_outside, 0, 0);
}

__global__ __launch_bounds__(SD_TB) void k_sf_hist_own(const int32_t* __restrict__ cls, uint32_t n_classes, const uint32_t* __restrict__ perm,
                                                       const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                       const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                                       const uint32_t* __restrict__ seg_chunk, uint32_t K, unsigned long long* __restrict__ hist,
                                                       unsigned long long* __restrict__ n_outside, int64_t own_first, int64_t own_end) {
  sf_hist_body<true>(cls, n_classes, perm, vox_start, ids, vp, seg_node, seg_chunk, K, hist, n_outside, own_first, own_end);
}

// one wavefront per segment: the lowest class with the largest count (-1 and 0 when every count is 0)
__global__ __launch_bounds__(256) void k_sf_majority(const unsigned long long* __restrict__ hist, uint32_t n_classes, uint32_t K,
                                                     int32_t* __restrict__ majority, long long* __restrict__ majority_count) {
  const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= K) return;   // (whole wavefronts; no barrier follows)
  unsigned long long best = 0;
  uint32_t arg = 0xffffffffu;
  for (uint32_t j = lane; j < n_classes; j += 64) {   // ascending j per lane: a strictly larger count only
    const unsigned long long v = hist[(size_t)k * n_classes + j];
    if (v > best) { best = v; arg = j; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long ob = __shfl_xor(best, m, 64);
    const uint32_t oa = __shfl_xor(arg, m, 64);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (lane != 0) return;
  majority[k] = best > 0 ? (int32_t)arg : -1;
  majority_count[k] = (long long)best;
}

// ---------------------------------------------------------------------------------------------------------------------- host
// the launch sites of the folds, for the drivers of attrpass.hpp: k_sf_final and, for tile contexts, k_sf_own_records over the partials
// of one channel group, k_sf_majority over a K x n_classes table; left on the context's stream
void sf_launch_final(vgs_ctx* c, const uint32_t* seg_chunk, const double* part, uint32_t n_part, int64_t K, uint32_t C, uint32_t c0, uint32_t ng,
                     const double* anchor, int64_t* o_n, double* o_mean, double* o_var, float* o_min, float* o_max) {
  hipLaunchKernelGGL(k_sf_final, dim3((unsigned)(((size_t)K * ng + 3) / 4)), dim3(256), 0, c->stream, seg_chunk, part, n_part, (uint32_t)K, C, c0, ng, anchor,
                     o_n, o_mean, o_var, o_min, o_max);
}
void sf_launch_own_records(vgs_ctx* c, const uint32_t* seg_chunk, const double* part, uint32_t n_part, int64_t K, uint32_t C, uint32_t c0, uint32_t ng,
                           int64_t* o_n, double* o_s1, double* o_s2, float* o_min, float* o_max) {
  hipLaunchKernelGGL(k_sf_own_records, dim3((unsigned)(((size_t)K * ng + 3) / 4)), dim3(256), 0, c->stream, seg_chunk, part, n_part, (uint32_t)K, C, c0, ng,
                     o_n, o_s1, o_s2, o_min, o_max);
}
void sf_launch_majority(vgs_ctx* c, const int64_t* hist, int32_t n_classes, int64_t K, int32_t* majority, int64_t* majority_count) {
  hipLaunchKernelGGL(k_sf_majority, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, c->stream, (const unsigned long long*)hist, (uint32_t)n_classes,
                     (uint32_t)K, majority, (long long*)majority_count);
}

// The source of the node labelling (attrpass.hpp): sd_prepare for the labels 0 .. K-1 of vox_label -- one context: its kept segments; a
// tile context (own): the global labels after vgs_apply_tile_labels, only the own points counting.  Without a segment, a voxel or a point
// in the octree nothing is written.  A tile context's first own points (sd_own_anchor into sd_apos) are queued by the first launch below.
static vgs_status sf_source(vgs_ctx* c, int64_t K, bool own, AttrSource<SdPrep>& S) {
  S.K = K;
  S.own = own;
  if (K == 0 || c->V == 0 || c->Nf == 0) return VGS_OK;
  vgs_status s = sd_prepare(c, K, S.d);
  if (s != VGS_OK) return s;
  S.seg_chunk = S.d.seg_chunk;
  S.n_chunks_max = S.d.n_chunks_max;
  S.live = S.chunks = true;
  if (own) { S.own_first = c->own_first; S.own_end = c->own_first + c->n_own; }
  return VGS_OK;
}

template <> vgs_status attr_launch_anchor<SdPrep>(vgs_ctx* c, const AttrSource<SdPrep>& S, const float* field, int64_t stride_f, uint32_t C) {
  const dim3 grid((unsigned)(((size_t)S.K * C + 255) / 256));
  if (!S.own) {
    hipLaunchKernelGGL(k_sf_anchor, grid, dim3(256), 0, c->stream, field, stride_f, C, c->perm_b.p, c->vox_start.p, S.d.ids, S.d.seg_node, (uint32_t)S.K,
                       c->sf_anchor.p);
    return VGS_OK;
  }
  vgs_status s = sd_own_anchor(c, S.K, S.d);
  if (s != VGS_OK) return s;
  hipLaunchKernelGGL(k_sf_anchor_own, grid, dim3(256), 0, c->stream, field, stride_f, C, c->perm_b.p, c->sd_apos.p, S.own_first, S.own_end, (uint32_t)S.K,
                     c->sf_anchor.p);
  return VGS_OK;
}

template <> void attr_launch_chunks<SdPrep>(vgs_ctx* c, const AttrSource<SdPrep>& S, const float* field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng) {
  const dim3 grid((unsigned)S.n_chunks_max);
  if (S.own)
    hipLaunchKernelGGL(k_sf_chunks_own, grid, dim3(SD_TB), 0, c->stream, field, stride_f, C, c0, ng, c->perm_b.p, c->vox_start.p, S.d.ids, S.d.vp, S.d.seg_node,
                       S.d.seg_chunk, (uint32_t)S.K, c->sf_anchor.p, c->sf_part.p, S.own_first, S.own_end, c->sd_apos.p);
  else
    hipLaunchKernelGGL(k_sf_chunks, grid, dim3(SD_TB), 0, c->stream, field, stride_f, C, c0, ng, c->perm_b.p, c->vox_start.p, S.d.ids, S.d.vp, S.d.seg_node,
                       S.d.seg_chunk, (uint32_t)S.K, c->sf_anchor.p, c->sf_part.p);
}

template <> vgs_status attr_launch_hist<SdPrep>(vgs_ctx* c, const AttrSource<SdPrep>& S, const int32_t* cls, uint32_t n_classes, unsigned long long* hist,
                                   unsigned long long* n_outside) {
  const dim3 grid((unsigned)S.n_chunks_max);
  if (!S.own) {
    hipLaunchKernelGGL(k_sf_hist, grid, dim3(SD_TB), 0, c->stream, cls, n_classes, c->perm_b.p, c->vox_start.p, S.d.ids, S.d.vp, S.d.seg_node, S.d.seg_chunk,
                       (uint32_t)S.K, hist, n_outside);
    return VGS_OK;
  }
  vgs_status s = sd_own_anchor(c, S.K, S.d);   // (the record rule reads sd_apos)
  if (s != VGS_OK) return s;
  hipLaunchKernelGGL(k_sf_hist_own, grid, dim3(SD_TB), 0, c->stream, cls, n_classes, c->perm_b.p, c->vox_start.p, S.d.ids, S.d.vp, S.d.seg_node, S.d.seg_chunk,
                     (uint32_t)S.K, hist, n_outside, S.own_first, S.own_end);
  return VGS_OK;
}

// the labels with an own labelled point leave a record: sd_apos[k] != 0xffffffff (the label set of vgs_get_own_segment_extents)
template <> size_t attr_rule_words<SdPrep>(vgs_ctx* c, const AttrSource<SdPrep>& S, const uint32_t** dev) { *dev = c->sd_apos.p; return (size_t)S.K; }
template <> bool attr_has_record<SdPrep>(const AttrSource<SdPrep>&, const uint32_t* apos, size_t k) { return apos[k] != 0xffffffffu; }

// The rules both tables share, in this family's order.  own: the calls of a tile context, K the global label count and n the rank's own
// points; otherwise one context with the whole cloud.
static vgs_status sf_check(vgs_ctx* c, const char* fn, bool own, int64_t K, const void* in, int64_t n) {
  vgs_status s = attr_check_segmented(c, fn);
  if (s != VGS_OK) return s;
  if (own) {
    if ((s = attr_check_tile_only(c, fn)) != VGS_OK || (s = attr_check_K(c, fn, K, (int64_t)0xfffffffeLL)) != VGS_OK) return s;
    s = attr_check_n(c, fn, "n_own", n, "own points of the context", c->n_own);
  } else {
    if (vgs_is_tile(c))
      return attr_fail(c, fn, VGS_E_STATE, "a tile context (owned region / own point range) holds only part of its segments; field statistics need the whole cloud in one context");
    s = attr_check_n(c, fn, "n", n, "points of the cloud", c->N);
  }
  return s != VGS_OK ? s : attr_check_array(c, fn, "the input array", in, n);
}

// The eight entry points of a table come through one function.  R = NULL: one context, K its kept count, dense rows.  R given: a tile
// context, K the caller's, compact records (n_records is required and zeroed once the arguments hold).  A host variant without a segment
// or a point returns before the device is touched.
static vgs_status sf_field_run(vgs_ctx* c, bool on_device, int64_t K, const float* field, int64_t n, int32_t n_channels, int64_t stride_bytes,
                               const AttrRecords* R, const AttrFieldOut& O) {
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  vgs_status s = on_device ? VGS_OK : attr_upload_field(c, &field, n, n_channels, stride_bytes);
  AttrSource<SdPrep> S;
  if (s != VGS_OK || (s = sf_source(c, K, R != nullptr, S)) != VGS_OK) return s;
  return attr_field_table(c, S, field, n_channels, stride_bytes, R, O);
}

static vgs_status sf_field_entry(vgs_ctx* c, const char* fn, bool on_device, int64_t K, const float* field, int64_t n, int32_t n_channels,
                                 int64_t stride_bytes, const AttrRecords* R, const AttrFieldOut& O) {
  if (!c || (R && !R->n_records)) return VGS_E_ARG;
  if (!R) K = c->counts[VGS_N_KEPT];
  vgs_status s = sf_check(c, fn, R != nullptr, K, field, n);
  if (s != VGS_OK || (s = attr_check_channels(c, fn, n_channels)) != VGS_OK || (s = attr_check_stride(c, fn, n_channels, stride_bytes)) != VGS_OK) return s;
  if (R) *R->n_records = 0;
  if (!on_device && (K == 0 || n == 0)) return VGS_OK;
  return attr_settle(c, sf_field_run(c, on_device, K, field, n, n_channels, stride_bytes, R, O));
}

static vgs_status sf_hist_run(vgs_ctx* c, bool on_device, int64_t K, const int32_t* cls, int64_t n, int32_t n_classes, const AttrRecords* R,
                              const AttrHistOut& O) {
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  vgs_status s = on_device ? VGS_OK : attr_upload_classes(c, &cls, n);
  AttrSource<SdPrep> S;
  if (s != VGS_OK || (s = sf_source(c, K, R != nullptr, S)) != VGS_OK) return s;
  return attr_hist_table(c, S, cls, n_classes, R, O);
}

static vgs_status sf_hist_entry(vgs_ctx* c, const char* fn, bool on_device, int64_t K, const int32_t* cls, int64_t n, int32_t n_classes,
                                const AttrRecords* R, const AttrHistOut& O) {
  if (!c || (R && !R->n_records)) return VGS_E_ARG;
  if (!R) K = c->counts[VGS_N_KEPT];
  vgs_status s = sf_check(c, fn, R != nullptr, K, cls, n);
  if (s != VGS_OK || (s = attr_check_classes(c, fn, n_classes)) != VGS_OK ||
      (s = attr_check_limit(c, fn, K, "segments", n_classes, "classes", "counters")) != VGS_OK)
    return s;
  if (R) *R->n_records = 0;
  if (!on_device && (K == 0 || n == 0)) return VGS_OK;
  return attr_settle(c, sf_hist_run(c, on_device, K, cls, n, n_classes, R, O));
}

extern "C" vgs_status vgs_segment_field_stats(vgs_ctx* c, const float* field_host, int64_t n, int32_t n_channels, int64_t stride_bytes,
                                              int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax) {
  return sf_field_entry(c, "vgs_segment_field_stats", false, 0, field_host, n, n_channels, stride_bytes, nullptr, {n_valid, anchor, mean, var, vmin, vmax});
}

extern "C" vgs_status vgs_segment_field_stats_device(vgs_ctx* c, const float* field_dev, int64_t n, int32_t n_channels, int64_t stride_bytes,
                                                     int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax) {
  return sf_field_entry(c, "vgs_segment_field_stats_device", true, 0, field_dev, n, n_channels, stride_bytes, nullptr, {n_valid, anchor, mean, var, vmin, vmax});
}

extern "C" vgs_status vgs_segment_class_histogram(vgs_ctx* c, const int32_t* cls_host, int64_t n, int32_t n_classes, int64_t* hist,
                                                  int64_t* n_outside, int32_t* majority, int64_t* majority_count) {
  return sf_hist_entry(c, "vgs_segment_class_histogram", false, 0, cls_host, n, n_classes, nullptr, {hist, n_outside, majority, majority_count});
}

extern "C" vgs_status vgs_segment_class_histogram_device(vgs_ctx* c, const int32_t* cls_dev, int64_t n, int32_t n_classes, int64_t* hist,
                                                         int64_t* n_outside, int32_t* majority, int64_t* majority_count) {
  return sf_hist_entry(c, "vgs_segment_class_histogram_device", true, 0, cls_dev, n, n_classes, nullptr, {hist, n_outside, majority, majority_count});
}

// ------------------------------------------------------------------------------------------------ tile contexts (include/vgs_tiles.h)
// This rank's moments and class counts of the global labels 0 .. K-1 over its own points, n_own rows: dense on the device, compact on the host.
extern "C" vgs_status vgs_get_own_segment_field_moments(vgs_ctx* c, int64_t K, const float* field_host, int64_t n_own, int32_t n_channels,
                                                        int64_t stride_bytes, int64_t* n_records, int32_t* label, int64_t* n_valid, double* anchor,
                                                        double* s1, double* s2, float* vmin, float* vmax) {
  const AttrRecords R = {n_records, label};
  return sf_field_entry(c, "vgs_get_own_segment_field_moments", false, K, field_host, n_own, n_channels, stride_bytes, &R, {n_valid, anchor, s1, s2, vmin, vmax});
}

extern "C" vgs_status vgs_get_own_segment_field_moments_device(vgs_ctx* c, int64_t K, const float* field_dev, int64_t n_own, int32_t n_channels,
                                                               int64_t stride_bytes, int64_t* n_records, int32_t* label, int64_t* n_valid,
                                                               double* anchor, double* s1, double* s2, float* vmin, float* vmax) {
  const AttrRecords R = {n_records, label};
  return sf_field_entry(c, "vgs_get_own_segment_field_moments_device", true, K, field_dev, n_own, n_channels, stride_bytes, &R,
                        {n_valid, anchor, s1, s2, vmin, vmax});
}

extern "C" vgs_status vgs_get_own_segment_class_counts(vgs_ctx* c, int64_t K, const int32_t* cls_host, int64_t n_own, int32_t n_classes,
                                                       int64_t* n_records, int32_t* label, int64_t* hist, int64_t* n_outside) {
  const AttrRecords R = {n_records, label};
  return sf_hist_entry(c, "vgs_get_own_segment_class_counts", false, K, cls_host, n_own, n_classes, &R, {hist, n_outside, nullptr, nullptr});
}

extern "C" vgs_status vgs_get_own_segment_class_counts_device(vgs_ctx* c, int64_t K, const int32_t* cls_dev, int64_t n_own, int32_t n_classes,
                                                              int64_t* n_records, int32_t* label, int64_t* hist, int64_t* n_outside) {
  const AttrRecords R = {n_records, label};
  return sf_hist_entry(c, "vgs_get_own_segment_class_counts_device", true, K, cls_dev, n_own, n_classes, &R, {hist, n_outside, nullptr, nullptr});
}

// The table from moments folded over the ranks: one partial record per (segment, channel) and seg_chunk[k] = k, so k_sf_final itself runs
// unchanged -- its fold over one record adds zeros, its tail is the arithmetic of vgs_segment_field_stats.  Records of all channel groups
// in one upload, group after group.
extern "C" vgs_status vgs_segment_field_stats_from_moments(vgs_ctx* c, int64_t K, int32_t n_channels, const int64_t* n_valid, const double* anchor,
                                                           const double* s1, const double* s2, const float* vmin, const float* vmax, double* mean,
                                                           double* var, float* vmin_out, float* vmax_out) {
  if (!c || K < 0 || K >= (int64_t)0xffffffffLL) return VGS_E_ARG;
  vgs_status s = attr_check_channels(c, "vgs_segment_field_stats_from_moments", n_channels);
  if (s != VGS_OK) return s;
  if (K > 0 && (!n_valid || !anchor || !s1 || !s2 || !vmin || !vmax)) { c->err = "vgs_segment_field_stats_from_moments: an input array is NULL"; return VGS_E_ARG; }
  if (K == 0) return VGS_OK;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t C = (uint32_t)n_channels, n_groups = (C + SF_G - 1) / SF_G;
  const size_t k = (size_t)K, kc = k * C, per_group = k * SF_G * SF_REC;
  std::vector<double> part((size_t)n_groups * per_group, 0.0);
  for (size_t i = 0; i < k; ++i)
    for (uint32_t ch = 0; ch < C; ++ch) {
      double* r = part.data() + (size_t)(ch / SF_G) * per_group + (i * SF_G + ch % SF_G) * SF_REC;
      const size_t o = i * C + ch;
      r[0] = s1[o]; r[1] = s2[o]; r[2] = (double)n_valid[o]; r[3] = (double)vmin[o]; r[4] = (double)vmax[o];
    }
  std::vector<uint32_t> idx(k + 1);
  for (size_t i = 0; i <= k; ++i) idx[i] = (uint32_t)i;
  VGS_HIP_TRY(c, c->sf_part.ensure(part.size())); VGS_HIP_TRY(c, c->sf_idx.ensure(idx.size()));
  if ((s = attr_ensure_field_rows(c, kc)) != VGS_OK) return s;
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_part.p, part.data(), part.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_anchor.p, anchor, kc * sizeof(double), hipMemcpyHostToDevice, c->stream));
  for (uint32_t c0 = 0; c0 < C; c0 += SF_G) {
    const uint32_t ng = C - c0 < SF_G ? C - c0 : SF_G;
    sf_launch_final(c, c->sf_idx.p, c->sf_part.p + (size_t)(c0 / SF_G) * per_group, (uint32_t)K, K, C, c0, ng, c->sf_anchor.p, c->sf_nvalid.p, c->sf_mean.p,
                    c->sf_var.p, c->sf_min.p, c->sf_max.p);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  const RowCol col[4] = {{mean, c->sf_mean.p, C * sizeof(double)}, {var, c->sf_var.p, C * sizeof(double)},
                          {vmin_out, c->sf_min.p, C * sizeof(float)}, {vmax_out, c->sf_max.p, C * sizeof(float)}};
  return vgs_copy_rows(c, k, col, 4);   // (its wait frees the staged records and the caller's anchor as well)
}
