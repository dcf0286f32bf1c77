// pointfield.hip -- field statistics and class histograms of a per-POINT labelling of the context's cloud that the CALLER supplies
// (include/vgs.h: vgs_point_label_field_stats, vgs_point_label_class_histogram): the two attribute tables of segfield.hip for the refined
// labels, ground-truth instances, anything made from the engine's output.  segfield.hip walks whole nodes (sd_prepare), so it cannot
// express a boundary voxel that holds two or three labels; here the points themselves are sorted, as pointseg.hip sorts them for the
// descriptors.  Row k covers the points i with labels[i] == k that are in the octree -- the set vgs_point_label_descriptors counts in
// n_points; the row fields and the arithmetic are those of the node tables.
//
// Data flow (perm_b gives the input index of a sorted position; the attribute arrays are in input order):
//   1. ps_sort_points (pointseg.hip), ONCE per call whatever the number of channels: the range check, one stable radix sort of the octree
//      positions by label -> pos_sorted, per label the start of its run and its first chunk of SD_CHUNK points; a label without a point
//      has no chunk
//   2. k_pf_anchor   one thread per (label, channel): the value of the label's first point in that order,
//                    field[perm_b[pos_sorted[seg_start[k]]]], as a double; 0.0 where it is not finite and for a label without a point
//   3. k_pf_chunks   per group of SF_G channels, one workgroup per chunk (ps_walk): sf_chunk_sums (segpass.hpp, the body k_sf_chunks
//                    runs) with the point of a lane pos_sorted[a + it * SD_TB + tid]
//   4. k_sf_final    (segfield.hip, through sf_launch_final) the fold of the partials and the row entries -- the one copy of both.  The
//                    workgroups past a label's real chunks do not exist here, so the fold of a label without a point is the empty one
//                    (seg_chunk[k] == seg_chunk[k + 1]): n_valid 0 and NaN
//   histogram: k_pf_hist, one workgroup per chunk: sf_hist_chunk (the body k_sf_hist runs) over pos_sorted, integer adds of its
//   non-zero counters to the zeroed K x n_classes table; k_sf_majority (segfield.hip, through sf_launch_majority)
// Determinism: which point a lane reads depends on (chunk, lane, step) only, every fold has a fixed shape, no float atomics -- the tables
// are bit-identical from call to call and engine to engine.  And for a labelling that is constant on nodes the stable sort gives
// sd_prepare's virtual point sequence (pointseg.hip's argument), hence the same chunks a + it * SD_TB + tid, the same anchor and, the
// arithmetic being the same code, the same bytes: handed the context's own point labels with K = the kept count, the two calls return
// vgs_segment_field_stats and vgs_segment_class_histogram byte for byte.
// Scratch: the sort's (ps_*) and the tables and partials of segfield.hip (sf_*); nothing a getter or a cached table reads.  Nothing is
// cached: the input is the caller's.
// Tile contexts (the tiled driver, include/vgs_tiles.h; the entry points at the end of this file): a rank hands in one label and one row per
// point of its OWN load (own point i = cloud point own_first + i) and only per-label records travel.  ps_sort_points sorts the own points
// alone (k_ps_keys gives every other position the key K), so the anchor, the chunks and the folds see own points only; the row of a point
// is field + (perm_b[pos] - own_first) * stride.  The same kernel bodies with OWN = true (k_pf_own_chunks, k_pf_own_hist), k_pf_anchor with
// the own range's start, and k_sf_own_records (segfield.hip, through sf_launch_own_records) in place of k_sf_final: the sums leave as they
// are (vgs_own_point_label_field_moments, vgs_own_point_label_class_counts), the driver folds all ranks' records on the host and
// vgs_segment_field_stats_from_moments finishes the table.
// Host side: the drivers, uploads, copy-out and argument rules are attrpass.hpp's, one copy shared with segfield.hip.  This file gives them
// the source of a point labelling (pf_source: ps_sort_points over the cloud or over the own range), its launch lines and record rule (the
// attr_* specialisations for PsSort) and the order of the checks (pf_check, then the table's own rules); the eight entry points of a
// table go through one function with an on_device flag (pf_field_entry, pf_hist_entry), a record set selecting the tile context's calls.
// After a failure too an entry waits for the stream (attr_settle): arrays read in place are the caller's again.
#include <string.h>

#include <algorithm>
#include <string>

#include "attrpass.hpp"

// Step 2.  One thread per (label, channel).  row0: the input index of the field's first row (0; a tile context: own_first -- the sorted
// points are own points there, so the row index is never negative).
__global__ __launch_bounds__(256) void k_pf_anchor(const float* __restrict__ field, int64_t stride_f, uint32_t C, const uint32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ seg_start, uint32_t K,
                                                   int64_t row0, double* __restrict__ anchor) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)K * C) return;
  const uint32_t k = (uint32_t)(t / C), ch = (uint32_t)(t % C);
  const uint32_t s0 = seg_start[k];
  double v = 0.0;
  if (seg_start[k + 1] > s0) {
    const float x = field[(size_t)((int64_t)perm[pos_sorted[s0]] - row0) * (size_t)stride_f + ch];
    if (sf_valid(x)) v = (double)x;
  }
  anchor[t] = v;
}

// Step 3.  Grid: the bound of ps_sort_points; workgroups past the real number of chunks leave at once (whole workgroups, before any
// barrier) and write nothing -- no fold reads their records.  OWN (k_pf_own_chunks, tile contexts): pos_sorted holds own points only and
// the row of a point is field + (perm[pos] - own_first) * stride (sf_chunk_sums<true>; its own-range test guards the read).
template <bool OWN>
__device__ __forceinline__ void pf_chunk_body(const float* __restrict__ field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng,
                                              const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pos_sorted,
                                              const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                              const double* __restrict__ anchor, double* __restrict__ part, int64_t own_first, int64_t own_end) {
  PsChunk wk;
  if (!ps_walk(seg_start, seg_chunk, K, wk)) return;
  double an[SF_G];
#pragma unroll
  for (int g = 0; g < SF_G; ++g) an[g] = (uint32_t)g < ng ? anchor[(size_t)wk.k * C + c0 + g] : 0.0;
  sf_chunk_sums<OWN>(field, stride_f, c0, ng, wk.a, wk.b, an, [&](uint32_t q) { return pos_sorted[q]; }, perm, own_first, own_end,
                     part + (size_t)blockIdx.x * (SF_G * SF_REC));
}

__global__ __launch_bounds__(SD_TB) void k_pf_chunks(const float* __restrict__ field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng,
                                                     const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pos_sorted,
                                                     const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                                     const double* __restrict__ anchor, double* __restrict__ part) {
  pf_chunk_body<false>(field, stride_f, C, c0, ng, perm, pos_sorted, seg_start, seg_chunk, K, anchor, part, 0, 0);
}

__global__ __launch_bounds__(SD_TB) void k_pf_own_chunks(const float* __restrict__ field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng,
                                                         const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pos_sorted,
                                                         const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_chunk, uint32_t K,
                                                         const double* __restrict__ anchor, double* __restrict__ part, int64_t own_first,
                                                         int64_t own_end) {
  pf_chunk_body<true>(field, stride_f, C, c0, ng, perm, pos_sorted, seg_start, seg_chunk, K, anchor, part, own_first, own_end);
}

// The histogram's chunks: the same grid, the same walk, as the walk object of sf_hist_chunk (nothing to stage: pos_sorted is in HBM).
struct PfWalk {
  const uint32_t *pos_sorted, *seg_start, *seg_chunk;
  uint32_t K;
  __device__ __forceinline__ bool begin(uint32_t& k, uint32_t& a, uint32_t& b) const {
    PsChunk wk;
    if (!ps_walk(seg_start, seg_chunk, K, wk)) return false;
    k = wk.k; a = wk.a; b = wk.b;
    return true;
  }
  __device__ __forceinline__ uint32_t pos(uint32_t q) const { return pos_sorted[q]; }
};
__global__ __launch_bounds__(SD_TB) void k_pf_hist(const int32_t* __restrict__ cls, uint32_t n_classes, const uint32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ seg_start,
                                                   const uint32_t* __restrict__ seg_chunk, uint32_t K, unsigned long long* __restrict__ hist,
                                                   unsigned long long* __restrict__ n_outside) {
  sf_hist_chunk<false>(cls, n_classes, perm, PfWalk{pos_sorted, seg_start, seg_chunk, K}, hist, n_outside, 0, 0);
}
// tile contexts: the class of an own point is cls[perm[pos] - own_first]
__global__ __launch_bounds__(SD_TB) void k_pf_own_hist(const int32_t* __restrict__ cls, uint32_t n_classes, const uint32_t* __restrict__ perm,
                                                       const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ seg_start,
                                                       const uint32_t* __restrict__ seg_chunk, uint32_t K, unsigned long long* __restrict__ hist,
                                                       unsigned long long* __restrict__ n_outside, int64_t own_first, int64_t own_end) {
  sf_hist_chunk<true>(cls, n_classes, perm, PfWalk{pos_sorted, seg_start, seg_chunk, K}, hist, n_outside, own_first, own_end);
}

// ---------------------------------------------------------------------------------------------------------------------- host
// The source of a caller's per-point labelling (attrpass.hpp): ps_sort_points over labels_dev -- one context: the whole cloud; a tile
// context (own): its own point range alone, one label per own point.  K = 0 (nothing sorted): validated, the skipped points counted,
// nothing to write.  No point in the octree: one context still writes the empty rows, a tile context has no record.
static vgs_status pf_source(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, bool own, int64_t* n_skipped, AttrSource<PsSort>& S) {
  S.K = K;
  S.own = own;
  S.own_first = own ? c->own_first : 0;
  S.own_end = S.own_first + (own ? c->n_own : c->N);
  vgs_status s = ps_sort_points(c, fn, labels_dev, S.own_first, S.own_end - S.own_first, K, 0, n_skipped, S.d);
  if (s != VGS_OK || !S.d.sorted) return s;
  S.seg_chunk = S.d.seg_chunk;
  S.n_chunks_max = S.d.n_chunks_max;
  S.chunks = c->Nf > 0;
  S.live = S.chunks || !own;
  return VGS_OK;
}

// row0 of k_pf_anchor is the source's own_first: 0 for one context
template <> vgs_status attr_launch_anchor<PsSort>(vgs_ctx* c, const AttrSource<PsSort>& S, const float* field, int64_t stride_f, uint32_t C) {
  hipLaunchKernelGGL(k_pf_anchor, dim3((unsigned)(((size_t)S.K * C + 255) / 256)), dim3(256), 0, c->stream, field, stride_f, C, c->perm_b.p, S.d.pos,
                     S.d.seg_start, (uint32_t)S.K, S.own_first, c->sf_anchor.p);
  return VGS_OK;
}

template <> void attr_launch_chunks<PsSort>(vgs_ctx* c, const AttrSource<PsSort>& S, const float* field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng) {
  const dim3 grid((unsigned)S.n_chunks_max);
  if (S.own)
    hipLaunchKernelGGL(k_pf_own_chunks, grid, dim3(SD_TB), 0, c->stream, field, stride_f, C, c0, ng, c->perm_b.p, S.d.pos, S.d.seg_start, S.d.seg_chunk,
                       (uint32_t)S.K, c->sf_anchor.p, c->sf_part.p, S.own_first, S.own_end);
  else
    hipLaunchKernelGGL(k_pf_chunks, grid, dim3(SD_TB), 0, c->stream, field, stride_f, C, c0, ng, c->perm_b.p, S.d.pos, S.d.seg_start, S.d.seg_chunk,
                       (uint32_t)S.K, c->sf_anchor.p, c->sf_part.p);
}

template <> vgs_status attr_launch_hist<PsSort>(vgs_ctx* c, const AttrSource<PsSort>& S, const int32_t* cls, uint32_t n_classes, unsigned long long* hist,
                                   unsigned long long* n_outside) {
  const dim3 grid((unsigned)S.n_chunks_max);
  if (S.own)
    hipLaunchKernelGGL(k_pf_own_hist, grid, dim3(SD_TB), 0, c->stream, cls, n_classes, c->perm_b.p, S.d.pos, S.d.seg_start, S.d.seg_chunk, (uint32_t)S.K, hist,
                       n_outside, S.own_first, S.own_end);
  else
    hipLaunchKernelGGL(k_pf_hist, grid, dim3(SD_TB), 0, c->stream, cls, n_classes, c->perm_b.p, S.d.pos, S.d.seg_start, S.d.seg_chunk, (uint32_t)S.K, hist,
                       n_outside);
  return VGS_OK;
}

// the labels with an own point in the octree leave a record: a run of seg_start (K + 1 words) that is not empty
template <> size_t attr_rule_words<PsSort>(vgs_ctx*, const AttrSource<PsSort>& S, const uint32_t** dev) { *dev = S.d.seg_start; return (size_t)S.K + 1; }
template <> bool attr_has_record<PsSort>(const AttrSource<PsSort>&, const uint32_t* seg_start, size_t k) { return seg_start[k + 1] > seg_start[k]; }

// The rules both tables share, in this family's order: the state, the labelling (the rules of vgs_point_label_descriptors; own: of
// vgs_own_point_label_moments) and the attribute array.  own: the calls of a tile context, n the rank's own points.
static vgs_status pf_check(vgs_ctx* c, const char* fn, bool own, const int32_t* labels, int64_t K, const void* in, int64_t n) {
  vgs_status s = attr_check_segmented(c, fn);
  if (s != VGS_OK) return s;
  if (own) {
    if ((s = attr_check_tile_only(c, fn)) != VGS_OK || (s = attr_check_K(c, fn, K, (int64_t)0x7fffffff)) != VGS_OK) return s;
    s = attr_check_n(c, fn, "n_own", n, "own points of the context", c->n_own);
  } else {
    if (vgs_is_tile(c))
      return attr_fail(c, fn, VGS_E_STATE, "a tile context (owned region / own point range) holds only part of the cloud, and the attribute tables of a point labelling over all ranks are vgs_tiles_point_label_field_stats and vgs_tiles_point_label_class_histogram of the tiled driver");
    s = attr_check_n(c, fn, "n", n, "points of the cloud", c->N);
  }
  if (s != VGS_OK || (s = attr_check_array(c, fn, "labels", labels, n)) != VGS_OK || (s = attr_check_array(c, fn, "the input array", in, n)) != VGS_OK) return s;
  if (!own) return attr_check_K(c, fn, K, (int64_t)0x7fffffff);
  if (c->own_first < 0 || c->own_first + n > c->N)
    return attr_fail(c, fn, VGS_E_ARG, "the own point range ends at " + std::to_string(c->own_first + n) + ", the cloud holds " + std::to_string(c->N) + " points");
  return VGS_OK;
}

// The eight entry points of a table come through one function.  R = NULL: one context, dense rows.  R given: a tile context, compact
// records.  labels and the attribute array are both in HBM (on_device) or both the host's, uploaded here.
static vgs_status pf_field_run(vgs_ctx* c, const char* fn, bool on_device, const int32_t* labels, int64_t K, const float* field, int64_t n,
                               int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, const AttrRecords* R, const AttrFieldOut& O) {
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  vgs_status s = VGS_OK;
  if (!on_device && ((s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK || (s = attr_upload_field(c, &field, n, n_channels, stride_bytes)) != VGS_OK))
    return s;
  AttrSource<PsSort> S;
  if ((s = pf_source(c, fn, labels, K, R != nullptr, n_skipped, S)) != VGS_OK) return s;
  return attr_field_table(c, S, field, n_channels, stride_bytes, R, O);
}

static vgs_status pf_field_entry(vgs_ctx* c, const char* fn, bool on_device, const int32_t* labels, int64_t K, const float* field, int64_t n,
                                 int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, const AttrRecords* R, const AttrFieldOut& O) {
  if (!c) return VGS_E_ARG;
  if (R && R->n_records) *R->n_records = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = pf_check(c, fn, R != nullptr, labels, K, field, n);
  if (s != VGS_OK || (s = attr_check_channels(c, fn, n_channels)) != VGS_OK || (s = attr_check_stride(c, fn, n_channels, stride_bytes)) != VGS_OK ||
      (s = attr_check_limit(c, fn, K, "labels", n_channels, "channels", "entries")) != VGS_OK)
    return s;
  return attr_settle(c, pf_field_run(c, fn, on_device, labels, K, field, n, n_channels, stride_bytes, n_skipped, R, O));
}

static vgs_status pf_hist_run(vgs_ctx* c, const char* fn, bool on_device, const int32_t* labels, int64_t K, const int32_t* cls, int64_t n,
                              int32_t n_classes, int64_t* n_skipped, const AttrRecords* R, const AttrHistOut& O) {
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  vgs_status s = VGS_OK;
  if (!on_device && ((s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK || (s = attr_upload_classes(c, &cls, n)) != VGS_OK)) return s;
  AttrSource<PsSort> S;
  if ((s = pf_source(c, fn, labels, K, R != nullptr, n_skipped, S)) != VGS_OK) return s;
  return attr_hist_table(c, S, cls, n_classes, R, O);
}

static vgs_status pf_hist_entry(vgs_ctx* c, const char* fn, bool on_device, const int32_t* labels, int64_t K, const int32_t* cls, int64_t n,
                                int32_t n_classes, int64_t* n_skipped, const AttrRecords* R, const AttrHistOut& O) {
  if (!c) return VGS_E_ARG;
  if (R && R->n_records) *R->n_records = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = pf_check(c, fn, R != nullptr, labels, K, cls, n);
  if (s != VGS_OK || (s = attr_check_classes(c, fn, n_classes)) != VGS_OK ||
      (s = attr_check_limit(c, fn, K, "labels", n_classes, "classes", "counters")) != VGS_OK)
    return s;
  return attr_settle(c, pf_hist_run(c, fn, on_device, labels, K, cls, n, n_classes, n_skipped, R, O));
}

extern "C" vgs_status vgs_point_label_field_stats(vgs_ctx* c, const int32_t* labels_host, int64_t K, const float* field_host, int64_t n,
                                                  int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor,
                                                  double* mean, double* var, float* vmin, float* vmax) {
  return pf_field_entry(c, "vgs_point_label_field_stats", false, labels_host, K, field_host, n, n_channels, stride_bytes, n_skipped, nullptr,
                        {n_valid, anchor, mean, var, vmin, vmax});
}

extern "C" vgs_status vgs_point_label_field_stats_device(vgs_ctx* c, const int32_t* labels_dev, int64_t K, const float* field_dev, int64_t n,
                                                         int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid,
                                                         double* anchor, double* mean, double* var, float* vmin, float* vmax) {
  return pf_field_entry(c, "vgs_point_label_field_stats_device", true, labels_dev, K, field_dev, n, n_channels, stride_bytes, n_skipped, nullptr,
                        {n_valid, anchor, mean, var, vmin, vmax});
}

extern "C" vgs_status vgs_point_label_class_histogram(vgs_ctx* c, const int32_t* labels_host, int64_t K, const int32_t* cls_host, int64_t n,
                                                      int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority,
                                                      int64_t* majority_count) {
  return pf_hist_entry(c, "vgs_point_label_class_histogram", false, labels_host, K, cls_host, n, n_classes, n_skipped, nullptr,
                       {hist, n_outside, majority, majority_count});
}

extern "C" vgs_status vgs_point_label_class_histogram_device(vgs_ctx* c, const int32_t* labels_dev, int64_t K, const int32_t* cls_dev, int64_t n,
                                                             int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside,
                                                             int32_t* majority, int64_t* majority_count) {
  return pf_hist_entry(c, "vgs_point_label_class_histogram_device", true, labels_dev, K, cls_dev, n, n_classes, n_skipped, nullptr,
                       {hist, n_outside, majority, majority_count});
}

// ------------------------------------------------------------------------------------------------ tile contexts (include/vgs_tiles.h)
// This rank's raw moments and class counts of the caller's labels 0 .. K-1 over its own octree points, n_own labels and rows: dense on
// the device, compact on the host.
extern "C" vgs_status vgs_own_point_label_field_moments(vgs_ctx* c, int64_t K, const int32_t* labels_host, const float* field_host, int64_t n_own,
                                                        int32_t n_channels, int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped,
                                                        int32_t* label, int64_t* n_valid, double* anchor, double* s1, double* s2, float* vmin,
                                                        float* vmax) {
  const AttrRecords R = {n_records, label};
  return pf_field_entry(c, "vgs_own_point_label_field_moments", false, labels_host, K, field_host, n_own, n_channels, stride_bytes, n_skipped, &R,
                        {n_valid, anchor, s1, s2, vmin, vmax});
}

extern "C" vgs_status vgs_own_point_label_field_moments_device(vgs_ctx* c, int64_t K, const int32_t* labels_dev, const float* field_dev, int64_t n_own,
                                                               int32_t n_channels, int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped,
                                                               int32_t* label, int64_t* n_valid, double* anchor, double* s1, double* s2,
                                                               float* vmin, float* vmax) {
  const AttrRecords R = {n_records, label};
  return pf_field_entry(c, "vgs_own_point_label_field_moments_device", true, labels_dev, K, field_dev, n_own, n_channels, stride_bytes, n_skipped, &R,
                        {n_valid, anchor, s1, s2, vmin, vmax});
}

extern "C" vgs_status vgs_own_point_label_class_counts(vgs_ctx* c, int64_t K, const int32_t* labels_host, const int32_t* cls_host, int64_t n_own,
                                                       int32_t n_classes, int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* hist,
                                                       int64_t* n_outside) {
  const AttrRecords R = {n_records, label};
  return pf_hist_entry(c, "vgs_own_point_label_class_counts", false, labels_host, K, cls_host, n_own, n_classes, n_skipped, &R,
                       {hist, n_outside, nullptr, nullptr});
}

extern "C" vgs_status vgs_own_point_label_class_counts_device(vgs_ctx* c, int64_t K, const int32_t* labels_dev, const int32_t* cls_dev, int64_t n_own,
                                                              int32_t n_classes, int64_t* n_records, int64_t* n_skipped, int32_t* label,
                                                              int64_t* hist, int64_t* n_outside) {
  const AttrRecords R = {n_records, label};
  return pf_hist_entry(c, "vgs_own_point_label_class_counts_device", true, labels_dev, K, cls_dev, n_own, n_classes, n_skipped, &R,
                       {hist, n_outside, nullptr, nullptr});
}
