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
#include <string.h>

#include <algorithm>
#include <string>

#include "segpass.hpp"

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
// the checks both tables share: the state, the labelling (the rules of vgs_point_label_descriptors) and the attribute array
static vgs_status pf_check(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t K, const void* in, int64_t n) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of the cloud, and the attribute tables of a point labelling over all ranks are vgs_tiles_point_label_field_stats and vgs_tiles_point_label_class_histogram of the tiled driver";
    return VGS_E_STATE;
  }
  if (n != c->N) {
    c->err = std::string(fn) + ": n = " + std::to_string(n) + " must equal the number of points of the cloud, " + std::to_string(c->N);
    return VGS_E_ARG;
  }
  if (!labels && n > 0) { c->err = std::string(fn) + ": labels is NULL"; return VGS_E_ARG; }
  if (!in && n > 0) { c->err = std::string(fn) + ": the input array is NULL"; return VGS_E_ARG; }
  if (K < 0 || K > (int64_t)0x7fffffff) { c->err = std::string(fn) + ": K = " + std::to_string(K) + " is out of range"; return VGS_E_ARG; }
  return VGS_OK;
}

static vgs_status pf_check_field(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t K, const float* field, int64_t n, int32_t n_channels,
                                 int64_t stride_bytes) {
  vgs_status s = pf_check(c, fn, labels, K, field, n);
  if (s != VGS_OK) return s;
  if (n_channels < 1 || n_channels > 64) {
    c->err = std::string(fn) + ": n_channels = " + std::to_string(n_channels) + " must be in 1 .. 64";
    return VGS_E_ARG;
  }
  if (stride_bytes < 4 * (int64_t)n_channels || stride_bytes % 4 != 0) {
    c->err = std::string(fn) + ": stride_bytes = " + std::to_string(stride_bytes) + " must be a multiple of 4 and at least 4 * n_channels = " +
             std::to_string(4 * (int64_t)n_channels);
    return VGS_E_ARG;
  }
  if (K * (int64_t)n_channels > ((int64_t)1 << 27)) {
    c->err = std::string(fn) + ": " + std::to_string(K) + " labels x " + std::to_string(n_channels) + " channels = " +
             std::to_string(K * (int64_t)n_channels) + " entries exceed the table's limit of 2^27 = " + std::to_string((int64_t)1 << 27);
    return VGS_E_UNSUPPORTED;
  }
  return VGS_OK;
}

static vgs_status pf_check_hist(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t K, const int32_t* cls, int64_t n, int32_t n_classes) {
  vgs_status s = pf_check(c, fn, labels, K, cls, n);
  if (s != VGS_OK) return s;
  if (n_classes < 1 || n_classes > 1024) {
    c->err = std::string(fn) + ": n_classes = " + std::to_string(n_classes) + " must be in 1 .. 1024";
    return VGS_E_ARG;
  }
  if (K * (int64_t)n_classes > ((int64_t)1 << 27)) {
    c->err = std::string(fn) + ": " + std::to_string(K) + " labels x " + std::to_string(n_classes) + " classes = " +
             std::to_string(K * (int64_t)n_classes) + " counters exceed the table's limit of 2^27 = " + std::to_string((int64_t)1 << 27);
    return VGS_E_UNSUPPORTED;
  }
  return VGS_OK;
}

#define PF_COPY(dst, src, count) \
  if (dst) VGS_HIP_TRY(c, hipMemcpyAsync((dst), (src), (count) * sizeof(*(dst)), hipMemcpyDeviceToHost, c->stream))

// the field table of labels_dev over field_dev, both in HBM: every output a host array of K x n_channels, any may be NULL
static vgs_status pf_field_stats(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, const float* field_dev, int32_t n_channels,
                                 int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin,
                                 float* vmax) {
  PsSort S;
  vgs_status s = ps_sort_points(c, fn, labels_dev, 0, c->N, K, 0, n_skipped, S);
  if (s != VGS_OK) return s;
  if (!S.sorted) return VGS_OK;   // K = 0: validated, the skipped points counted, nothing to write
  const uint32_t C = (uint32_t)n_channels;
  const size_t kc = (size_t)K * C;
  const int64_t stride_f = stride_bytes / 4;
  VGS_HIP_TRY(c, c->sf_part.ensure((size_t)S.n_chunks_max * SF_G * SF_REC));
  VGS_HIP_TRY(c, c->sf_anchor.ensure(kc)); VGS_HIP_TRY(c, c->sf_mean.ensure(kc)); VGS_HIP_TRY(c, c->sf_var.ensure(kc));
  VGS_HIP_TRY(c, c->sf_nvalid.ensure(kc)); VGS_HIP_TRY(c, c->sf_min.ensure(kc)); VGS_HIP_TRY(c, c->sf_max.ensure(kc));
  hipLaunchKernelGGL(k_pf_anchor, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, c->stream, field_dev, stride_f, C, c->perm_b.p, S.pos, S.seg_start,
                     (uint32_t)K, (int64_t)0, c->sf_anchor.p);
  for (uint32_t c0 = 0; c0 < C; c0 += SF_G) {
    const uint32_t ng = C - c0 < SF_G ? C - c0 : SF_G;
    if (c->Nf > 0)
      hipLaunchKernelGGL(k_pf_chunks, dim3((unsigned)S.n_chunks_max), dim3(SD_TB), 0, c->stream, field_dev, stride_f, C, c0, ng, c->perm_b.p, S.pos,
                         S.seg_start, S.seg_chunk, (uint32_t)K, c->sf_anchor.p, c->sf_part.p);
    sf_launch_final(c, S.seg_chunk, c->sf_part.p, (uint32_t)S.n_chunks_max, K, C, c0, ng, c->sf_anchor.p, c->sf_nvalid.p, c->sf_mean.p, c->sf_var.p,
                    c->sf_min.p, c->sf_max.p);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  PF_COPY(n_valid, c->sf_nvalid.p, kc); PF_COPY(anchor, c->sf_anchor.p, kc); PF_COPY(mean, c->sf_mean.p, kc); PF_COPY(var, c->sf_var.p, kc);
  PF_COPY(vmin, c->sf_min.p, kc); PF_COPY(vmax, c->sf_max.p, kc);
  return VGS_OK;
}

static vgs_status pf_field_entry(vgs_ctx* c, const char* fn, bool on_device, const int32_t* labels, int64_t K, const float* field, int64_t n,
                                 int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor, double* mean,
                                 double* var, float* vmin, float* vmax) {
  if (!c) return VGS_E_ARG;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = pf_check_field(c, fn, labels, K, field, n, n_channels, stride_bytes);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device) {
    if ((s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK) return s;
    if (n > 0) {
      // one upload, rows at the caller's stride; the last row ends with its last channel
      const size_t bytes = (size_t)(n - 1) * (size_t)stride_bytes + 4 * (size_t)n_channels;
      VGS_HIP_TRY(c, c->sf_in.ensure((bytes + 3) / 4));
      VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_in.p, field, bytes, hipMemcpyHostToDevice, c->stream));
      VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
      field = c->sf_in.p;
    }
  }
  s = pf_field_stats(c, fn, labels, K, field, n_channels, stride_bytes, n_skipped, n_valid, anchor, mean, var, vmin, vmax);
  // the rows have arrived, and arrays read in place are the caller's again -- after a failure as well
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (s == VGS_OK) VGS_HIP_TRY(c, e);
  return s;
}

// the histogram of labels_dev over cls_dev, both in HBM: hist K x n_classes, the others K; host arrays, any may be NULL
static vgs_status pf_class_hist(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, const int32_t* cls_dev, int32_t n_classes,
                                int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority, int64_t* majority_count) {
  PsSort S;
  vgs_status s = ps_sort_points(c, fn, labels_dev, 0, c->N, K, 0, n_skipped, S);
  if (s != VGS_OK) return s;
  if (!S.sorted) return VGS_OK;
  const size_t k = (size_t)K, kc = k * (size_t)n_classes;
  VGS_HIP_TRY(c, c->sf_hist.ensure(kc + 2 * k)); VGS_HIP_TRY(c, c->sf_maj.ensure(k));
  int64_t *d_hist = c->sf_hist.p, *d_out = d_hist + kc, *d_majc = d_out + k;
  VGS_HIP_TRY(c, hipMemsetAsync(d_hist, 0, (kc + k) * sizeof(int64_t), c->stream));
  if (c->Nf > 0)
    hipLaunchKernelGGL(k_pf_hist, dim3((unsigned)S.n_chunks_max), dim3(SD_TB), 0, c->stream, cls_dev, (uint32_t)n_classes, c->perm_b.p, S.pos, S.seg_start,
                       S.seg_chunk, (uint32_t)K, (unsigned long long*)d_hist, (unsigned long long*)d_out);
  sf_launch_majority(c, d_hist, n_classes, K, c->sf_maj.p, d_majc);
  VGS_HIP_TRY(c, hipGetLastError());
  PF_COPY(hist, d_hist, kc); PF_COPY(n_outside, d_out, k); PF_COPY(majority, c->sf_maj.p, k); PF_COPY(majority_count, d_majc, k);
  return VGS_OK;
}

static vgs_status pf_hist_entry(vgs_ctx* c, const char* fn, bool on_device, const int32_t* labels, int64_t K, const int32_t* cls, int64_t n,
                                int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority,
                                int64_t* majority_count) {
  if (!c) return VGS_E_ARG;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = pf_check_hist(c, fn, labels, K, cls, n, n_classes);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device) {
    if ((s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK) return s;
    if (n > 0) {
      VGS_HIP_TRY(c, c->sf_cls.ensure((size_t)n));
      VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_cls.p, cls, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
      VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
      cls = c->sf_cls.p;
    }
  }
  s = pf_class_hist(c, fn, labels, K, cls, n_classes, n_skipped, hist, n_outside, majority, majority_count);
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (s == VGS_OK) VGS_HIP_TRY(c, e);
  return s;
}

extern "C" vgs_status vgs_point_label_field_stats(vgs_ctx* c, const int32_t* labels_host, int64_t K, const float* field_host, int64_t n,
                                                  int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor,
                                                  double* mean, double* var, float* vmin, float* vmax) {
  return pf_field_entry(c, "vgs_point_label_field_stats", false, labels_host, K, field_host, n, n_channels, stride_bytes, n_skipped, n_valid, anchor, mean,
                        var, vmin, vmax);
}

extern "C" vgs_status vgs_point_label_field_stats_device(vgs_ctx* c, const int32_t* labels_dev, int64_t K, const float* field_dev, int64_t n,
                                                         int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid,
                                                         double* anchor, double* mean, double* var, float* vmin, float* vmax) {
  return pf_field_entry(c, "vgs_point_label_field_stats_device", true, labels_dev, K, field_dev, n, n_channels, stride_bytes, n_skipped, n_valid, anchor,
                        mean, var, vmin, vmax);
}

extern "C" vgs_status vgs_point_label_class_histogram(vgs_ctx* c, const int32_t* labels_host, int64_t K, const int32_t* cls_host, int64_t n,
                                                      int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority,
                                                      int64_t* majority_count) {
  return pf_hist_entry(c, "vgs_point_label_class_histogram", false, labels_host, K, cls_host, n, n_classes, n_skipped, hist, n_outside, majority,
                       majority_count);
}

extern "C" vgs_status vgs_point_label_class_histogram_device(vgs_ctx* c, const int32_t* labels_dev, int64_t K, const int32_t* cls_dev, int64_t n,
                                                             int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside,
                                                             int32_t* majority, int64_t* majority_count) {
  return pf_hist_entry(c, "vgs_point_label_class_histogram_device", true, labels_dev, K, cls_dev, n, n_classes, n_skipped, hist, n_outside, majority,
                       majority_count);
}

// ------------------------------------------------------------------------------------------------ tile contexts (include/vgs_tiles.h)
// the checks both record calls share: the state, the labelling (the rules of vgs_own_point_label_moments) and the attribute array
static vgs_status pfo_check(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t K, const void* in, int64_t n_own) {
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
  if (!in && n_own > 0) { c->err = std::string(fn) + ": the input array is NULL"; return VGS_E_ARG; }
  if (c->own_first < 0 || c->own_first + n_own > c->N) {
    c->err = std::string(fn) + ": the own point range ends at " + std::to_string(c->own_first + n_own) + ", the cloud holds " + std::to_string(c->N) + " points";
    return VGS_E_ARG;
  }
  return VGS_OK;
}

// the labels with an own point in the octree, ascending: a run that is not empty (seg_start, K + 1 words in HBM)
static vgs_status pfo_own_labels(vgs_ctx* c, const uint32_t* seg_start, int64_t K, std::vector<int64_t>& rows) {
  std::vector<uint32_t> st((size_t)K + 1);
  VGS_HIP_TRY(c, hipMemcpyAsync(st.data(), seg_start, st.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  rows.clear();
  for (int64_t k = 0; k < K; ++k) if (st[(size_t)k + 1] > st[(size_t)k]) rows.push_back(k);
  return VGS_OK;
}

// rows of a dense device table (K rows of `per` entries) into a compact host array, which may be NULL
template <typename T>
static vgs_status pfo_compact(vgs_ctx* c, const T* dev, int64_t K, size_t per, const std::vector<int64_t>& rows, T* out) {
  if (!out || rows.empty()) return VGS_OK;
  std::vector<T> h((size_t)K * per);
  VGS_HIP_TRY(c, hipMemcpyAsync(h.data(), dev, h.size() * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < rows.size(); ++i) std::copy(h.begin() + (size_t)rows[i] * per, h.begin() + ((size_t)rows[i] + 1) * per, out + i * per);
  return VGS_OK;
}

// This rank's raw moments of the caller's labels 0 .. K-1 over its own octree points, labels_dev and field_dev in HBM (n_own rows each):
// the sort of the own points, their anchors, the own-row chunks per channel group, the fold without the finish.  Dense on the device
// (K x n_channels), compact on the host.
static vgs_status pfo_field_moments(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, const float* field_dev, int32_t n_channels,
                                    int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* n_valid, double* anchor,
                                    double* s1, double* s2, float* vmin, float* vmax) {
  PsSort S;
  vgs_status s = ps_sort_points(c, fn, labels_dev, c->own_first, c->n_own, K, 0, n_skipped, S);
  if (s != VGS_OK) return s;
  if (!S.sorted || c->Nf == 0) return VGS_OK;   // K = 0 or no point in the octree: validated, the skipped points counted, no record
  const uint32_t C = (uint32_t)n_channels;
  const size_t kc = (size_t)K * C;
  const int64_t stride_f = stride_bytes / 4, own_end = c->own_first + c->n_own;
  VGS_HIP_TRY(c, c->sf_part.ensure((size_t)S.n_chunks_max * SF_G * SF_REC));
  VGS_HIP_TRY(c, c->sf_anchor.ensure(kc)); VGS_HIP_TRY(c, c->sf_mean.ensure(kc)); VGS_HIP_TRY(c, c->sf_var.ensure(kc));
  VGS_HIP_TRY(c, c->sf_nvalid.ensure(kc)); VGS_HIP_TRY(c, c->sf_min.ensure(kc)); VGS_HIP_TRY(c, c->sf_max.ensure(kc));
  hipLaunchKernelGGL(k_pf_anchor, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, c->stream, field_dev, stride_f, C, c->perm_b.p, S.pos, S.seg_start,
                     (uint32_t)K, c->own_first, c->sf_anchor.p);
  for (uint32_t c0 = 0; c0 < C; c0 += SF_G) {
    const uint32_t ng = C - c0 < SF_G ? C - c0 : SF_G;
    hipLaunchKernelGGL(k_pf_own_chunks, dim3((unsigned)S.n_chunks_max), dim3(SD_TB), 0, c->stream, field_dev, stride_f, C, c0, ng, c->perm_b.p, S.pos,
                       S.seg_start, S.seg_chunk, (uint32_t)K, c->sf_anchor.p, c->sf_part.p, c->own_first, own_end);
    sf_launch_own_records(c, S.seg_chunk, c->sf_part.p, (uint32_t)S.n_chunks_max, K, C, c0, ng, c->sf_nvalid.p, c->sf_mean.p, c->sf_var.p, c->sf_min.p,
                          c->sf_max.p);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  std::vector<int64_t> rows;
  if ((s = pfo_own_labels(c, S.seg_start, K, rows)) != VGS_OK) return s;
  if (label) for (size_t i = 0; i < rows.size(); ++i) label[i] = (int32_t)rows[i];
  if ((s = pfo_compact(c, c->sf_nvalid.p, K, C, rows, n_valid)) != VGS_OK) return s;
  if ((s = pfo_compact(c, c->sf_anchor.p, K, C, rows, anchor)) != VGS_OK) return s;
  if ((s = pfo_compact(c, c->sf_mean.p, K, C, rows, s1)) != VGS_OK) return s;
  if ((s = pfo_compact(c, c->sf_var.p, K, C, rows, s2)) != VGS_OK) return s;
  if ((s = pfo_compact(c, c->sf_min.p, K, C, rows, vmin)) != VGS_OK) return s;
  if ((s = pfo_compact(c, c->sf_max.p, K, C, rows, vmax)) != VGS_OK) return s;
  if (n_records) *n_records = (int64_t)rows.size();
  return VGS_OK;
}

static vgs_status pfo_field_entry(vgs_ctx* c, const char* fn, bool on_device, int64_t K, const int32_t* labels, const float* field, int64_t n_own,
                                  int32_t n_channels, int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* n_valid,
                                  double* anchor, double* s1, double* s2, float* vmin, float* vmax) {
  if (!c) return VGS_E_ARG;
  if (n_records) *n_records = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = pfo_check(c, fn, labels, K, field, n_own);
  if (s != VGS_OK) return s;
  if (n_channels < 1 || n_channels > 64) {
    c->err = std::string(fn) + ": n_channels = " + std::to_string(n_channels) + " must be in 1 .. 64";
    return VGS_E_ARG;
  }
  if (stride_bytes < 4 * (int64_t)n_channels || stride_bytes % 4 != 0) {
    c->err = std::string(fn) + ": stride_bytes = " + std::to_string(stride_bytes) + " must be a multiple of 4 and at least 4 * n_channels = " +
             std::to_string(4 * (int64_t)n_channels);
    return VGS_E_ARG;
  }
  if (K * (int64_t)n_channels > ((int64_t)1 << 27)) {
    c->err = std::string(fn) + ": " + std::to_string(K) + " labels x " + std::to_string(n_channels) + " channels = " +
             std::to_string(K * (int64_t)n_channels) + " entries exceed the table's limit of 2^27 = " + std::to_string((int64_t)1 << 27);
    return VGS_E_UNSUPPORTED;
  }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device) {
    if ((s = vgs_upload_point_labels(c, labels, n_own, &labels)) != VGS_OK) return s;
    if (n_own > 0) {
      // one upload, rows at the caller's stride; the last row ends with its last channel
      const size_t bytes = (size_t)(n_own - 1) * (size_t)stride_bytes + 4 * (size_t)n_channels;
      VGS_HIP_TRY(c, c->sf_in.ensure((bytes + 3) / 4));
      VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_in.p, field, bytes, hipMemcpyHostToDevice, c->stream));
      VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
      field = c->sf_in.p;
    }
  }
  s = pfo_field_moments(c, fn, labels, K, field, n_channels, stride_bytes, n_records, n_skipped, label, n_valid, anchor, s1, s2, vmin, vmax);
  // arrays read in place are the caller's again -- after a failure as well
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (s == VGS_OK) VGS_HIP_TRY(c, e);
  return s;
}

// this rank's class counts of the caller's labels over its own octree points: dense on the device, compact on the host
static vgs_status pfo_class_counts(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, const int32_t* cls_dev, int32_t n_classes,
                                   int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* hist, int64_t* n_outside) {
  PsSort S;
  vgs_status s = ps_sort_points(c, fn, labels_dev, c->own_first, c->n_own, K, 0, n_skipped, S);
  if (s != VGS_OK) return s;
  if (!S.sorted || c->Nf == 0) return VGS_OK;
  const size_t k = (size_t)K, nc = (size_t)n_classes, kc = k * nc;
  VGS_HIP_TRY(c, c->sf_hist.ensure(kc + 2 * k));
  int64_t *d_hist = c->sf_hist.p, *d_out = d_hist + kc;
  VGS_HIP_TRY(c, hipMemsetAsync(d_hist, 0, (kc + k) * sizeof(int64_t), c->stream));
  hipLaunchKernelGGL(k_pf_own_hist, dim3((unsigned)S.n_chunks_max), dim3(SD_TB), 0, c->stream, cls_dev, (uint32_t)n_classes, c->perm_b.p, S.pos, S.seg_start,
                     S.seg_chunk, (uint32_t)K, (unsigned long long*)d_hist, (unsigned long long*)d_out, c->own_first, c->own_first + c->n_own);
  VGS_HIP_TRY(c, hipGetLastError());
  std::vector<int64_t> rows;
  if ((s = pfo_own_labels(c, S.seg_start, K, rows)) != VGS_OK) return s;
  if (label) for (size_t i = 0; i < rows.size(); ++i) label[i] = (int32_t)rows[i];
  if ((s = pfo_compact(c, (const int64_t*)d_hist, K, nc, rows, hist)) != VGS_OK) return s;
  if ((s = pfo_compact(c, (const int64_t*)d_out, K, 1, rows, n_outside)) != VGS_OK) return s;
  if (n_records) *n_records = (int64_t)rows.size();
  return VGS_OK;
}

static vgs_status pfo_hist_entry(vgs_ctx* c, const char* fn, bool on_device, int64_t K, const int32_t* labels, const int32_t* cls, int64_t n_own,
                                 int32_t n_classes, int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* hist, int64_t* n_outside) {
  if (!c) return VGS_E_ARG;
  if (n_records) *n_records = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = pfo_check(c, fn, labels, K, cls, n_own);
  if (s != VGS_OK) return s;
  if (n_classes < 1 || n_classes > 1024) {
    c->err = std::string(fn) + ": n_classes = " + std::to_string(n_classes) + " must be in 1 .. 1024";
    return VGS_E_ARG;
  }
  if (K * (int64_t)n_classes > ((int64_t)1 << 27)) {
    c->err = std::string(fn) + ": " + std::to_string(K) + " labels x " + std::to_string(n_classes) + " classes = " +
             std::to_string(K * (int64_t)n_classes) + " counters exceed the table's limit of 2^27 = " + std::to_string((int64_t)1 << 27);
    return VGS_E_UNSUPPORTED;
  }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device) {
    if ((s = vgs_upload_point_labels(c, labels, n_own, &labels)) != VGS_OK) return s;
    if (n_own > 0) {
      VGS_HIP_TRY(c, c->sf_cls.ensure((size_t)n_own));
      VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_cls.p, cls, (size_t)n_own * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
      VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
      cls = c->sf_cls.p;
    }
  }
  s = pfo_class_counts(c, fn, labels, K, cls, n_classes, n_records, n_skipped, label, hist, n_outside);
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (s == VGS_OK) VGS_HIP_TRY(c, e);
  return s;
}

extern "C" vgs_status vgs_own_point_label_field_moments(vgs_ctx* c, int64_t K, const int32_t* labels_host, const float* field_host, int64_t n_own,
                                                        int32_t n_channels, int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped,
                                                        int32_t* label, int64_t* n_valid, double* anchor, double* s1, double* s2, float* vmin,
                                                        float* vmax) {
  return pfo_field_entry(c, "vgs_own_point_label_field_moments", false, K, labels_host, field_host, n_own, n_channels, stride_bytes, n_records, n_skipped,
                         label, n_valid, anchor, s1, s2, vmin, vmax);
}

extern "C" vgs_status vgs_own_point_label_field_moments_device(vgs_ctx* c, int64_t K, const int32_t* labels_dev, const float* field_dev, int64_t n_own,
                                                               int32_t n_channels, int64_t stride_bytes, int64_t* n_records, int64_t* n_skipped,
                                                               int32_t* label, int64_t* n_valid, double* anchor, double* s1, double* s2,
                                                               float* vmin, float* vmax) {
  return pfo_field_entry(c, "vgs_own_point_label_field_moments_device", true, K, labels_dev, field_dev, n_own, n_channels, stride_bytes, n_records,
                         n_skipped, label, n_valid, anchor, s1, s2, vmin, vmax);
}

extern "C" vgs_status vgs_own_point_label_class_counts(vgs_ctx* c, int64_t K, const int32_t* labels_host, const int32_t* cls_host, int64_t n_own,
                                                       int32_t n_classes, int64_t* n_records, int64_t* n_skipped, int32_t* label, int64_t* hist,
                                                       int64_t* n_outside) {
  return pfo_hist_entry(c, "vgs_own_point_label_class_counts", false, K, labels_host, cls_host, n_own, n_classes, n_records, n_skipped, label, hist,
                        n_outside);
}

extern "C" vgs_status vgs_own_point_label_class_counts_device(vgs_ctx* c, int64_t K, const int32_t* labels_dev, const int32_t* cls_dev, int64_t n_own,
                                                              int32_t n_classes, int64_t* n_records, int64_t* n_skipped, int32_t* label,
                                                              int64_t* hist, int64_t* n_outside) {
  return pfo_hist_entry(c, "vgs_own_point_label_class_counts_device", true, K, labels_dev, cls_dev, n_own, n_classes, n_records, n_skipped, label, hist,
                        n_outside);
}
