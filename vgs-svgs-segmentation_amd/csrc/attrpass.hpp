// attrpass.hpp -- the host side of the attribute tables (field statistics, class histograms), one copy for the four callers: the node
// labelling of one context and of a tile context (segfield.hip), a caller's per-point labelling of one context and of a tile context
// (pointfield.hip).  The kernels stay in those files and in segpass.hpp; what the files plug in here is an AttrSource from one of their
// makers and, as specialisations for its decomposition type of the five templates declared below, the launch lines and the rule that
// gives a label a record (a missing one is an undefined symbol of that name at link time):
//   vgs_status attr_launch_anchor(c, S, field, stride_f, C)           anchor[k, ch] into sf_anchor
//   void       attr_launch_chunks(c, S, field, stride_f, C, c0, ng)   the partials of one channel group into sf_part
//   vgs_status attr_launch_hist(c, S, cls, n_classes, hist, n_outside)
//   size_t     attr_rule_words(c, S, dev)                             the words in HBM the rule reads, and how many
//   bool       attr_has_record(S, words, k)                           tile contexts: label k leaves a record
// attr_field_table and attr_hist_table are the two drivers, vgs_copy_rows (vgs_context.hpp) / attr_copy_compact the two ways rows reach the host,
// attr_upload_field / attr_upload_classes the host variants' uploads, attr_check_* the argument rules with one text each (the order in
// which a family applies them is its own).  An entry point ends with attr_settle: after a failure it still waits for the stream, so that
// arrays read in place are the caller's again.
#ifndef VGS_ATTRPASS_HPP_
#define VGS_ATTRPASS_HPP_

#include <string.h>

#include <string>
#include <vector>

#include "segpass.hpp"

// Where a pass gets its points from.  Dec: the decomposition the launch lines read (SdPrep: nodes sorted by label; PsSort: points sorted
// by label).  live = false: nothing is written at all; chunks = false: no point in the octree, the folds alone give the empty rows.
template <typename Dec>
struct AttrSource {
  int64_t K = 0;
  const uint32_t* seg_chunk = nullptr;   // K + 1 first chunks
  int64_t n_chunks_max = 0;              // grid of the chunk kernels
  bool live = false, chunks = false;
  bool own = false;                      // a tile context: only the input indices own_first .. own_end - 1 count
  int64_t own_first = 0, own_end = 0;
  Dec d;
};

// the compact records of a tile context: their number and labels
struct AttrRecords { int64_t* n_records; int32_t* label; };
// m1, m2: mean and variance of the rows (k_sf_final), S1 and S2 of a tile context's records (k_sf_own_records)
struct AttrFieldOut { int64_t* n_valid; double *anchor, *m1, *m2; float *vmin, *vmax; };
struct AttrHistOut { int64_t *hist, *n_outside; int32_t* majority; int64_t* majority_count; };

// What a file plugs in for its decomposition type Dec, as explicit specialisations defined before its entry points: the anchor kernel
// (anchor[k, ch] into sf_anchor), the chunk kernel of one channel group (partials into sf_part), the histogram's chunk kernel, the words
// in HBM that the record rule of a tile context reads (their number is returned) and the rule itself over a host copy of them.
template <typename Dec> vgs_status attr_launch_anchor(vgs_ctx* c, const AttrSource<Dec>& S, const float* field, int64_t stride_f, uint32_t C);
template <typename Dec> void attr_launch_chunks(vgs_ctx* c, const AttrSource<Dec>& S, const float* field, int64_t stride_f, uint32_t C, uint32_t c0, uint32_t ng);
template <typename Dec> vgs_status attr_launch_hist(vgs_ctx* c, const AttrSource<Dec>& S, const int32_t* cls, uint32_t n_classes, unsigned long long* hist,
                                                    unsigned long long* n_outside);
template <typename Dec> size_t attr_rule_words(vgs_ctx* c, const AttrSource<Dec>& S, const uint32_t** dev);
template <typename Dec> bool attr_has_record(const AttrSource<Dec>& S, const uint32_t* words, size_t k);

// ------------------------------------------------------------------------------------------------------------------------- checks
static inline vgs_status attr_fail(vgs_ctx* c, const char* fn, vgs_status s, const std::string& what) {
  c->err = std::string(fn) + ": " + what;
  return s;
}
static inline vgs_status attr_check_segmented(vgs_ctx* c, const char* fn) {
  return c->stage < ST_SEGMENTED ? attr_fail(c, fn, VGS_E_STATE, "segment first") : VGS_OK;
}
static inline vgs_status attr_check_tile_only(vgs_ctx* c, const char* fn) {
  if (c->have_region && c->n_own >= 0) return VGS_OK;
  return attr_fail(c, fn, VGS_E_STATE, "a tile context (vgs_set_owned_region and vgs_set_own_point_range) only");
}
static inline vgs_status attr_check_K(vgs_ctx* c, const char* fn, int64_t K, int64_t k_max) {
  return K < 0 || K > k_max ? attr_fail(c, fn, VGS_E_ARG, "K = " + std::to_string(K) + " is out of range") : VGS_OK;
}
// name: "n" / "n_own"; of: what the context counts ("points of the cloud" / "own points of the context")
static inline vgs_status attr_check_n(vgs_ctx* c, const char* fn, const char* name, int64_t n, const char* of, int64_t want) {
  if (n == want) return VGS_OK;
  return attr_fail(c, fn, VGS_E_ARG, std::string(name) + " = " + std::to_string(n) + " must equal the number of " + of + ", " + std::to_string(want));
}
static inline vgs_status attr_check_array(vgs_ctx* c, const char* fn, const char* what, const void* p, int64_t n) {
  return !p && n > 0 ? attr_fail(c, fn, VGS_E_ARG, std::string(what) + " is NULL") : VGS_OK;
}
static inline vgs_status attr_check_channels(vgs_ctx* c, const char* fn, int32_t n_channels) {
  if (n_channels >= 1 && n_channels <= 64) return VGS_OK;
  return attr_fail(c, fn, VGS_E_ARG, "n_channels = " + std::to_string(n_channels) + " must be in 1 .. 64");
}
static inline vgs_status attr_check_stride(vgs_ctx* c, const char* fn, int32_t n_channels, int64_t stride_bytes) {
  if (stride_bytes >= 4 * (int64_t)n_channels && stride_bytes % 4 == 0) return VGS_OK;
  return attr_fail(c, fn, VGS_E_ARG, "stride_bytes = " + std::to_string(stride_bytes) + " must be a multiple of 4 and at least 4 * n_channels = " +
                                         std::to_string(4 * (int64_t)n_channels));
}
static inline vgs_status attr_check_classes(vgs_ctx* c, const char* fn, int32_t n_classes) {
  if (n_classes >= 1 && n_classes <= 1024) return VGS_OK;
  return attr_fail(c, fn, VGS_E_ARG, "n_classes = " + std::to_string(n_classes) + " must be in 1 .. 1024");
}
// K rows of `per` columns each: "segments" / "labels" x "channels" / "classes" = "entries" / "counters"
static inline vgs_status attr_check_limit(vgs_ctx* c, const char* fn, int64_t K, const char* rows, int32_t per, const char* cols, const char* cells) {
  const int64_t lim = (int64_t)1 << 27;
  if (K * (int64_t)per <= lim) return VGS_OK;
  return attr_fail(c, fn, VGS_E_UNSUPPORTED, std::to_string(K) + " " + rows + " x " + std::to_string(per) + " " + cols + " = " + std::to_string(K * (int64_t)per) +
                                                 " " + cells + " exceed the table's limit of 2^27 = " + std::to_string(lim));
}

// after a failure too the entry points wait for the stream (once the device has been touched): arrays read in place are the caller's again
static inline vgs_status attr_settle(vgs_ctx* c, vgs_status s) {
  if (s != VGS_OK) (void)hipStreamSynchronize(c->stream);
  return s;
}

// ------------------------------------------------------------------------------------------------------------------------ uploads
// The host variants' one upload of n rows at the caller's stride into sf_in (the last row ends with its last channel) and of n classes
// into sf_cls; the pointer then names the copy.  n = 0: nothing to upload.
static inline vgs_status attr_upload_field(vgs_ctx* c, const float** field, int64_t n, int32_t n_channels, int64_t stride_bytes) {
  if (n <= 0) return VGS_OK;
  const size_t bytes = (size_t)(n - 1) * (size_t)stride_bytes + 4 * (size_t)n_channels;
  VGS_HIP_TRY(c, c->sf_in.ensure((bytes + 3) / 4));
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_in.p, *field, bytes, hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
  *field = c->sf_in.p;
  return VGS_OK;
}
static inline vgs_status attr_upload_classes(vgs_ctx* c, const int32_t** cls, int64_t n) {
  if (n <= 0) return VGS_OK;
  VGS_HIP_TRY(c, c->sf_cls.ensure((size_t)n));
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sf_cls.p, *cls, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
  *cls = c->sf_cls.p;
  return VGS_OK;
}

// ----------------------------------------------------------------------------------------------------------------------- copy-out
// A tile context's records: the rows of the labels the source's rule selects, ascending, packed.  The rule's words and every wanted
// column come over in one go -- one wait for the whole record set.
template <typename Dec>
static vgs_status attr_copy_compact(vgs_ctx* c, const AttrSource<Dec>& S, const RowCol* col, int n_col, const AttrRecords& R) {
  const size_t K = (size_t)S.K;
  const uint32_t* rule_dev = nullptr;
  std::vector<uint32_t> rule(attr_rule_words(c, S, &rule_dev));
  std::vector<std::vector<char>> rows((size_t)n_col);
  hipError_t e = hipMemcpyAsync(rule.data(), rule_dev, rule.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  for (int i = 0; i < n_col && e == hipSuccess; ++i) {
    if (!col[i].dst) continue;
    rows[i].resize(K * col[i].row_bytes);
    e = hipMemcpyAsync(rows[i].data(), col[i].src, rows[i].size(), hipMemcpyDeviceToHost, c->stream);
  }
  const hipError_t waited = hipStreamSynchronize(c->stream);   // after a failed copy as well: the copies queued before it write into the vectors here
  VGS_HIP_TRY(c, e);
  VGS_HIP_TRY(c, waited);
  size_t n = 0;
  for (size_t k = 0; k < K; ++k) {
    if (!attr_has_record(S, rule.data(), k)) continue;
    if (R.label) R.label[n] = (int32_t)k;
    for (int i = 0; i < n_col; ++i)
      if (col[i].dst) memcpy((char*)col[i].dst + n * col[i].row_bytes, rows[i].data() + k * col[i].row_bytes, col[i].row_bytes);
    ++n;
  }
  if (R.n_records) *R.n_records = (int64_t)n;
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ drivers
// the K x n_channels tables of the field pass (from_moments fills them without a source)
static inline vgs_status attr_ensure_field_rows(vgs_ctx* c, size_t kc) {
  VGS_HIP_TRY(c, c->sf_anchor.ensure(kc)); VGS_HIP_TRY(c, c->sf_mean.ensure(kc)); VGS_HIP_TRY(c, c->sf_var.ensure(kc));
  VGS_HIP_TRY(c, c->sf_nvalid.ensure(kc)); VGS_HIP_TRY(c, c->sf_min.ensure(kc)); VGS_HIP_TRY(c, c->sf_max.ensure(kc));
  return VGS_OK;
}

// The field table of a source over field_dev (HBM, rows at stride_bytes): the anchors, then per group of SF_G channels the chunk partials
// and their fold.  R = NULL: k_sf_final's rows, dense, K x n_channels per column.  R given (tile contexts): k_sf_own_records' raw sums,
// compact.  Every destination may be NULL.
template <typename Dec>
static vgs_status attr_field_table(vgs_ctx* c, const AttrSource<Dec>& S, const float* field_dev, int32_t n_channels, int64_t stride_bytes,
                                   const AttrRecords* R, const AttrFieldOut& O) {
  if (!S.live) return VGS_OK;
  const uint32_t C = (uint32_t)n_channels, n_part = (uint32_t)S.n_chunks_max;
  const size_t kc = (size_t)S.K * C;
  const int64_t stride_f = stride_bytes / 4;
  VGS_HIP_TRY(c, c->sf_part.ensure((size_t)S.n_chunks_max * SF_G * SF_REC));
  vgs_status s = attr_ensure_field_rows(c, kc);
  if (s != VGS_OK || (s = attr_launch_anchor(c, S, field_dev, stride_f, C)) != VGS_OK) return s;
  for (uint32_t c0 = 0; c0 < C; c0 += SF_G) {
    const uint32_t ng = C - c0 < SF_G ? C - c0 : SF_G;
    if (S.chunks) attr_launch_chunks(c, S, field_dev, stride_f, C, c0, ng);
    if (R) sf_launch_own_records(c, S.seg_chunk, c->sf_part.p, n_part, S.K, C, c0, ng, c->sf_nvalid.p, c->sf_mean.p, c->sf_var.p, c->sf_min.p, c->sf_max.p);
    else sf_launch_final(c, S.seg_chunk, c->sf_part.p, n_part, S.K, C, c0, ng, c->sf_anchor.p, c->sf_nvalid.p, c->sf_mean.p, c->sf_var.p, c->sf_min.p, c->sf_max.p);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  const RowCol col[6] = {{O.n_valid, c->sf_nvalid.p, C * sizeof(int64_t)}, {O.anchor, c->sf_anchor.p, C * sizeof(double)},
                          {O.m1, c->sf_mean.p, C * sizeof(double)},         {O.m2, c->sf_var.p, C * sizeof(double)},
                          {O.vmin, c->sf_min.p, C * sizeof(float)},         {O.vmax, c->sf_max.p, C * sizeof(float)}};
  return R ? attr_copy_compact(c, S, col, 6, *R) : vgs_copy_rows(c, (size_t)S.K, col, 6);
}

// The class histogram of a source over cls_dev (HBM): the zeroed K x n_classes table and K out-of-range counts, the chunk counts added.
// R = NULL: k_sf_majority behind it, four dense columns.  R given (tile contexts): the counts as they are, compact.
template <typename Dec>
static vgs_status attr_hist_table(vgs_ctx* c, const AttrSource<Dec>& S, const int32_t* cls_dev, int32_t n_classes, const AttrRecords* R,
                                  const AttrHistOut& O) {
  if (!S.live) return VGS_OK;
  const size_t k = (size_t)S.K, nc = (size_t)n_classes, kc = k * nc;
  VGS_HIP_TRY(c, c->sf_hist.ensure(kc + 2 * k));
  if (!R) VGS_HIP_TRY(c, c->sf_maj.ensure(k));
  int64_t *d_hist = c->sf_hist.p, *d_out = d_hist + kc, *d_majc = d_out + k;
  VGS_HIP_TRY(c, hipMemsetAsync(d_hist, 0, (kc + k) * sizeof(int64_t), c->stream));
  vgs_status s = VGS_OK;
  if (S.chunks && (s = attr_launch_hist(c, S, cls_dev, (uint32_t)n_classes, (unsigned long long*)d_hist, (unsigned long long*)d_out)) != VGS_OK) return s;
  if (!R) sf_launch_majority(c, d_hist, n_classes, S.K, c->sf_maj.p, d_majc);
  VGS_HIP_TRY(c, hipGetLastError());
  const RowCol col[4] = {{O.hist, d_hist, nc * sizeof(int64_t)}, {O.n_outside, d_out, sizeof(int64_t)},
                          {O.majority, c->sf_maj.p, sizeof(int32_t)}, {O.majority_count, d_majc, sizeof(int64_t)}};
  return R ? attr_copy_compact(c, S, col, 2, *R) : vgs_copy_rows(c, k, col, 4);
}

#endif
