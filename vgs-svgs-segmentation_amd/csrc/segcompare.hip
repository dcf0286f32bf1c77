// segcompare.hip -- the sparse contingency table between the engine's point labels and a caller-supplied labelling of the same points
// (include/vgs.h: vgs_compare_labels, vgs_get_label_comparison).  Everything is an integer count or one fp64 quotient of counts, so the
// tables are bit-identical from call to call and from engine to engine whatever the order of the integer atomics below.
//
//   1. k_cmp_scan     one pass over ref: unannotated points and the largest id (two atomics per workgroup)          -> read-back 1
//   2. k_cmp_keys     labels and ref in input order (coalesced, no permutation): key = (L + 1) << gbits | g per annotated point, the
//                     row K + 1 for an unannotated one, so that the sort leaves those behind the n_ann keys that count;
//                     gbits = the bits of the largest id, and the sort runs over gbits + bits(K + 1) bits only
//   3. rocprim::radix_sort_keys; heads, inclusive scan, run starts: the cells in ascending (L, g) order             -> read-back 2
//   4. k_cmp_row_starts (a search per row), k_cmp_seg_rows: one wavefront per row L = -1 .. K-1 folds its contiguous cells, lane stride
//      then butterfly: seg_annotated, seg_refs, seg_best_ref / _n (the lowest id on a tie)
//   5. a stable sort of the cell indices by cell_ref (far fewer cells than points); heads, scan, starts: the ids    -> read-back 3
//      k_cmp_ref_rows: one wavefront per id over its cells (ascending label inside an id, the sort being stable): ref_points,
//      ref_dropped, ref_best_seg / _n (the lowest label on a tie) and ref_best_iou
//   6. k_cmp_seg_iou (a search of the best id per segment) and the summary sums, kept per wavefront and added once -> read-back 4
// A row and an id of any number of cells are read in chunks of 64 (the lane-stride loops).  Positions are uint32: N < 2^31.
// Scratch: own buffers only (cmp_*); labels, descriptors, boxes and graph are read-only here.
// vgs_compare_point_labels runs the same six steps over a labelling of the caller's instead of the point labels, K rows of the caller's;
// any negative label is the dropped row, and a label not below K is refused first (one pass on the device, csrc/pointseg.hip).
//
// The tiled driver (include/vgs_tiles.h) runs the two halves on different inputs.  Steps 1-3 over a rank's OWN points only
// (vgs_own_label_cells: k_cmp_scan_own is step 1 with the largest label beside the largest id, so that a label not below K is refused
// before a key is made), and steps 4-6 from a cell list that did not come from this context's points
// (vgs_label_comparison_from_cells).  That list -- the ranks' lists one after another -- holds a pair once per rank that saw it, so it is
// merged first, by the pipeline of steps 1-3 one level up:
//   a. k_cmp_cells_scan   one pass over the input cells: the largest id, the sum of the counts and the FIRST input that is not a cell
//                         (a segment outside -1 .. K-1, a negative id, a count below 1), at most three atomics per workgroup -> read-back
//   b. k_cmp_cells_keys   key = (seg + 1) << gbits | ref
//   c. rocprim::radix_sort_pairs of (key, count) over gbits + bits(K) bits; heads, inclusive scan, k_cmp_cell_starts as in step 3
//   d. k_cmp_cells_sums   one thread per merged cell walks its run and adds the int64 counts (integers: any order gives the same bits),
//                         and C(cell_n, 2) of the MERGED cell goes into the summary
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"

#define CMP_TB 256
#define CMP_WAVES (CMP_TB / 64)
#define CMP_SCAN_GRID 1024u  // workgroups of the pass over ref: four per compute unit
#define CMP_GRID_MAX 2048u   // workgroups of the folding kernels: each wavefront walks its items by grid stride and adds its sums once

// slots of cmp_meta (uint64 each)
enum { CM_UNANN = 0, CM_MAXID = 1, CM_NCELLS = 2, CM_NREFS = 3, CM_SEGS = 4, CM_SEGBEST = 5, CM_REFBEST = 6, CM_PAIRS_CELL = 7, CM_PAIRS_ROW = 8,
       CM_PAIRS_REF = 9, CM_DROPPED = 10, CM_TOTAL = 11, CM_BAD = 12, CM_MAXLAB = 13, CM_SLOTS = 16 };

typedef unsigned long long cmp_u64;

__device__ __forceinline__ cmp_u64 cmp_wave_sum(cmp_u64 v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ cmp_u64 cmp_pairs(cmp_u64 n) { return (n & 1ull) ? n * ((n - 1) >> 1) : (n >> 1) * (n - 1); }   // C(n, 2); 0 for n = 0

__global__ __launch_bounds__(CMP_TB) void k_cmp_scan(const int32_t* __restrict__ ref, int64_t N, cmp_u64* __restrict__ meta) {
  __shared__ cmp_u64 s_un[CMP_WAVES], s_mx[CMP_WAVES];
  cmp_u64 un = 0, mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * CMP_TB + threadIdx.x; i < N; i += (int64_t)gridDim.x * CMP_TB) {
    const int32_t g = ref[i];
    if (g < 0) ++un; else if ((cmp_u64)g > mx) mx = (cmp_u64)g;
  }
  un = cmp_wave_sum(un);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const cmp_u64 o = __shfl_xor(mx, m, 64); mx = o > mx ? o : mx; }
  if ((threadIdx.x & 63) == 0) { s_un[threadIdx.x >> 6] = un; s_mx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x != 0) return;   // two atomics per workgroup: thousands of them at one address would cost more than the pass itself
  for (int w = 1; w < CMP_WAVES; ++w) { un += s_un[w]; mx = s_mx[w] > mx ? s_mx[w] : mx; }
  if (un) atomicAdd(&meta[CM_UNANN], un);
  if (mx) atomicMax(&meta[CM_MAXID], mx);
}

__global__ __launch_bounds__(CMP_TB) void k_cmp_keys(const int32_t* __restrict__ labels, const int32_t* __restrict__ ref, int64_t N, uint32_t gbits,
                                                     uint32_t K, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * CMP_TB + threadIdx.x;
  if (i >= N) return;
  const int32_t g = ref[i];
  const int32_t l = labels[i];   // (any negative label is the row of the dropped points: a caller's labelling need not say -1)
  const uint64_t row = g < 0 ? (uint64_t)K + 1 : (l < 0 ? 0ull : (uint64_t)(uint32_t)l + 1);
  key[i] = (row << gbits) | (g < 0 ? 0ull : (uint64_t)(uint32_t)g);
}

template <typename T>
__global__ __launch_bounds__(CMP_TB) void k_cmp_heads(const T* __restrict__ key, uint32_t n, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * CMP_TB + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// run starts of the sorted point keys: cell c = inc - 1 of every head, with the pair the key holds
__global__ __launch_bounds__(CMP_TB) void k_cmp_cell_starts(const uint64_t* __restrict__ key, const uint32_t* __restrict__ head,
                                                            const uint32_t* __restrict__ inc, uint32_t n, uint32_t gbits, uint32_t* __restrict__ cstart,
                                                            int32_t* __restrict__ cell_seg, int32_t* __restrict__ cell_ref, cmp_u64* __restrict__ meta) {
  const uint32_t i = blockIdx.x * CMP_TB + threadIdx.x;
  if (i >= n) return;
  if (i == n - 1) meta[CM_NCELLS] = inc[i];
  if (!head[i]) return;
  const uint32_t cidx = inc[i] - 1;
  const uint64_t k = key[i];
  cstart[cidx] = i;
  cell_seg[cidx] = (int32_t)(uint32_t)(k >> gbits) - 1;
  cell_ref[cidx] = (int32_t)(uint32_t)(k & ((1ull << gbits) - 1));
}

__global__ __launch_bounds__(CMP_TB) void k_cmp_cell_counts(const uint32_t* __restrict__ cstart, uint32_t n_cells, uint32_t n_ann,
                                                            long long* __restrict__ cell_n, cmp_u64* __restrict__ meta) {
  cmp_u64 acc = 0;
  for (uint32_t i = blockIdx.x * CMP_TB + threadIdx.x; i < n_cells; i += gridDim.x * CMP_TB) {
    const uint32_t e = i + 1 < n_cells ? cstart[i + 1] : n_ann;
    const cmp_u64 n = e - cstart[i];
    cell_n[i] = (long long)n;
    acc += cmp_pairs(n);
  }
  acc = cmp_wave_sum(acc);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&meta[CM_PAIRS_CELL], acc);
}

// step 1 over a rank's own points (labels = pt_label + own_first, beside ref): the largest label + 1 as well, for the check against K
__global__ __launch_bounds__(CMP_TB) void k_cmp_scan_own(const int32_t* __restrict__ labels, const int32_t* __restrict__ ref, int64_t N,
                                                         cmp_u64* __restrict__ meta) {
  __shared__ cmp_u64 s_un[CMP_WAVES], s_mx[CMP_WAVES], s_ml[CMP_WAVES];
  cmp_u64 un = 0, mx = 0, ml = 0;
  for (int64_t i = (int64_t)blockIdx.x * CMP_TB + threadIdx.x; i < N; i += (int64_t)gridDim.x * CMP_TB) {
    const int32_t g = ref[i];
    const int32_t l = labels[i];
    if (g < 0) ++un; else if ((cmp_u64)g > mx) mx = (cmp_u64)g;
    if (l >= 0 && (cmp_u64)l + 1 > ml) ml = (cmp_u64)l + 1;
  }
  un = cmp_wave_sum(un);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const cmp_u64 o = __shfl_xor(mx, m, 64); mx = o > mx ? o : mx;
    const cmp_u64 p = __shfl_xor(ml, m, 64); ml = p > ml ? p : ml;
  }
  if ((threadIdx.x & 63) == 0) { s_un[threadIdx.x >> 6] = un; s_mx[threadIdx.x >> 6] = mx; s_ml[threadIdx.x >> 6] = ml; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < CMP_WAVES; ++w) { un += s_un[w]; mx = s_mx[w] > mx ? s_mx[w] : mx; ml = s_ml[w] > ml ? s_ml[w] : ml; }
  if (un) atomicAdd(&meta[CM_UNANN], un);
  if (mx) atomicMax(&meta[CM_MAXID], mx);
  if (ml) atomicMax(&meta[CM_MAXLAB], ml);
}

// One pass over n_in input cells.  A count is clamped to 2^32 + 1 before it is added, so that 2^31 of them cannot wrap the sum and a total
// above the limit of 2^32 is still seen as one.  CM_BAD holds n_in - i for the first input i that is not a cell, 0 when all are.
#define CMP_COUNT_CLAMP 0x100000001ull
__global__ __launch_bounds__(CMP_TB) void k_cmp_cells_scan(const int32_t* __restrict__ seg, const int32_t* __restrict__ ref,
                                                           const long long* __restrict__ cnt, uint32_t n_in, uint32_t K,
                                                           cmp_u64* __restrict__ meta) {
  __shared__ cmp_u64 s_tot[CMP_WAVES], s_mx[CMP_WAVES], s_bad[CMP_WAVES];
  cmp_u64 tot = 0, mx = 0, bad = 0;
  for (uint32_t i = blockIdx.x * CMP_TB + threadIdx.x; i < n_in; i += gridDim.x * CMP_TB) {
    const int32_t s = seg[i], g = ref[i];
    const long long n = cnt[i];
    if (s < -1 || (int64_t)s >= (int64_t)K || g < 0 || n < 1) {
      const cmp_u64 b = (cmp_u64)(n_in - i);
      if (b > bad) bad = b;
      continue;
    }
    if ((cmp_u64)g > mx) mx = (cmp_u64)g;
    tot += (cmp_u64)n < CMP_COUNT_CLAMP ? (cmp_u64)n : CMP_COUNT_CLAMP;
  }
  tot = cmp_wave_sum(tot);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const cmp_u64 o = __shfl_xor(mx, m, 64); mx = o > mx ? o : mx;
    const cmp_u64 p = __shfl_xor(bad, m, 64); bad = p > bad ? p : bad;
  }
  if ((threadIdx.x & 63) == 0) { s_tot[threadIdx.x >> 6] = tot; s_mx[threadIdx.x >> 6] = mx; s_bad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < CMP_WAVES; ++w) { tot += s_tot[w]; mx = s_mx[w] > mx ? s_mx[w] : mx; bad = s_bad[w] > bad ? s_bad[w] : bad; }
  if (tot) atomicAdd(&meta[CM_TOTAL], tot);
  if (mx) atomicMax(&meta[CM_MAXID], mx);
  if (bad) atomicMax(&meta[CM_BAD], bad);
}

__global__ __launch_bounds__(CMP_TB) void k_cmp_cells_keys(const int32_t* __restrict__ seg, const int32_t* __restrict__ ref, uint32_t n_in,
                                                           uint32_t gbits, uint64_t* __restrict__ key) {
  const uint32_t i = blockIdx.x * CMP_TB + threadIdx.x;
  if (i >= n_in) return;
  key[i] = ((uint64_t)(uint32_t)(seg[i] + 1) << gbits) | (uint64_t)(uint32_t)ref[i];
}

// the merged cell i = the run [cstart[i], cstart[i + 1]) of the sorted input cells: its count is the sum of theirs
__global__ __launch_bounds__(CMP_TB) void k_cmp_cells_sums(const uint32_t* __restrict__ cstart, uint32_t n_cells, uint32_t n_in,
                                                           const long long* __restrict__ cnt, long long* __restrict__ cell_n,
                                                           cmp_u64* __restrict__ meta) {
  cmp_u64 acc = 0;
  for (uint32_t i = blockIdx.x * CMP_TB + threadIdx.x; i < n_cells; i += gridDim.x * CMP_TB) {
    const uint32_t e = i + 1 < n_cells ? cstart[i + 1] : n_in;
    cmp_u64 n = 0;
    for (uint32_t j = cstart[i]; j < e; ++j) n += (cmp_u64)cnt[j];
    cell_n[i] = (long long)n;
    acc += cmp_pairs(n);
  }
  acc = cmp_wave_sum(acc);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&meta[CM_PAIRS_CELL], acc);
}

// rowstart[r] = the first cell whose row (label + 1) is >= r, r = 0 .. K + 1
__global__ __launch_bounds__(CMP_TB) void k_cmp_row_starts(const int32_t* __restrict__ cell_seg, uint32_t n_cells, uint32_t K,
                                                           uint32_t* __restrict__ rowstart) {
  const uint64_t r = (uint64_t)blockIdx.x * CMP_TB + threadIdx.x;
  if (r > (uint64_t)K + 1) return;
  uint32_t lo = 0, hi = n_cells;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)cell_seg[mid] + 1 < (int64_t)r) lo = mid + 1; else hi = mid;
  }
  rowstart[r] = lo;
}

// one wavefront per row r = 0 .. K (label r - 1): lane stride over its cells, then butterfly
__global__ __launch_bounds__(CMP_TB) void k_cmp_seg_rows(const uint32_t* __restrict__ rowstart, const int32_t* __restrict__ cell_ref,
                                                         const long long* __restrict__ cell_n, uint32_t K, long long* __restrict__ seg_annotated,
                                                         int32_t* __restrict__ seg_refs, int32_t* __restrict__ seg_best_ref,
                                                         long long* __restrict__ seg_best_n, cmp_u64* __restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n_waves = (uint64_t)gridDim.x * CMP_WAVES;
  cmp_u64 s_segs = 0, s_best = 0, s_pairs = 0, s_drop = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * CMP_WAVES + (threadIdx.x >> 6); r <= (uint64_t)K; r += n_waves) {
    const uint32_t lo = rowstart[r], hi = rowstart[r + 1];
    cmp_u64 a = 0, best = 0;
    uint32_t arg = 0xffffffffu;
    for (uint32_t j = lo + lane; j < hi; j += 64) {   // ascending id per lane: a strictly larger count only
      const cmp_u64 n = (cmp_u64)cell_n[j];
      a += n;
      if (n > best) { best = n; arg = (uint32_t)cell_ref[j]; }
    }
    a = cmp_wave_sum(a);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const cmp_u64 ob = __shfl_xor(best, m, 64);
      const uint32_t oa = __shfl_xor(arg, m, 64);
      if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane != 0) continue;
    s_pairs += cmp_pairs(a);
    if (r == 0) { s_drop += a; continue; }
    seg_annotated[r - 1] = (long long)a;
    seg_refs[r - 1] = (int32_t)(hi - lo);
    seg_best_ref[r - 1] = best > 0 ? (int32_t)arg : -1;
    seg_best_n[r - 1] = (long long)best;
    s_segs += a > 0 ? 1 : 0;
    s_best += best;
  }
  if (lane != 0) return;
  if (s_segs) atomicAdd(&meta[CM_SEGS], s_segs);
  if (s_best) atomicAdd(&meta[CM_SEGBEST], s_best);
  if (s_pairs) atomicAdd(&meta[CM_PAIRS_ROW], s_pairs);
  if (s_drop) atomicAdd(&meta[CM_DROPPED], s_drop);
}

__global__ __launch_bounds__(CMP_TB) void k_cmp_ref_keys(const int32_t* __restrict__ cell_ref, uint32_t n_cells, uint32_t* __restrict__ rkey,
                                                         uint32_t* __restrict__ ridx) {
  const uint32_t i = blockIdx.x * CMP_TB + threadIdx.x;
  if (i >= n_cells) return;
  rkey[i] = (uint32_t)cell_ref[i];
  ridx[i] = i;
}

__global__ __launch_bounds__(CMP_TB) void k_cmp_ref_starts(const uint32_t* __restrict__ rkey, const uint32_t* __restrict__ head,
                                                           const uint32_t* __restrict__ inc, uint32_t n, uint32_t* __restrict__ rstart,
                                                           int32_t* __restrict__ ref_id, cmp_u64* __restrict__ meta) {
  const uint32_t i = blockIdx.x * CMP_TB + threadIdx.x;
  if (i >= n) return;
  if (i == n - 1) meta[CM_NREFS] = inc[i];
  if (!head[i]) return;
  rstart[inc[i] - 1] = i;
  ref_id[inc[i] - 1] = (int32_t)rkey[i];
}

// one wavefront per id: lane stride over its cells (ascending label), then butterfly
__global__ __launch_bounds__(CMP_TB) void k_cmp_ref_rows(const uint32_t* __restrict__ rstart, uint32_t G, uint32_t n_cells,
                                                         const uint32_t* __restrict__ ridx, const int32_t* __restrict__ cell_seg,
                                                         const long long* __restrict__ cell_n, const long long* __restrict__ seg_annotated,
                                                         long long* __restrict__ ref_points, long long* __restrict__ ref_dropped,
                                                         int32_t* __restrict__ ref_best_seg, long long* __restrict__ ref_best_n,
                                                         double* __restrict__ ref_best_iou, cmp_u64* __restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n_waves = (uint64_t)gridDim.x * CMP_WAVES;
  cmp_u64 s_best = 0, s_pairs = 0;
  for (uint64_t g = (uint64_t)blockIdx.x * CMP_WAVES + (threadIdx.x >> 6); g < (uint64_t)G; g += n_waves) {
    const uint32_t lo = rstart[g], hi = g + 1 < (uint64_t)G ? rstart[g + 1] : n_cells;
    cmp_u64 pts = 0, drop = 0, best = 0;
    uint32_t arg = 0xffffffffu;
    for (uint32_t j = lo + lane; j < hi; j += 64) {
      const uint32_t ci = ridx[j];
      const cmp_u64 n = (cmp_u64)cell_n[ci];
      const int32_t s = cell_seg[ci];
      pts += n;
      if (s < 0) drop += n;
      else if (n > best) { best = n; arg = (uint32_t)s; }
    }
    pts = cmp_wave_sum(pts);
    drop = cmp_wave_sum(drop);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const cmp_u64 ob = __shfl_xor(best, m, 64);
      const uint32_t oa = __shfl_xor(arg, m, 64);
      if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane != 0) continue;
    ref_points[g] = (long long)pts;
    ref_dropped[g] = (long long)drop;
    ref_best_seg[g] = best > 0 ? (int32_t)arg : -1;
    ref_best_n[g] = (long long)best;
    ref_best_iou[g] = best > 0 ? (double)(long long)best / (double)(seg_annotated[arg] + (long long)pts - (long long)best) : 0.0;
    s_best += best;
    s_pairs += cmp_pairs(pts);
  }
  if (lane != 0) return;
  if (s_best) atomicAdd(&meta[CM_REFBEST], s_best);
  if (s_pairs) atomicAdd(&meta[CM_PAIRS_REF], s_pairs);
}

__global__ __launch_bounds__(CMP_TB) void k_cmp_seg_iou(uint32_t K, const int32_t* __restrict__ seg_best_ref, const long long* __restrict__ seg_best_n,
                                                        const long long* __restrict__ seg_annotated, const int32_t* __restrict__ ref_id,
                                                        const long long* __restrict__ ref_points, uint32_t G, double* __restrict__ seg_best_iou) {
  const uint32_t k = blockIdx.x * CMP_TB + threadIdx.x;
  if (k >= K) return;
  const int32_t id = seg_best_ref[k];
  double iou = 0.0;
  if (id >= 0 && G > 0) {
    uint32_t lo = 0, hi = G - 1;   // the id is in the table: the first row with ref_id >= id
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ref_id[mid] < id) lo = mid + 1; else hi = mid; }
    const long long n = seg_best_n[k];
    iou = (double)n / (double)(seg_annotated[k] + ref_points[lo] - n);
  }
  seg_best_iou[k] = iou;
}

static inline unsigned cmp_grid(uint64_t n) { return (unsigned)((n + CMP_TB - 1) / CMP_TB); }
static inline unsigned cmp_fold_grid(uint64_t items_per_block_unit) {
  const uint64_t g = items_per_block_unit < 1 ? 1 : items_per_block_unit;
  return (unsigned)(g < CMP_GRID_MAX ? g : CMP_GRID_MAX);
}
static inline unsigned cmp_bits(uint64_t v) { unsigned b = 1; while (b < 64 && (v >> b) != 0) ++b; return b; }   // v < 2^b, b >= 1

static vgs_status cmp_check(vgs_ctx* c, const char* fn, const int32_t* ref, int64_t n) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of its segments; a comparison needs the whole cloud in one context";
    return VGS_E_STATE;
  }
  if (n != c->N) {
    c->err = std::string(fn) + ": n = " + std::to_string(n) + " must equal the number of points of the cloud, " + std::to_string(c->N);
    return VGS_E_ARG;
  }
  if (!ref && n > 0) { c->err = std::string(fn) + ": ref is NULL"; return VGS_E_ARG; }
  return VGS_OK;
}

// steps 2 and 3: the cells of N points (labels beside ref, both on the device) into cmp_cell_i32 (cell_seg | cell_ref at a stride of n_ann)
// and cmp_cell_n, after step 1 gave n_ann and the largest id
static vgs_status cmp_point_cells(vgs_ctx* c, const int32_t* labels_dev, const int32_t* ref_dev, int64_t N, int64_t K, uint32_t n_ann, unsigned gbits,
                                  cmp_u64* meta, uint64_t* m, uint32_t& n_cells) {
  n_cells = 0;
  if (n_ann > 0) {
    VGS_HIP_TRY(c, c->cmp_key.ensure(2 * (size_t)N)); VGS_HIP_TRY(c, c->cmp_work.ensure(2 * (size_t)n_ann));
    uint64_t *key_in = c->cmp_key.p, *key_out = key_in + N;
    uint32_t *head = c->cmp_work.p, *inc = head + n_ann;
    hipLaunchKernelGGL(k_cmp_keys, dim3(cmp_grid((uint64_t)N)), dim3(CMP_TB), 0, c->stream, labels_dev, ref_dev, N, gbits, (uint32_t)K, key_in);
    const unsigned bits = gbits + cmp_bits((uint64_t)K + 1);   // rows 0 .. K + 1
    size_t t_sort = 0, t_scan = 0;
    VGS_HIP_TRY(c, rocprim::radix_sort_keys(nullptr, t_sort, key_in, key_out, (size_t)N, 0, bits, c->stream));
    VGS_HIP_TRY(c, rocprim::inclusive_scan(nullptr, t_scan, head, inc, (size_t)n_ann, rocprim::plus<uint32_t>(), c->stream));
    VGS_HIP_TRY(c, c->cmp_tmp.ensure(std::max(t_sort, t_scan)));
    VGS_HIP_TRY(c, rocprim::radix_sort_keys(c->cmp_tmp.p, t_sort, key_in, key_out, (size_t)N, 0, bits, c->stream));
    hipLaunchKernelGGL(k_cmp_heads<uint64_t>, dim3(cmp_grid(n_ann)), dim3(CMP_TB), 0, c->stream, key_out, n_ann, head);
    VGS_HIP_TRY(c, rocprim::inclusive_scan(c->cmp_tmp.p, t_scan, head, inc, (size_t)n_ann, rocprim::plus<uint32_t>(), c->stream));
    // the cell tables are sized before their number is known: at most one cell per annotated point
    VGS_HIP_TRY(c, c->cmp_cstart.ensure(n_ann)); VGS_HIP_TRY(c, c->cmp_cell_i32.ensure(2 * (size_t)n_ann)); VGS_HIP_TRY(c, c->cmp_cell_n.ensure(n_ann));
    int32_t *cell_seg = c->cmp_cell_i32.p, *cell_ref = cell_seg + n_ann;
    hipLaunchKernelGGL(k_cmp_cell_starts, dim3(cmp_grid(n_ann)), dim3(CMP_TB), 0, c->stream, key_out, head, inc, n_ann, gbits, c->cmp_cstart.p, cell_seg,
                       cell_ref, meta);
    VGS_HIP_TRY(c, hipGetLastError());
    VGS_READBACK(c, &m[CM_NCELLS], meta + CM_NCELLS, sizeof(uint64_t));   // read-back 2: the number of cells
    n_cells = (uint32_t)m[CM_NCELLS];
    hipLaunchKernelGGL(k_cmp_cell_counts, dim3(cmp_fold_grid(cmp_grid(n_cells))), dim3(CMP_TB), 0, c->stream, c->cmp_cstart.p, n_cells, n_ann,
                       (long long*)c->cmp_cell_n.p, meta);
  }
  c->cmp_ann = n_ann;
  return VGS_OK;
}

// steps 4 to 6: the segment table of K rows, the reference table and the summary from the n_cells cells in cmp_cell_i32 (at a stride of
// `stride`) and cmp_cell_n, whichever pipeline left them there; `total` and `unann` are summary[0] and summary[1].  The tables become the
// context's last comparison.
static vgs_status cmp_cell_tables(vgs_ctx* c, int64_t K, uint32_t stride, uint32_t n_cells, unsigned gbits, int64_t total, int64_t unann, cmp_u64* meta,
                                  uint64_t* m) {
  const size_t k1 = (size_t)K > 0 ? (size_t)K : 1;
  VGS_HIP_TRY(c, c->cmp_seg_i64.ensure(2 * k1)); VGS_HIP_TRY(c, c->cmp_seg_i32.ensure(2 * k1)); VGS_HIP_TRY(c, c->cmp_seg_iou.ensure(k1));
  VGS_HIP_TRY(c, c->cmp_rowstart.ensure((size_t)K + 2));
  long long *seg_ann = (long long*)c->cmp_seg_i64.p, *seg_bn = seg_ann + k1;
  int32_t *seg_refs = c->cmp_seg_i32.p, *seg_br = seg_refs + k1;
  uint32_t G = 0;
  const int32_t *cell_seg = c->cmp_cell_i32.p, *cell_ref = stride > 0 ? cell_seg + stride : nullptr;
  const long long* cell_n = (const long long*)c->cmp_cell_n.p;
  hipLaunchKernelGGL(k_cmp_row_starts, dim3(cmp_grid((uint64_t)K + 2)), dim3(CMP_TB), 0, c->stream, cell_seg, n_cells, (uint32_t)K, c->cmp_rowstart.p);
  hipLaunchKernelGGL(k_cmp_seg_rows, dim3(cmp_fold_grid(((uint64_t)K + CMP_WAVES) / CMP_WAVES)), dim3(CMP_TB), 0, c->stream, c->cmp_rowstart.p, cell_ref,
                     cell_n, (uint32_t)K, seg_ann, seg_refs, seg_br, seg_bn, meta);
  VGS_HIP_TRY(c, hipGetLastError());
  if (n_cells > 0) {
    VGS_HIP_TRY(c, c->cmp_rsort.ensure(4 * (size_t)n_cells));
    uint32_t *rk_in = c->cmp_rsort.p, *rk_out = rk_in + n_cells, *ri_in = rk_out + n_cells, *ri_out = ri_in + n_cells;
    uint32_t *head = c->cmp_work.p, *inc = head + stride;   // (free again: n_cells <= stride)
    hipLaunchKernelGGL(k_cmp_ref_keys, dim3(cmp_grid(n_cells)), dim3(CMP_TB), 0, c->stream, cell_ref, n_cells, rk_in, ri_in);
    size_t t_sort = 0, t_scan2 = 0;
    VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, rk_in, rk_out, ri_in, ri_out, (size_t)n_cells, 0, gbits, c->stream));
    VGS_HIP_TRY(c, rocprim::inclusive_scan(nullptr, t_scan2, head, inc, (size_t)n_cells, rocprim::plus<uint32_t>(), c->stream));
    VGS_HIP_TRY(c, c->cmp_tmp.ensure(std::max(t_sort, t_scan2)));
    VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->cmp_tmp.p, t_sort, rk_in, rk_out, ri_in, ri_out, (size_t)n_cells, 0, gbits, c->stream));
    hipLaunchKernelGGL(k_cmp_heads<uint32_t>, dim3(cmp_grid(n_cells)), dim3(CMP_TB), 0, c->stream, rk_out, n_cells, head);
    VGS_HIP_TRY(c, rocprim::inclusive_scan(c->cmp_tmp.p, t_scan2, head, inc, (size_t)n_cells, rocprim::plus<uint32_t>(), c->stream));
    // at most one id per cell
    VGS_HIP_TRY(c, c->cmp_rstart.ensure(n_cells)); VGS_HIP_TRY(c, c->cmp_ref_i32.ensure(2 * (size_t)n_cells));
    VGS_HIP_TRY(c, c->cmp_ref_i64.ensure(3 * (size_t)n_cells)); VGS_HIP_TRY(c, c->cmp_ref_iou.ensure(n_cells));
    int32_t *ref_id = c->cmp_ref_i32.p, *ref_bs = ref_id + n_cells;
    long long *ref_pts = (long long*)c->cmp_ref_i64.p, *ref_drop = ref_pts + n_cells, *ref_bn = ref_drop + n_cells;
    hipLaunchKernelGGL(k_cmp_ref_starts, dim3(cmp_grid(n_cells)), dim3(CMP_TB), 0, c->stream, rk_out, head, inc, n_cells, c->cmp_rstart.p, ref_id, meta);
    VGS_HIP_TRY(c, hipGetLastError());
    VGS_READBACK(c, &m[CM_NREFS], meta + CM_NREFS, sizeof(uint64_t));   // read-back 3: the number of ids
    G = (uint32_t)m[CM_NREFS];
    hipLaunchKernelGGL(k_cmp_ref_rows, dim3(cmp_fold_grid(((uint64_t)G + CMP_WAVES - 1) / CMP_WAVES)), dim3(CMP_TB), 0, c->stream, c->cmp_rstart.p, G, n_cells,
                       ri_out, cell_seg, cell_n, seg_ann, ref_pts, ref_drop, ref_bs, ref_bn, c->cmp_ref_iou.p, meta);
  }
  if (K > 0)
    hipLaunchKernelGGL(k_cmp_seg_iou, dim3(cmp_grid((uint64_t)K)), dim3(CMP_TB), 0, c->stream, (uint32_t)K, seg_br, seg_bn, seg_ann, c->cmp_ref_i32.p,
                       (const long long*)c->cmp_ref_i64.p, G, c->cmp_seg_iou.p);
  VGS_HIP_TRY(c, hipGetLastError());
  VGS_READBACK(c, m, meta, CM_SLOTS * sizeof(uint64_t));   // read-back 4: the summary sums
  int64_t* s = c->cmp_summary;
  s[0] = total; s[1] = unann; s[2] = (int64_t)m[CM_DROPPED]; s[3] = (int64_t)G; s[4] = (int64_t)n_cells;
  s[5] = (int64_t)m[CM_SEGS]; s[6] = (int64_t)m[CM_SEGBEST]; s[7] = (int64_t)m[CM_REFBEST]; s[8] = (int64_t)m[CM_PAIRS_CELL];
  s[9] = (int64_t)m[CM_PAIRS_ROW]; s[10] = (int64_t)m[CM_PAIRS_REF]; s[11] = 0;
  c->cmp_cells = n_cells; c->cmp_refs = G;
  c->cmp_valid = true;
  return VGS_OK;
}

// the three tables from a device labelling into the cmp_* buffers; sizes and summary into the context.  labels_dev, K: the labels that are
// scored and their number of rows -- the point labels and the kept count, or a caller's (vgs_compare_point_labels)
static vgs_status cmp_build(vgs_ctx* c, const int32_t* ref_dev, const int32_t* labels_dev, int64_t K) {
  c->cmp_valid = false; c->cmp_own_cells = -1;
  const int64_t N = c->N;
  c->cmp_cells = 0; c->cmp_refs = 0; c->cmp_K = K;
  for (int i = 0; i < 12; ++i) c->cmp_summary[i] = 0;
  if (N == 0) { c->cmp_K = 0; c->cmp_valid = true; return VGS_OK; }
  VGS_HIP_TRY(c, c->cmp_meta.ensure(CM_SLOTS));
  cmp_u64* meta = (cmp_u64*)c->cmp_meta.p;
  VGS_HIP_TRY(c, hipMemsetAsync(meta, 0, CM_SLOTS * sizeof(uint64_t), c->stream));
  hipLaunchKernelGGL(k_cmp_scan, dim3(std::min(cmp_grid((uint64_t)N), CMP_SCAN_GRID)), dim3(CMP_TB), 0, c->stream, ref_dev, N, meta);
  VGS_HIP_TRY(c, hipGetLastError());
  uint64_t m[CM_SLOTS];
  VGS_READBACK(c, m, meta, 2 * sizeof(uint64_t));   // read-back 1: unannotated points, the largest id
  const uint32_t n_ann = (uint32_t)((uint64_t)N - m[CM_UNANN]);
  const unsigned gbits = cmp_bits(m[CM_MAXID]);
  uint32_t n_cells = 0;
  vgs_status s = cmp_point_cells(c, labels_dev, ref_dev, N, K, n_ann, gbits, meta, m, n_cells);
  if (s != VGS_OK) return s;
  return cmp_cell_tables(c, K, n_ann, n_cells, gbits, (int64_t)n_ann, (int64_t)m[CM_UNANN], meta, m);
}

static void cmp_report(vgs_ctx* c, int64_t* n_cells, int64_t* n_refs, int64_t* summary) {
  if (n_cells) *n_cells = c->cmp_cells;
  if (n_refs) *n_refs = c->cmp_refs;
  if (summary) std::copy(c->cmp_summary, c->cmp_summary + 12, summary);
}

extern "C" vgs_status vgs_compare_labels_device(vgs_ctx* c, const int32_t* ref_dev, int64_t n, int64_t* n_cells, int64_t* n_refs, int64_t* summary) {
  if (!c) return VGS_E_ARG;
  vgs_status s = cmp_check(c, "vgs_compare_labels_device", ref_dev, n);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if ((s = cmp_build(c, ref_dev, c->pt_label.p, c->counts[VGS_N_KEPT])) != VGS_OK) return s;
  cmp_report(c, n_cells, n_refs, summary);
  return VGS_OK;
}

extern "C" vgs_status vgs_compare_labels(vgs_ctx* c, const int32_t* ref_host, int64_t n, int64_t* n_cells, int64_t* n_refs, int64_t* summary) {
  if (!c) return VGS_E_ARG;
  vgs_status s = cmp_check(c, "vgs_compare_labels", ref_host, n);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (n > 0) {
    VGS_HIP_TRY(c, c->cmp_ref.ensure((size_t)n));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->cmp_ref.p, ref_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
  }
  if ((s = cmp_build(c, c->cmp_ref.p, c->pt_label.p, c->counts[VGS_N_KEPT])) != VGS_OK) return s;
  cmp_report(c, n_cells, n_refs, summary);
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ a caller's labelling against ref
// The same tables with L[i] = seg_labels[i] (any negative label the dropped row) and K rows of the caller's: the argument checks, one
// pass that refuses a label not below K (pointseg.hip), then cmp_build over that array instead of the point labels.
static vgs_status cmp_point_check(vgs_ctx* c, const char* fn, const int32_t* seg, int64_t K, const int32_t* ref, int64_t n) {
  vgs_status s = cmp_check(c, fn, ref, n);
  if (s != VGS_OK) return s;
  if (!seg && n > 0) { c->err = std::string(fn) + ": seg_labels is NULL"; return VGS_E_ARG; }
  if (K < 0 || K > (int64_t)0x7fffffff) { c->err = std::string(fn) + ": K = " + std::to_string(K) + " is out of range"; return VGS_E_ARG; }
  return VGS_OK;
}

extern "C" vgs_status vgs_compare_point_labels_device(vgs_ctx* c, const int32_t* seg_dev, int64_t K, const int32_t* ref_dev, int64_t n, int64_t* n_cells,
                                                      int64_t* n_refs, int64_t* summary) {
  if (!c) return VGS_E_ARG;
  const char* fn = "vgs_compare_point_labels_device";
  vgs_status s = cmp_point_check(c, fn, seg_dev, K, ref_dev, n);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if ((s = vgs_check_label_range(c, fn, seg_dev, n, K)) != VGS_OK) return s;
  if ((s = cmp_build(c, ref_dev, seg_dev, K)) != VGS_OK) return s;
  cmp_report(c, n_cells, n_refs, summary);
  return VGS_OK;
}

extern "C" vgs_status vgs_compare_point_labels(vgs_ctx* c, const int32_t* seg_host, int64_t K, const int32_t* ref_host, int64_t n, int64_t* n_cells,
                                               int64_t* n_refs, int64_t* summary) {
  if (!c) return VGS_E_ARG;
  const char* fn = "vgs_compare_point_labels";
  vgs_status s = cmp_point_check(c, fn, seg_host, K, ref_host, n);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const int32_t* seg_dev = nullptr;
  if ((s = vgs_upload_point_labels(c, seg_host, n, &seg_dev)) != VGS_OK) return s;
  if ((s = vgs_check_label_range(c, fn, seg_dev, n, K)) != VGS_OK) return s;
  if (n > 0) {
    VGS_HIP_TRY(c, c->cmp_ref.ensure((size_t)n));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->cmp_ref.p, ref_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
  }
  if ((s = cmp_build(c, c->cmp_ref.p, seg_dev, K)) != VGS_OK) return s;
  cmp_report(c, n_cells, n_refs, summary);
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ tile contexts (include/vgs_tiles.h)
static vgs_status cmp_own_check(vgs_ctx* c, const char* fn, int64_t K, const int32_t* ref, int64_t n_own) {
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
  if (!ref && n_own > 0) { c->err = std::string(fn) + ": ref is NULL"; return VGS_E_ARG; }
  if (c->own_first + n_own > c->N) {
    c->err = std::string(fn) + ": the own point range ends at " + std::to_string(c->own_first + n_own) + ", the cloud holds " + std::to_string(c->N) + " points";
    return VGS_E_ARG;
  }
  return VGS_OK;
}

// steps 1-3 over the own points: pt_label[own_first + i] beside ref[i].  The cells stay in cmp_cell_i32 / cmp_cell_n (cmp_own_cells of
// them, at a stride of cmp_ann) until vgs_get_own_label_cells copies them or another comparison takes the buffers.
// seg_dev: the caller's labels of the own points in their order (vgs_own_point_label_cells; checked against K before), or nullptr for
// the engine's own point labels.
static vgs_status cmp_own_cells(vgs_ctx* c, const char* fn, int64_t K, const int32_t* ref_dev, int64_t* n_cells_out, int64_t* n_unann,
                                const int32_t* seg_dev = nullptr) {
  c->cmp_valid = false; c->cmp_own_cells = -1;
  if (n_cells_out) *n_cells_out = 0;
  if (n_unann) *n_unann = 0;
  const int64_t N = c->n_own;
  if (N == 0) { c->cmp_ann = 0; c->cmp_own_cells = 0; return VGS_OK; }
  vgs_status s = seg_dev ? VGS_OK : vgs_ensure_point_labels(c);   // a tile's merge stage leaves the scatter to whoever asks first
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, c->cmp_meta.ensure(CM_SLOTS));
  cmp_u64* meta = (cmp_u64*)c->cmp_meta.p;
  const int32_t* labels = seg_dev ? seg_dev : c->pt_label.p + c->own_first;
  VGS_HIP_TRY(c, hipMemsetAsync(meta, 0, CM_SLOTS * sizeof(uint64_t), c->stream));
  hipLaunchKernelGGL(k_cmp_scan_own, dim3(std::min(cmp_grid((uint64_t)N), CMP_SCAN_GRID)), dim3(CMP_TB), 0, c->stream, labels, ref_dev, N, meta);
  VGS_HIP_TRY(c, hipGetLastError());
  uint64_t m[CM_SLOTS];
  VGS_READBACK(c, m, meta, CM_SLOTS * sizeof(uint64_t));   // unannotated points, the largest id, the largest label + 1
  if ((int64_t)m[CM_MAXLAB] > K) {
    c->err = std::string(fn) + ": an own point has label " + std::to_string((int64_t)m[CM_MAXLAB] - 1) + ", not below K = " + std::to_string(K);
    return VGS_E_ARG;
  }
  const uint32_t n_ann = (uint32_t)((uint64_t)N - m[CM_UNANN]);
  uint32_t n_cells = 0;
  if ((s = cmp_point_cells(c, labels, ref_dev, N, K, n_ann, cmp_bits(m[CM_MAXID]), meta, m, n_cells)) != VGS_OK) return s;
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // ref is the caller's again
  c->cmp_own_cells = n_cells;
  if (n_cells_out) *n_cells_out = n_cells;
  if (n_unann) *n_unann = (int64_t)m[CM_UNANN];
  return VGS_OK;
}

extern "C" vgs_status vgs_own_label_cells_device(vgs_ctx* c, int64_t K, const int32_t* ref_dev, int64_t n_own, int64_t* n_cells, int64_t* n_unannotated) {
  if (!c) return VGS_E_ARG;
  vgs_status s = cmp_own_check(c, "vgs_own_label_cells_device", K, ref_dev, n_own);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  return cmp_own_cells(c, "vgs_own_label_cells_device", K, ref_dev, n_cells, n_unannotated);
}

extern "C" vgs_status vgs_own_label_cells(vgs_ctx* c, int64_t K, const int32_t* ref_host, int64_t n_own, int64_t* n_cells, int64_t* n_unannotated) {
  if (!c) return VGS_E_ARG;
  vgs_status s = cmp_own_check(c, "vgs_own_label_cells", K, ref_host, n_own);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (n_own > 0) {
    VGS_HIP_TRY(c, c->cmp_ref.ensure((size_t)n_own));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->cmp_ref.p, ref_host, (size_t)n_own * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
  }
  return cmp_own_cells(c, "vgs_own_label_cells", K, c->cmp_ref.p, n_cells, n_unannotated);
}

// The same cells with L[i] = seg_labels[i] (a caller's labelling of the own points, K rows of the caller's; any negative label the dropped
// row) instead of the point labels: purely index-wise, so a non-finite own point takes part.  A label not below K is refused first, the
// message naming the first own index and its value (pointseg.hip).  vgs_get_own_label_cells serves the cells.
static vgs_status cmp_own_point_check(vgs_ctx* c, const char* fn, int64_t K, const int32_t* seg, const int32_t* ref, int64_t n_own) {
  vgs_status s = cmp_own_check(c, fn, K, ref, n_own);
  if (s != VGS_OK) return s;
  if (!seg && n_own > 0) { c->err = std::string(fn) + ": seg_labels is NULL"; return VGS_E_ARG; }
  return VGS_OK;
}

extern "C" vgs_status vgs_own_point_label_cells_device(vgs_ctx* c, int64_t K, const int32_t* seg_dev, const int32_t* ref_dev, int64_t n_own,
                                                       int64_t* n_cells, int64_t* n_unannotated) {
  if (!c) return VGS_E_ARG;
  const char* fn = "vgs_own_point_label_cells_device";
  vgs_status s = cmp_own_point_check(c, fn, K, seg_dev, ref_dev, n_own);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if ((s = vgs_check_label_range(c, fn, seg_dev, n_own, K)) != VGS_OK) return s;
  return cmp_own_cells(c, fn, K, ref_dev, n_cells, n_unannotated, seg_dev);
}

extern "C" vgs_status vgs_own_point_label_cells(vgs_ctx* c, int64_t K, const int32_t* seg_host, const int32_t* ref_host, int64_t n_own, int64_t* n_cells,
                                                int64_t* n_unannotated) {
  if (!c) return VGS_E_ARG;
  const char* fn = "vgs_own_point_label_cells";
  vgs_status s = cmp_own_point_check(c, fn, K, seg_host, ref_host, n_own);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const int32_t* seg_dev = nullptr;
  if ((s = vgs_upload_point_labels(c, seg_host, n_own, &seg_dev)) != VGS_OK) return s;
  if ((s = vgs_check_label_range(c, fn, seg_dev, n_own, K)) != VGS_OK) return s;
  if (n_own > 0) {
    VGS_HIP_TRY(c, c->cmp_ref.ensure((size_t)n_own));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->cmp_ref.p, ref_host, (size_t)n_own * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the caller's array is free again, whatever follows
  }
  return cmp_own_cells(c, fn, K, c->cmp_ref.p, n_cells, n_unannotated, seg_dev);
}

extern "C" vgs_status vgs_get_own_label_cells(vgs_ctx* c, int32_t* cell_seg, int32_t* cell_ref, int64_t* cell_n) {
  if (!c) return VGS_E_ARG;
  if (c->cmp_own_cells < 0) {
    c->err = "vgs_get_own_label_cells: no own cells (vgs_own_label_cells first; a comparison, a run of the stages or new labels discard them)";
    return VGS_E_STATE;
  }
  const size_t nc = (size_t)c->cmp_own_cells, na = (size_t)c->cmp_ann;
  if (nc == 0) return VGS_OK;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const RowCol col[3] = {{cell_seg, c->cmp_cell_i32.p, sizeof(int32_t)}, {cell_ref, c->cmp_cell_i32.p + na, sizeof(int32_t)}, {cell_n, c->cmp_cell_n.p, sizeof(int64_t)}};
  return vgs_copy_rows(c, nc, col, 3);
}

// ------------------------------------------------------------------------------------------------ the tables from a cell list
#define CMP_TOTAL_MAX 0x100000000ull   // 2^32 points: C(total, 2) fits int64

extern "C" vgs_status vgs_label_comparison_from_cells(vgs_ctx* c, int64_t K, int64_t n_in, const int32_t* cell_seg, const int32_t* cell_ref,
                                                      const int64_t* cell_n, int64_t n_unannotated, int64_t* n_cells_out, int64_t* n_refs,
                                                      int64_t* summary) {
  if (!c) return VGS_E_ARG;
  const char* fn = "vgs_label_comparison_from_cells";
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (K < 0 || K > (int64_t)0x7fffffff) { c->err = std::string(fn) + ": K = " + std::to_string(K) + " is out of range"; return VGS_E_ARG; }
  if (n_in < 0) { c->err = std::string(fn) + ": n_in = " + std::to_string(n_in) + " is negative"; return VGS_E_ARG; }
  if (n_unannotated < 0) { c->err = std::string(fn) + ": n_unannotated = " + std::to_string(n_unannotated) + " is negative"; return VGS_E_ARG; }
  if (n_in > 0 && (!cell_seg || !cell_ref || !cell_n)) { c->err = std::string(fn) + ": an input array is NULL"; return VGS_E_ARG; }
  if (n_in >= ((int64_t)1 << 31)) {
    c->err = std::string(fn) + ": n_in = " + std::to_string(n_in) + " input cells reach the limit of 2^31 = " + std::to_string((int64_t)1 << 31);
    return VGS_E_UNSUPPORTED;
  }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  c->cmp_valid = false; c->cmp_own_cells = -1;
  c->cmp_cells = 0; c->cmp_refs = 0; c->cmp_K = K;
  for (int i = 0; i < 12; ++i) c->cmp_summary[i] = 0;
  VGS_HIP_TRY(c, c->cmp_meta.ensure(CM_SLOTS));
  cmp_u64* meta = (cmp_u64*)c->cmp_meta.p;
  VGS_HIP_TRY(c, hipMemsetAsync(meta, 0, CM_SLOTS * sizeof(uint64_t), c->stream));
  uint64_t m[CM_SLOTS] = {0};
  const uint32_t n = (uint32_t)n_in;
  uint32_t n_cells = 0;
  unsigned gbits = 1;
  if (n > 0) {
    // the input cells: seg | ref in cmp_ref; keys in, keys out, counts in, counts out in cmp_key
    VGS_HIP_TRY(c, c->cmp_ref.ensure(2 * (size_t)n)); VGS_HIP_TRY(c, c->cmp_key.ensure(4 * (size_t)n)); VGS_HIP_TRY(c, c->cmp_work.ensure(2 * (size_t)n));
    int32_t *in_seg = c->cmp_ref.p, *in_ref = in_seg + n;
    uint64_t *key_in = c->cmp_key.p, *key_out = key_in + n;
    long long *cnt_in = (long long*)(key_out + n), *cnt_out = cnt_in + n;
    uint32_t *head = c->cmp_work.p, *inc = head + n;
    VGS_HIP_TRY(c, hipMemcpyAsync(in_seg, cell_seg, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(in_ref, cell_ref, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(cnt_in, cell_n, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_cmp_cells_scan, dim3(std::min(cmp_grid(n), CMP_SCAN_GRID)), dim3(CMP_TB), 0, c->stream, in_seg, in_ref, cnt_in, n, (uint32_t)K, meta);
    VGS_HIP_TRY(c, hipGetLastError());
    VGS_READBACK(c, m, meta, CM_SLOTS * sizeof(uint64_t));   // the largest id, the sum of the counts, the first input that is not a cell
    if (m[CM_BAD] != 0) {
      const size_t i = (size_t)(n - (uint32_t)m[CM_BAD]);
      c->err = std::string(fn) + ": input cell " + std::to_string(i) + " = (seg " + std::to_string(cell_seg[i]) + ", ref " + std::to_string(cell_ref[i]) +
               ", n " + std::to_string(cell_n[i]) + "): seg must be in -1 .. K-1 = " + std::to_string(K - 1) + ", ref >= 0 and n >= 1";
      return VGS_E_ARG;
    }
    if (m[CM_TOTAL] > CMP_TOTAL_MAX) {
      c->err = std::string(fn) + ": the counts add up to " + (m[CM_TOTAL] >= CMP_COUNT_CLAMP ? std::string("at least ") : std::string()) +
               std::to_string(m[CM_TOTAL]) + " points, above the limit of 2^32 = " + std::to_string(CMP_TOTAL_MAX);
      return VGS_E_UNSUPPORTED;
    }
    gbits = cmp_bits(m[CM_MAXID]);
    const unsigned bits = gbits + cmp_bits((uint64_t)K);   // rows 0 .. K
    hipLaunchKernelGGL(k_cmp_cells_keys, dim3(cmp_grid(n)), dim3(CMP_TB), 0, c->stream, in_seg, in_ref, n, gbits, key_in);
    size_t t_sort = 0, t_scan = 0;
    VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, key_in, key_out, cnt_in, cnt_out, (size_t)n, 0, bits, c->stream));
    VGS_HIP_TRY(c, rocprim::inclusive_scan(nullptr, t_scan, head, inc, (size_t)n, rocprim::plus<uint32_t>(), c->stream));
    VGS_HIP_TRY(c, c->cmp_tmp.ensure(std::max(t_sort, t_scan)));
    VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->cmp_tmp.p, t_sort, key_in, key_out, cnt_in, cnt_out, (size_t)n, 0, bits, c->stream));
    hipLaunchKernelGGL(k_cmp_heads<uint64_t>, dim3(cmp_grid(n)), dim3(CMP_TB), 0, c->stream, key_out, n, head);
    VGS_HIP_TRY(c, rocprim::inclusive_scan(c->cmp_tmp.p, t_scan, head, inc, (size_t)n, rocprim::plus<uint32_t>(), c->stream));
    // at most one merged cell per input cell
    VGS_HIP_TRY(c, c->cmp_cstart.ensure(n)); VGS_HIP_TRY(c, c->cmp_cell_i32.ensure(2 * (size_t)n)); VGS_HIP_TRY(c, c->cmp_cell_n.ensure(n));
    int32_t *m_seg = c->cmp_cell_i32.p, *m_ref = m_seg + n;
    hipLaunchKernelGGL(k_cmp_cell_starts, dim3(cmp_grid(n)), dim3(CMP_TB), 0, c->stream, key_out, head, inc, n, gbits, c->cmp_cstart.p, m_seg, m_ref, meta);
    VGS_HIP_TRY(c, hipGetLastError());
    VGS_READBACK(c, &m[CM_NCELLS], meta + CM_NCELLS, sizeof(uint64_t));   // the number of merged cells
    n_cells = (uint32_t)m[CM_NCELLS];
    hipLaunchKernelGGL(k_cmp_cells_sums, dim3(cmp_fold_grid(cmp_grid(n_cells))), dim3(CMP_TB), 0, c->stream, c->cmp_cstart.p, n_cells, n, cnt_out,
                       (long long*)c->cmp_cell_n.p, meta);
  }
  c->cmp_ann = n;   // (the stride of cell_seg | cell_ref)
  vgs_status s = cmp_cell_tables(c, K, n, n_cells, gbits, (int64_t)m[CM_TOTAL], n_unannotated, meta, m);
  if (s != VGS_OK) return s;
  cmp_report(c, n_cells_out, n_refs, summary);
  return VGS_OK;
}

// pointers into the tables of the last compare (rows: cmp_cells, cmp_refs, cmp_K)
struct CmpTables {
  const int32_t *cell_seg, *cell_ref; const int64_t* cell_n;
  const int32_t* ref_id; const int64_t *ref_points, *ref_dropped; const int32_t* ref_best_seg; const int64_t* ref_best_n; const double* ref_best_iou;
  const int64_t* seg_annotated; const int32_t *seg_refs, *seg_best_ref; const int64_t* seg_best_n; const double* seg_best_iou;
};

static vgs_status cmp_tables(vgs_ctx* c, const char* fn, CmpTables& t) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (!c->cmp_valid) { c->err = std::string(fn) + ": no comparison since the last run of the stages (vgs_compare_labels first)"; return VGS_E_STATE; }
  const size_t na = (size_t)c->cmp_ann, nc = (size_t)c->cmp_cells, k1 = c->cmp_K > 0 ? (size_t)c->cmp_K : 1;
  memset(&t, 0, sizeof(t));
  if (nc > 0) {
    t.cell_seg = c->cmp_cell_i32.p; t.cell_ref = c->cmp_cell_i32.p + na; t.cell_n = c->cmp_cell_n.p;
    t.ref_id = c->cmp_ref_i32.p; t.ref_best_seg = c->cmp_ref_i32.p + nc;
    t.ref_points = c->cmp_ref_i64.p; t.ref_dropped = c->cmp_ref_i64.p + nc; t.ref_best_n = c->cmp_ref_i64.p + 2 * nc;
    t.ref_best_iou = c->cmp_ref_iou.p;
  }
  if (c->cmp_K > 0) {
    t.seg_annotated = c->cmp_seg_i64.p; t.seg_best_n = c->cmp_seg_i64.p + k1;
    t.seg_refs = c->cmp_seg_i32.p; t.seg_best_ref = c->cmp_seg_i32.p + k1;
    t.seg_best_iou = c->cmp_seg_iou.p;
  }
  return VGS_OK;
}

extern "C" vgs_status vgs_get_label_comparison_device(vgs_ctx* c, const int32_t** cell_seg, const int32_t** cell_ref, const int64_t** cell_n,
                                                      const int32_t** ref_id, const int64_t** ref_points, const int64_t** ref_dropped,
                                                      const int32_t** ref_best_seg, const int64_t** ref_best_n, const double** ref_best_iou,
                                                      const int64_t** seg_annotated, const int32_t** seg_refs, const int32_t** seg_best_ref,
                                                      const int64_t** seg_best_n, const double** seg_best_iou) {
  if (!c) return VGS_E_ARG;
  CmpTables t;
  vgs_status s = cmp_tables(c, "vgs_get_label_comparison_device", t);
  if (s != VGS_OK) return s;
  if (cell_seg) *cell_seg = t.cell_seg;
  if (cell_ref) *cell_ref = t.cell_ref;
  if (cell_n) *cell_n = t.cell_n;
  if (ref_id) *ref_id = t.ref_id;
  if (ref_points) *ref_points = t.ref_points;
  if (ref_dropped) *ref_dropped = t.ref_dropped;
  if (ref_best_seg) *ref_best_seg = t.ref_best_seg;
  if (ref_best_n) *ref_best_n = t.ref_best_n;
  if (ref_best_iou) *ref_best_iou = t.ref_best_iou;
  if (seg_annotated) *seg_annotated = t.seg_annotated;
  if (seg_refs) *seg_refs = t.seg_refs;
  if (seg_best_ref) *seg_best_ref = t.seg_best_ref;
  if (seg_best_n) *seg_best_n = t.seg_best_n;
  if (seg_best_iou) *seg_best_iou = t.seg_best_iou;
  return VGS_OK;
}

extern "C" vgs_status vgs_get_label_comparison(vgs_ctx* c, int32_t* cell_seg, int32_t* cell_ref, int64_t* cell_n, int32_t* ref_id, int64_t* ref_points,
                                               int64_t* ref_dropped, int32_t* ref_best_seg, int64_t* ref_best_n, double* ref_best_iou,
                                               int64_t* seg_annotated, int32_t* seg_refs, int32_t* seg_best_ref, int64_t* seg_best_n,
                                               double* seg_best_iou) {
  if (!c) return VGS_E_ARG;
  CmpTables t;
  vgs_status s = cmp_tables(c, "vgs_get_label_comparison", t);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const size_t nc = (size_t)c->cmp_cells, G = (size_t)c->cmp_refs, K = (size_t)c->cmp_K;
#define CMP_COPY(dst, src, rows) \
  if ((dst) && (rows) > 0) VGS_HIP_TRY(c, hipMemcpyAsync((dst), (src), (rows) * sizeof(*(dst)), hipMemcpyDeviceToHost, c->stream))
  CMP_COPY(cell_seg, t.cell_seg, nc); CMP_COPY(cell_ref, t.cell_ref, nc); CMP_COPY(cell_n, t.cell_n, nc);
  CMP_COPY(ref_id, t.ref_id, G); CMP_COPY(ref_points, t.ref_points, G); CMP_COPY(ref_dropped, t.ref_dropped, G);
  CMP_COPY(ref_best_seg, t.ref_best_seg, G); CMP_COPY(ref_best_n, t.ref_best_n, G); CMP_COPY(ref_best_iou, t.ref_best_iou, G);
  CMP_COPY(seg_annotated, t.seg_annotated, K); CMP_COPY(seg_refs, t.seg_refs, K); CMP_COPY(seg_best_ref, t.seg_best_ref, K);
  CMP_COPY(seg_best_n, t.seg_best_n, K); CMP_COPY(seg_best_iou, t.seg_best_iou, K);
#undef CMP_COPY
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGS_OK;
}
