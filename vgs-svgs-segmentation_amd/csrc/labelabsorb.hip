// labelabsorb.hip -- absorb the stranded and the small connected parts of a per-POINT labelling that the CALLER supplies into the
// neighbour they touch most (include/vgs.h: vgs_absorb_point_label_parts; no reference counterpart).  labelcc.hip says which parts a
// labelling has and labelgraph.hip which of them touch; this pass acts on both and returns a labelling.
//
// Definition (include/vgs.h states it in full).  EVALUATION of a labelling L: the parts of L (labelcc.hip: C parts, P = part of every
// point), the graph of the parts (labelgraph.hip over P with K = C: parts of one label never touch, so every edge joins two labels).
// threshold(p) = min_points for the largest part of its label, max(min_points, island_points) for every other; p is a CANDIDATE when
// part_points[p] < threshold(p), STABLE otherwise.  The TARGET of a candidate is its stable neighbour q with the largest triple
// (n_shared + n_pairs, part_points[q], -q).  ROUNDS: evaluate; stop at round max_rounds or when no candidate has a target; otherwise all
// points of every candidate with a target take the target's label and the next round evaluates the new labelling.
//
// Data flow of one evaluation, behind the two existing passes and on their device tables:
//   1. k_la_candidates  one thread per part: threshold, candidate flag; the candidates and their points are counted (wave-reduced
//                       integer adds).  Read-back: no candidate, or the round is the cap -> this evaluation is the final one, and the graph
//                       of the parts is not needed and not built.
//   2. k_la_records     the 2E directed records (p, q, score) of the E edges, of which those with p a candidate and q stable are kept:
//                       the two directions of one edge cannot both qualify, so an edge gives at most ONE kept record and the record is
//                       the edge itself -- key = its candidate endpoint, or C for an edge that gives none, value = the edge.  One stable
//                       radix sort by key brings them into runs by p (the C-keys form the tail); k_la_runs marks every run.
//   3. k_la_targets     one wavefront per part; a candidate's wavefront folds its run to the lexicographic maximum: lane stride over the
//                       run, then the xor butterfly of wavefold.hpp's shape on the triple.  The order (score, points, -q) is total on a
//                       run (its q are distinct), so the maximum does not depend on who meets whom first; no atomic takes part in it.
//                       Lane 0 writes target[p] (-1: none) and counts the absorbed part.  Read-back: no target -> final evaluation.
//   4. k_la_apply       one thread per point: out[i] = part_label[target[P[i]]] where there is a target, else in[i]; the relabelled points
//                       are counted (ballot, one add per wavefront).
// Behind the final evaluation k_la_finish writes labels_out: the current labelling, with -1 for every point of a candidate when drop is
// set (counted the same way).
// Determinism: every decision is a function of integer tables that are themselves functions of the labelling; the counters are integer
// sums.  Bit-identical from call to call and engine to engine.
// Buffers: la_out (the result, N words) and la_alt (the second labelling of the rounds, N words) belong to the context; the caller's
// labelling is only read.  Rounds alternate between the two; the final pass writes la_out in place when the last round ended there.
// Scratch: 1 B + 4 B + 8 B per part (flag, target, run), 16 B per edge (keys and values, in and out) and rocprim's storage, four 64-bit
// counter words.  The two inner passes' results are overwritten every round: lcc_valid and lg_valid are false afterwards.
#include <climits>
#include <string.h>

#include <algorithm>
#include <string>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "wavefold.hpp"

#define LA_TB 256
#define LA_WAVES 4   // wavefronts (parts) per workgroup of k_la_targets
// counter words (la_cnt)
enum { LA_N_CAND = 0, LA_CAND_POINTS = 1, LA_N_TARGETS = 2, LA_POINTS = 3, LA_N_WORDS = 4 };

__device__ __forceinline__ unsigned long long la_wave_sum(unsigned long long x) { return (unsigned long long)sg_wave_sum((long long)x); }

// Step 1.  One thread per part; whole wavefronts reach the fold (no early return in front of it).
__global__ __launch_bounds__(LA_TB) void k_la_candidates(const int32_t* __restrict__ p_label, const int64_t* __restrict__ p_points,
                                                         const int32_t* __restrict__ l_largest, uint32_t C, uint32_t K, int64_t min_points,
                                                         int64_t island_points, uint8_t* __restrict__ cand, unsigned long long* __restrict__ cnt) {
  const uint64_t p = (uint64_t)blockIdx.x * LA_TB + threadIdx.x;
  unsigned long long one = 0, pts = 0;
  if (p < (uint64_t)C) {
    const uint32_t l = (uint32_t)p_label[p];
    const bool largest = l < K && l_largest[l] == (int32_t)p;
    const int64_t thr = (largest || island_points < min_points) ? min_points : island_points;
    const int64_t n = p_points[p];
    const bool is = n < thr;
    cand[p] = is ? 1 : 0;
    if (is) { one = 1; pts = (unsigned long long)n; }
  }
  one = la_wave_sum(one); pts = la_wave_sum(pts);
  if ((threadIdx.x & 63) == 0 && one) { atomicAdd(&cnt[LA_N_CAND], one); atomicAdd(&cnt[LA_CAND_POINTS], pts); }
}

// Step 2.  One thread per edge {a < b} of the graph of the parts: the candidate endpoint that has the other, stable, as a possible target
__global__ __launch_bounds__(LA_TB) void k_la_records(const int32_t* __restrict__ ab, const uint8_t* __restrict__ cand, uint32_t E, uint32_t C,
                                                      uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t e = blockIdx.x * LA_TB + threadIdx.x;
  if (e >= E) return;
  const uint32_t a = (uint32_t)ab[2 * (size_t)e], b = (uint32_t)ab[2 * (size_t)e + 1];
  uint32_t k = C;
  if (a < C && b < C) {   // (the table's own ids: the bound only guards the flags)
    const bool ca = cand[a] != 0, cb = cand[b] != 0;
    if (ca != cb) k = ca ? a : b;
  }
  key[e] = k;
  val[e] = e;
}
// behind the sort: the run of every part that has records (rbeg = rend = 0, the fill, for every other)
__global__ __launch_bounds__(LA_TB) void k_la_runs(const uint32_t* __restrict__ skey, uint32_t E, uint32_t C, uint32_t* __restrict__ rbeg,
                                                   uint32_t* __restrict__ rend) {
  const uint32_t i = blockIdx.x * LA_TB + threadIdx.x;
  if (i >= E) return;
  const uint32_t p = skey[i];
  if (p >= C) return;
  if (i == 0 || skey[i - 1] != p) rbeg[p] = i;
  if (i + 1 == E || skey[i + 1] != p) rend[p] = i + 1;
}

// most boundary, then the bigger part, then the lower part id
__device__ __forceinline__ bool la_better(long long s, long long n, int q, long long bs, long long bn, int bq) {
  return s > bs || (s == bs && (n > bn || (n == bn && q < bq)));
}

// Step 3.  One wavefront per part.
__global__ __launch_bounds__(64 * LA_WAVES) void k_la_targets(const uint32_t* __restrict__ sval, const uint32_t* __restrict__ rbeg,
                                                              const uint32_t* __restrict__ rend, const uint8_t* __restrict__ cand,
                                                              const int32_t* __restrict__ ab, const int64_t* __restrict__ n_shared,
                                                              const int64_t* __restrict__ n_pairs, const int64_t* __restrict__ p_points, uint32_t C,
                                                              uint32_t E, int32_t* __restrict__ target, unsigned long long* __restrict__ cnt) {
  const uint32_t p = blockIdx.x * LA_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= C) return;   // (whole wavefronts; no barrier follows)
  const uint32_t a = rbeg[p], b = min(rend[p], E);
  if (!cand[p] || a >= b) { if (lane == 0) target[p] = -1; return; }
  long long bs = -1, bn = -1;   // (a record's score is at least 1: a lane without a record loses every comparison)
  int bq = INT_MAX;
  for (uint32_t i = a + lane; i < b; i += 64) {
    const uint32_t e = min(sval[i], E - 1);   // (the sort's own values: the bound only guards the table)
    const int ea = ab[2 * (size_t)e], eb = ab[2 * (size_t)e + 1];
    const int q = ea == (int)p ? eb : ea;
    const long long s = n_shared[e] + n_pairs[e];
    const long long n = (uint32_t)q < C ? p_points[q] : -1;
    if (la_better(s, n, q, bs, bn, bq)) { bs = s; bn = n; bq = q; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const long long os = __shfl_xor(bs, m, 64), on = __shfl_xor(bn, m, 64);
    const int oq = __shfl_xor(bq, m, 64);
    if (la_better(os, on, oq, bs, bn, bq)) { bs = os; bn = on; bq = oq; }
  }
  if (lane != 0) return;
  const bool found = bs > 0 && (uint32_t)bq < C;
  target[p] = found ? bq : -1;
  if (found) atomicAdd(&cnt[LA_N_TARGETS], 1ull);
}

// Step 4.  One thread per point.  in and out are different buffers
__global__ __launch_bounds__(LA_TB) void k_la_apply(const int32_t* __restrict__ in, const int32_t* __restrict__ part_of_point,
                                                    const int32_t* __restrict__ target, const int32_t* __restrict__ p_label, int64_t N, uint32_t C,
                                                    int32_t* __restrict__ out, unsigned long long* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * LA_TB + threadIdx.x;
  bool moved = false;
  if (i < N) {
    int32_t l = in[i];
    const int32_t p = part_of_point[i];
    if (p >= 0 && (uint32_t)p < C) {
      const int32_t t = target[p];
      if (t >= 0 && (uint32_t)t < C) { l = p_label[t]; moved = true; }
    }
    out[i] = l;
  }
  const unsigned long long m = __ballot(moved);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[LA_POINTS], (unsigned long long)__popcll(m));
}

// Behind the final evaluation: labels_out = the current labelling, -1 for the points of its candidates when drop is set.  in may be out
// (a thread reads and writes its own word only), hence no __restrict__ on the two.
__global__ __launch_bounds__(LA_TB) void k_la_finish(const int32_t* in, const int32_t* __restrict__ part_of_point, const uint8_t* __restrict__ cand,
                                                     int64_t N, uint32_t C, int drop, int32_t* out, unsigned long long* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * LA_TB + threadIdx.x;
  bool gone = false;
  if (i < N) {
    int32_t l = in[i];
    if (drop) {
      const int32_t p = part_of_point[i];
      if (p >= 0 && (uint32_t)p < C && cand[p]) { l = -1; gone = true; }
    }
    out[i] = l;
  }
  const unsigned long long m = __ballot(gone);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[LA_POINTS], (unsigned long long)__popcll(m));
}

// ---------------------------------------------------------------------------------------------------------------------- host
static unsigned la_grid(uint64_t n) { return (unsigned)((n + LA_TB - 1) / LA_TB); }

static vgs_status la_check(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t n, int64_t K, const vgs_absorb_params* ap) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of the cloud and of its neighbourhood graph; absorbing the parts of a labelling across the ranks of the tiled driver does not exist yet";
    return VGS_E_STATE;
  }
  if (n != c->N) {
    c->err = std::string(fn) + ": n = " + std::to_string(n) + " must equal the number of points of the cloud, " + std::to_string(c->N);
    return VGS_E_ARG;
  }
  if (!labels && n > 0) { c->err = std::string(fn) + ": labels is NULL"; return VGS_E_ARG; }
  if (!ap) { c->err = std::string(fn) + ": params is NULL"; return VGS_E_ARG; }
  if (K < 0 || K > (int64_t)0x7fffffff) { c->err = std::string(fn) + ": K = " + std::to_string(K) + " is out of range"; return VGS_E_ARG; }
  if (ap->min_points < 0) { c->err = std::string(fn) + ": min_points = " + std::to_string(ap->min_points) + " is negative"; return VGS_E_ARG; }
  if (ap->island_points < 0) { c->err = std::string(fn) + ": island_points = " + std::to_string(ap->island_points) + " is negative"; return VGS_E_ARG; }
  if (ap->max_rounds < 0 || ap->max_rounds > 64) {
    c->err = std::string(fn) + ": max_rounds = " + std::to_string(ap->max_rounds) + " is outside 0 .. 64";
    return VGS_E_ARG;
  }
  return VGS_OK;
}

// the targets of the candidates of the evaluation in lcc_* (C parts): the graph of the parts, steps 2 and 3.  n_targets: how many have one
static vgs_status la_targets(vgs_ctx* c, uint32_t C, uint64_t* n_targets) {
  *n_targets = 0;
  int64_t E64 = 0;
  vgs_status s = vgs_point_label_graph_device(c, c->lcc_pop.p, c->N, (int64_t)C, &E64, nullptr);
  if (s != VGS_OK) return s;
  if (E64 <= 0) return VGS_OK;
  const uint32_t E = (uint32_t)E64;   // (labelgraph.hip keeps E below 2^31)
  VGS_HIP_TRY(c, c->la_key.ensure(2 * (size_t)E)); VGS_HIP_TRY(c, c->la_val.ensure(2 * (size_t)E)); VGS_HIP_TRY(c, c->la_run.ensure(2 * (size_t)C));
  VGS_HIP_TRY(c, c->la_target.ensure(C));
  uint32_t *key = c->la_key.p, *skey = key + E, *val = c->la_val.p, *sval = val + E, *rbeg = c->la_run.p, *rend = rbeg + C;
  unsigned bits = 1;
  while (bits < 32 && (1ull << bits) < (unsigned long long)C + 1) ++bits;   // keys 0 .. C
  size_t t_sort = 0;
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, key, skey, val, sval, (size_t)E, 0, bits, c->stream));
  VGS_HIP_TRY(c, c->la_tmp.ensure(t_sort));
  hipLaunchKernelGGL(k_la_records, dim3(la_grid(E)), dim3(LA_TB), 0, c->stream, c->lg_ab.p, c->la_cand.p, E, C, key, val);
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->la_tmp.p, t_sort, key, skey, val, sval, (size_t)E, 0, bits, c->stream));
  VGS_HIP_TRY(c, hipMemsetAsync(rbeg, 0, 2 * (size_t)C * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_la_runs, dim3(la_grid(E)), dim3(LA_TB), 0, c->stream, skey, E, C, rbeg, rend);
  hipLaunchKernelGGL(k_la_targets, dim3((C + LA_WAVES - 1) / LA_WAVES), dim3(64 * LA_WAVES), 0, c->stream, sval, rbeg, rend, c->la_cand.p, c->lg_ab.p,
                     c->lg_nshared.p, c->lg_npairs.p, c->lcc_ppoints.p, C, E, c->la_target.p, (unsigned long long*)c->la_cnt.p);
  VGS_HIP_TRY(c, hipGetLastError());
  VGS_READBACK(c, n_targets, c->la_cnt.p + LA_N_TARGETS, 8);   // read-back: the candidates that have a target
  return VGS_OK;
}

static vgs_status la_rounds(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, const vgs_absorb_params& ap, int64_t* counts8) {
  const int64_t N = c->N;
  VGS_HIP_TRY(c, c->la_out.ensure(N > 0 ? (size_t)N : 1)); VGS_HIP_TRY(c, c->la_alt.ensure(N > 0 ? (size_t)N : 1));
  VGS_HIP_TRY(c, c->la_cnt.ensure(LA_N_WORDS));
  unsigned long long* cnt = (unsigned long long*)c->la_cnt.p;
  VGS_HIP_TRY(c, hipMemsetAsync(cnt, 0, LA_N_WORDS * sizeof(uint64_t), c->stream));
  const int32_t* cur = labels_dev;
  int64_t rounds = 0, absorbed = 0, C64 = 0, n_skipped = 0;
  uint64_t w[LA_N_WORDS] = {0, 0, 0, 0};
  uint32_t C = 0;
  vgs_status s;
  for (int r = 0;; ++r) {
    // the evaluation of cur
    if ((s = vgs_label_parts_on_device(c, fn, cur, 0, N, K, &C64, &n_skipped)) != VGS_OK) return s;
    C = (uint32_t)C64;
    w[LA_N_CAND] = w[LA_CAND_POINTS] = 0;
    if (C > 0 && (ap.min_points > 0 || ap.island_points > 0)) {
      VGS_HIP_TRY(c, c->la_cand.ensure(C));
      VGS_HIP_TRY(c, hipMemsetAsync(cnt, 0, 3 * sizeof(uint64_t), c->stream));   // (the points relabelled add up over the rounds)
      hipLaunchKernelGGL(k_la_candidates, dim3(la_grid(C)), dim3(LA_TB), 0, c->stream, c->lcc_plabel.p, c->lcc_ppoints.p, c->lcc_llargest.p, C, (uint32_t)K,
                         ap.min_points, ap.island_points, c->la_cand.p, cnt);
      VGS_HIP_TRY(c, hipGetLastError());
      VGS_READBACK(c, w, cnt, 2 * sizeof(uint64_t));   // read-back: the candidates and their points
    }
    if (w[LA_N_CAND] == 0 || r == ap.max_rounds) break;
    uint64_t n_targets = 0;
    if ((s = la_targets(c, C, &n_targets)) != VGS_OK) return s;
    if (n_targets == 0) break;
    int32_t* next = cur == c->la_out.p ? c->la_alt.p : c->la_out.p;
    hipLaunchKernelGGL(k_la_apply, dim3(la_grid((uint64_t)N)), dim3(LA_TB), 0, c->stream, cur, c->lcc_pop.p, c->la_target.p, c->lcc_plabel.p, N, C, next, cnt);
    VGS_HIP_TRY(c, hipGetLastError());
    cur = next;
    ++rounds;
    absorbed += (int64_t)n_targets;
  }
  uint64_t moved = 0, dropped = 0;
  VGS_READBACK(c, &moved, cnt + LA_POINTS, 8);
  const bool drop = ap.drop != 0 && w[LA_N_CAND] > 0;
  if (N > 0 && (drop || cur != c->la_out.p)) {
    VGS_HIP_TRY(c, hipMemsetAsync(cnt + LA_POINTS, 0, sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_la_finish, dim3(la_grid((uint64_t)N)), dim3(LA_TB), 0, c->stream, cur, c->lcc_pop.p, c->la_cand.p, N, C, drop ? 1 : 0, c->la_out.p, cnt);
    VGS_HIP_TRY(c, hipGetLastError());
    VGS_READBACK(c, &dropped, cnt + LA_POINTS, 8);   // (waits for the stream: a labelling read in place is the caller's again)
  }
  counts8[0] = rounds; counts8[1] = absorbed; counts8[2] = (int64_t)moved; counts8[3] = (int64_t)w[LA_N_CAND]; counts8[4] = (int64_t)w[LA_CAND_POINTS];
  counts8[5] = (int64_t)dropped; counts8[6] = C64; counts8[7] = n_skipped;
  return VGS_OK;
}

static vgs_status la_absorb(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t n, int64_t K, const vgs_absorb_params* ap,
                            int64_t* counts) {
  if (!c) return VGS_E_ARG;
  if (counts) memset(counts, 0, 8 * sizeof(int64_t));
  vgs_status s = la_check(c, fn, labels, n, K, ap);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  c->la_valid = false;
  int64_t counts8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (on_device || (s = vgs_upload_point_labels(c, labels, n, &labels)) == VGS_OK) s = la_rounds(c, fn, labels, K, *ap, counts8);
  c->lcc_valid = false; c->lg_valid = false;   // the rounds overwrote both results
  if (s != VGS_OK) return s;
  c->la_valid = true;
  if (counts) memcpy(counts, counts8, sizeof(counts8));
  return VGS_OK;
}

extern "C" vgs_status vgs_absorb_params_default(vgs_absorb_params* ap) {
  if (!ap) return VGS_E_ARG;
  ap->min_points = 0; ap->island_points = 0; ap->max_rounds = 8; ap->drop = 0;
  return VGS_OK;
}

extern "C" vgs_status vgs_absorb_point_label_parts(vgs_ctx* c, const int32_t* labels_host, int64_t n, int64_t K, const vgs_absorb_params* ap,
                                                   int64_t* counts) {
  return la_absorb(c, "vgs_absorb_point_label_parts", labels_host, false, n, K, ap, counts);
}

extern "C" vgs_status vgs_absorb_point_label_parts_device(vgs_ctx* c, const int32_t* labels_dev, int64_t n, int64_t K, const vgs_absorb_params* ap,
                                                          int64_t* counts) {
  return la_absorb(c, "vgs_absorb_point_label_parts_device", labels_dev, true, n, K, ap, counts);
}

static vgs_status la_result(vgs_ctx* c, const char* fn) {
  if (!c) return VGS_E_ARG;
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context holds only part of the cloud; absorbing the parts of a labelling across the ranks of the tiled driver does not exist yet";
    return VGS_E_STATE;
  }
  if (c->stage < ST_SEGMENTED || !c->la_valid) {
    c->err = std::string(fn) + ": no absorbed labels since the last run of the stages (vgs_absorb_point_label_parts first)";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

extern "C" vgs_status vgs_get_absorbed_point_labels(vgs_ctx* c, int32_t* out) {
  vgs_status s = la_result(c, "vgs_get_absorbed_point_labels");
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (out && c->N > 0) VGS_HIP_TRY(c, hipMemcpy(out, c->la_out.p, (size_t)c->N * sizeof(int32_t), hipMemcpyDeviceToHost));
  return VGS_OK;
}

extern "C" vgs_status vgs_get_absorbed_point_labels_device(vgs_ctx* c, const int32_t** out) {
  if (out) *out = nullptr;
  vgs_status s = la_result(c, "vgs_get_absorbed_point_labels_device");
  if (s != VGS_OK) return s;
  if (out) *out = c->N > 0 ? c->la_out.p : nullptr;
  return VGS_OK;
}
