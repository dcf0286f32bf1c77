// merge.hip -- stages a8-a11: mutual-connection filter, isolated-voxel re-attachment, connected
// components, cluster size filter and per-point labels.
// Replaces crossValidation (voxel_segmentation.h:2111-2179), closestCheck (VS:2181-2303),
// clusteringVoxels + recursionSearch (VS:2032-2099) and the cluster filter / point lists of
// drawColorMapofPointsinClusters (VS:963-1009); SVGS twins SS:2142-2305, 2057-2130.
//
// The reference's sequential control flow becomes data-parallel:
//   * crossValidation is the symmetric intersection of the connect lists, one lane per
//     adjacency slot, the reverse slot found by binary search on the (d2, id) sort key (d2 is symmetric);
//   * closestCheck mutates lists while scanning voxels in order; its only order dependence is that a
//     re-attached voxel becomes an eligible target for LATER voxels.  "re-attachment succeeds" is therefore a
//     monotone fixed point over ascending ids, iterated in parallel; each voxel then picks its target among
//     the voxels eligible at its turn (ties: last in scan order, `>=` at VS:2281);
//   * the recursive DFS becomes a lock-free union-find (hook larger root under smaller) over the mutual and
//     re-attachment edges; the root of a component is its smallest voxel id, which is also the order in
//     which the reference discovers clusters (VS:2064).
#include <cstring>
#include <string.h>
#include <utility>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "unionfind.hpp"

struct MgParams {
  VgsWeightParams W;
  int adjacency_min;
  int q7;
  int64_t V;
};

// The merge front (k_cross, k_union_mutual) compacts a row before it looks anything up.  A row holds about 120 used neighbours, of
// which about a fifth carry a connect flag and a tenth a mutual flag with t > i; only those enter the chain of dependent loads
// (key -> used_rank -> connect-bit words / parent), and both kernels wait on loads, not on HBM's bandwidth.  So each row group first
// reads its flags (coalesced, independent loads, several trips issued together), appends the positions of the set ones to a list
// in LDS, and then walks the list with every lane carrying a load of the chain.  A list holds MF_CAP_TRIPS * W 16-bit positions per row
// group (adj_stride reaches 8192); a row with more set entries is taken in rounds: fill, drain, go on behind the last trip taken.
#define MF_CAP_TRIPS 8   // list capacity in trips of W entries: 8 * W * CX_ROWS (or UM_ROWS) * 2 bytes = 1 KB per workgroup
// one batch of the flag pass, in two halves.  mf_load: T trips of W flags from position k0 -- unconditional loads (a position at or
// beyond `limit` reads position 0, which every row has), so one wait covers all T and whatever else was issued beside them.
template <int W, int T>
__device__ __forceinline__ void mf_load(const uint8_t* __restrict__ flags, int limit, int k0, int sub, uint8_t (&f)[T]) {
#pragma unroll
  for (int q = 0; q < T; ++q) {
    const int k = k0 + q * W + sub;
    f[q] = flags[k < limit ? k : 0];
  }
}
// mf_append: the positions below n whose flag is set go to `list` at `cnt`, in ascending order (`mine`: the lanes of this row group;
// ballots of a wavefront whose groups have diverged carry zeros for the other group).  `zero`, when given, gets a 0 at every unset
// position (the mutual flags of entries that are not connected).
template <int W, int T>
__device__ __forceinline__ void mf_append(const uint8_t (&f)[T], uint8_t* __restrict__ zero, int n, int k0, int sub,
                                          unsigned long long mine, uint16_t* list, int& cnt) {
#pragma unroll
  for (int q = 0; q < T; ++q) {
    const int k = k0 + q * W + sub;
    const bool in = k < n, set = in && f[q] != 0;
    const unsigned long long mk = __ballot(set) & mine;
    if (set) list[cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u))] = (uint16_t)k;   // set lanes below this one
    else if (in && zero) zero[k] = 0;
    cnt += __popcll(mk);
  }
}
// LDS traffic inside one wavefront: earlier LDS writes of all lanes are visible and the compiler moves nothing across (the
// lanes run in lockstep and a row group reads only what its own lanes wrote, so no s_barrier is needed)
__device__ __forceinline__ void mf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------ crossValidation
// CX_ROWS rows per wavefront, 64 / CX_ROWS lanes each.  With the row compacted, the lanes of a group are what one trip of the
// dense pass keeps in flight: 32 lanes take the connected entries of most rows (median 23, 95 % <= 56) in one or two trips.
#ifndef CX_ROWS
#define CX_ROWS 2
#endif
// (eight wavefronts per SIMD asked for by name: the kernel's many arguments sit near the 96 scalar registers that allows)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void k_cross(const uint32_t* __restrict__ used_ids, const uint32_t* __restrict__ used_rank, int64_t U,
                                              const uint64_t* __restrict__ adj_key, const uint32_t* __restrict__ adj_cnt,
                                              int adj_stride, const uint8_t* __restrict__ conn, uint8_t* __restrict__ mutual,
                                              uint32_t* __restrict__ csize, uint32_t* __restrict__ parent,
                                              const uint16_t* __restrict__ gtab, int gstride, const uint8_t* __restrict__ nrank, float inv_res2,
                                              const uint8_t* __restrict__ pending, uint32_t* __restrict__ defer_list,
                                              unsigned int* __restrict__ n_defer, const uint32_t* __restrict__ work, int n_work,
                                              const uint16_t* __restrict__ adj_off, int cb_R,
                                              const uint32_t* __restrict__ cbits, int cb_words, uint8_t* __restrict__ defer_flag, LcGate gate,
                                              const uint8_t* __restrict__ owned = nullptr) {
  if (!lc_gate_open_early(gate)) return;
  // First pass (pending != null): all rows, while the hand-over kernels of the local cut still run -- a row whose voxel, or
  // one of whose connected neighbours, is handed over is put off (its flags or theirs are not final).  Second pass
  // (work != null): the rows put off.
  constexpr int W = 64 / CX_ROWS;
  const int lane = threadIdx.x, grp = lane / W, sub = lane % W;
  // rows of the voxel lattice carry a table of where each group of equal offset length starts: the reverse entry has
  // the same length, so only that group (a handful of entries) is searched instead of the whole row
  __shared__ uint32_t s_rank4[64];   // length -> group index (256 bytes)
  __shared__ uint16_t s_list[CX_ROWS][MF_CAP_TRIPS * W];
  constexpr int T = 4, CAP = MF_CAP_TRIPS * W;
  const uint32_t rank4 = gtab ? ((const uint32_t*)nrank)[lane] : 0u;
  int64_t u;
  bool live;
  if (work) {
    const int w = (int)blockIdx.x * CX_ROWS + grp;
    live = w < n_work;
    u = live ? (int64_t)work[w] : 0;
  } else {
    const int64_t ngroups = (U + CX_ROWS - 1) / CX_ROWS;
    const int64_t g = vgs_xcd_item(blockIdx.x, ngroups);   // consecutive rows share a wavefront, consecutive groups an XCD
    u = g * CX_ROWS + grp;
    live = g < ngroups && u < U;
    if (!live) u = 0;
  }
  // The head of the row's chain in one wait: its put-off flag, id and length, and the first batch of connect flags -- read without
  // knowing the length (the row's allocation, adj_stride, bounds the loads; what lies behind the length is not looked at).  Lanes
  // without a row read row 0 and leave below, behind the table's barrier.
  const uint64_t* row = adj_key + u * adj_stride;
  const uint8_t* crow = conn + u * adj_stride;
  uint8_t* mrow = mutual + u * adj_stride;
  const uint8_t put_off = pending ? pending[u] : (uint8_t)0;
  const uint32_t i = used_ids[u];
  const int n = (int)adj_cnt[u];
  uint8_t f[T];
  mf_load<W, T>(crow, adj_stride, 0, sub, f);
  if (gtab) s_rank4[lane] = rank4;
  __syncthreads();
  const uint8_t* s_rank = (const uint8_t*)s_rank4;
  if (!live) return;
  if (put_off) { if (sub == 0) { defer_list[atomicAdd(n_defer, 1u)] = (uint32_t)u; if (defer_flag) defer_flag[u] = 1; } return; }
  bool touches_pending = false;
  uint16_t* list = s_list[grp];
  const unsigned long long mine = (W == 64) ? ~0ull : (((1ull << W) - 1ull) << (grp * W));
  const bool own_tab = gtab && gtab[u * gstride] != 0xffffu;
  // lattice lookup (round 4): the neighbour t sits at ball offset o from i, so "i in L0(t)" is the bit of the NEGATED offset in t's row
  // of connect bits -- two dependent loads (t's row index, the word) instead of the chain rank -> group table -> binary search over
  // 8-byte keys -> flag.  A row without lattice offsets (its own, or t's: bit 0 clear) takes the search below.
  const uint16_t* orow = (cbits != nullptr && adj_off != nullptr) ? adj_off + u * adj_stride : nullptr;
  const bool own_bits = orow != nullptr && orow[0] != 0xffffu;
  int kept = 0;
  // first hook of the union-find (ECL-CC style): every used voxel points at its smallest trusted mutual neighbour below it.  Ids only
  // decrease along parent links, so this is a forest; it already joins most of every large segment without atomics.
  uint32_t best = i;
  // a list of length <= 1 is left alone (VS:2120): it is {self}.  Only a row whose flag pass ended in the first round can be that short.
  bool single = false;
  for (int k0 = 0, round = 0; k0 < n; ++round) {
    // flag pass: the positions of the set entries, as many trips as the list is sure to hold
    int cnt = 0;
    for (; k0 < n && cnt + T * W <= CAP; k0 += T * W) {
      if (k0 > 0) mf_load<W, T>(crow, n, k0, sub, f);
      mf_append<W, T>(f, mrow, n, k0, sub, mine, list, cnt);
    }
    if (round == 0) single = k0 >= n && cnt <= 1;
    mf_wave_sync();
    // dense pass: every lane carries a connected entry
    for (int j = sub; j < cnt; j += W) {
      const int k = (int)list[j];
      uint8_t mflag = 0;
      const uint64_t key = row[k];
      const uint32_t t = (uint32_t)key;
      if (single || t == i) {
        mflag = 1;
      } else {
        const uint32_t ut = used_rank[t];
        bool by_bits = false;
        if (ut != 0xffffffffu && own_bits) {
          const int D = 2 * cb_R + 1;
          const uint32_t centre = (uint32_t)((cb_R * D + cb_R) * D + cb_R);
          const uint32_t idx = (uint32_t)(D * D * D - 1) - vgs_cb_index(orow[k], cb_R);   // the negated offset: point symmetry of the cube
          const uint32_t* trow_bits = cbits + (size_t)ut * (size_t)cb_words;
          const uint32_t wc = trow_bits[centre >> 5];
          if ((wc >> (centre & 31u)) & 1u) {   // t's row has bits (its own voxel is always a member)
            by_bits = true;
            if (pending && pending[ut]) touches_pending = true;
            const uint32_t wd = (idx >> 5) == (centre >> 5) ? wc : trow_bits[idx >> 5];
            mflag = (uint8_t)((wd >> (idx & 31u)) & 1u);
          }
        }
        if (ut != 0xffffffffu && !by_bits) {
          if (pending && pending[ut]) touches_pending = true;
          const uint64_t want = (key & 0xffffffff00000000ull) | (uint64_t)i;
          const uint64_t* trow = adj_key + (int64_t)ut * adj_stride;
          int lo = 0, hi = -1, found = -1;
          bool ranged = false;
          if (own_tab) {
            const int len2 = (int)(vm_from_bits((uint32_t)(key >> 32)) * inv_res2 + 0.5f);  // integer offset length (exact: the row is in band)
            const int r = len2 < 256 ? (int)s_rank[len2] : 255;
            if (r != 255) {
              const uint16_t* gt = gtab + (int64_t)ut * gstride;
              const uint32_t g0 = gt[r], g1 = gt[r + 1];
              if (g0 != 0xffffu) { lo = (int)g0; hi = (int)g1 - 1; ranged = true; }   // 0xffff: t's row has no table
            } else {
              ranged = true;  // a length that no offset has: not in any row
            }
          }
          if (!ranged) { lo = 0; hi = (int)adj_cnt[ut] - 1; }
          while (lo <= hi) {
            const int mid = (lo + hi) >> 1;
            const uint64_t kk = trow[mid];
            if (kk == want) { found = mid; break; }
            if (kk < want) lo = mid + 1; else hi = mid - 1;
          }
          if (found >= 0 && conn[(int64_t)ut * adj_stride + found]) mflag = 1;
        }
      }
      if (mflag && t < best && (!owned || owned[i] || owned[t])) best = t;   // (tiled runs: a connection is trusted only if one endpoint is owned)
      mrow[k] = mflag;
      kept += mflag;
    }
    mf_wave_sync();   // the next round's fill overwrites the list
  }
  if (pending) {   // what was written to a row that is put off is overwritten by the second pass
    if ((__ballot(touches_pending) & mine) != 0ull) {
      if (sub == 0) { defer_list[atomicAdd(n_defer, 1u)] = (uint32_t)u; if (defer_flag) defer_flag[u] = 1; }
      return;
    }
    if (defer_flag && sub == 0) defer_flag[u] = 0;   // every row of the first pass writes its flag: nobody zeroes the array
  }
  for (int o = W / 2; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
  if (sub == 0) csize[i] = (uint32_t)kept;
  if (parent) {  // (null: a row put off while the unions ran early takes no first hook, its parent may have moved)
    for (int o = W / 2; o > 0; o >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)best, o, 64); best = other < best ? other : best; }
    if (sub == 0) parent[i] = best;
  }
}

// ------------------------------------------------------------------ closestCheck
// flags: bit0 candidate (list == {self} and adjacency vector longer than adjacency_min), bit1 success
__global__ void k_cc_candidates(const uint32_t* __restrict__ used_ids, int64_t U, const uint32_t* __restrict__ adj_nall,
                                const uint32_t* __restrict__ csize, int adjacency_min, uint8_t* __restrict__ flags,
                                uint32_t* __restrict__ cand_list, unsigned int* __restrict__ n_cand) {
  int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const uint32_t i = used_ids[u];
  // voxels_adjacency_idx_[i] = [count, idx...]: its size is n + 1 (VS:2201)
  const bool cand = (csize[i] == 1u) && ((int)adj_nall[u] + 1 > adjacency_min);
  if (cand) { flags[i] = 1; cand_list[atomicAdd(n_cand, 1u)] = (uint32_t)u; }
}

// scan entry j of voxel i's raw adjacency vector: j == 0 is the neighbour COUNT read as a voxel id (Q7, VS:2243)
__device__ __forceinline__ int cc_entry(int j, int n_all, const uint64_t* row, const MgParams& P) {
  if (j == 0) {
    if (!P.q7 || (int64_t)n_all >= P.V) return -1;
    return n_all;
  }
  return (int)(uint32_t)row[j - 1];
}

template <bool CHOOSE>
__global__ __launch_bounds__(64) void k_cc_pass(const uint32_t* __restrict__ cand_list, int n_cand, const uint32_t* __restrict__ used_ids,
                                                const uint64_t* __restrict__ adj_key, const uint32_t* __restrict__ adj_cnt,
                                                const uint32_t* __restrict__ adj_nall, int adj_stride,
                                                const NodeRec* __restrict__ node, const uint32_t* __restrict__ csize,
                                                uint8_t* __restrict__ flags, MgParams P, int32_t* __restrict__ attach,
                                                unsigned int* __restrict__ changed) {
  if ((int)blockIdx.x >= n_cand) return;
  const int lane = threadIdx.x;
  const uint32_t u = cand_list[blockIdx.x];
  const uint32_t i = used_ids[u];
  if (!CHOOSE && (flags[i] & 2)) return;
  if (CHOOSE && !(flags[i] & 2)) { if (lane == 0) attach[i] = -1; return; }
  // the row may hold the used neighbours only: an unused voxel is never an eligible target (its list is empty),
  // so skipping it changes neither the choice nor the "last equal weight wins" order
  const int n = (int)adj_cnt[u];
  const int n_all = (int)adj_nall[u];
  const uint64_t* row = adj_key + (int64_t)u * adj_stride;
  const NodeRec me = node[i];
  float best_w = -1.0f;
  int best_j = -1, best_t = -1;
  bool any = false;
  for (int j = lane; j < n + 1; j += 64) {
    const int t = cc_entry(j, n_all, row, P);
    if (t < 0) continue;
    // eligible at voxel i's turn: list longer than one after crossValidation, or an earlier candidate that succeeded
    const bool elig = (csize[t] > 1u) || ((uint32_t)t < i && (flags[t] & 3) == 3);
    if (!elig) continue;
    const float w = vm_pair_weight(me, node[t], P.W);  // distanceProbability == distanceWeight (Q8)
    if (w != w) continue;                               // NaN >= x is false (VS:2281)
    any = true;
    if (CHOOSE && w >= best_w) { best_w = w; best_j = j; best_t = t; }  // ascending j per lane: later equal weights win
  }
  if (!CHOOSE) {
    if (__ballot(any) != 0ull && lane == 0) { flags[i] |= 2; atomicOr(changed, 1u); }
  } else {
    // wave arg-max on (w, j)
    for (int o = 32; o > 0; o >>= 1) {
      const float ow = __shfl_xor(best_w, o, 64);
      const int oj = __shfl_xor(best_j, o, 64);
      const int ot = __shfl_xor(best_t, o, 64);
      if (ow > best_w || (ow == best_w && oj > best_j)) { best_w = ow; best_j = oj; best_t = ot; }
    }
    if (lane == 0) { attach[i] = best_t; if (best_t >= 0) atomicAdd(changed, 1u); }  // `changed` counts re-attachments in this pass
  }
}

// ------------------------------------------------------------------ connected components
// (uf_find, uf_union, uf_root: unionfind.hpp, shared with labelcc.hip)

// one pass instead of five fills: parent = identity, the per-voxel tables of the stage at their start values
__global__ void k_merge_init(uint32_t* __restrict__ parent, uint32_t* __restrict__ csize, int32_t* __restrict__ attach,
                             uint8_t* __restrict__ cc_flags, uint32_t* __restrict__ csz, int64_t n) {
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) { parent[v] = (uint32_t)v; csize[v] = 0u; attach[v] = -1; cc_flags[v] = 0; csz[v] = 0u; }
}

// UM_ROWS rows per wavefront, 64 / UM_ROWS lanes each.  The row is compacted like crossValidation's (see mf_load, mf_append): a
// fifth of its entries are mutual and half of those have t > i, so eight lanes take most rows' unions in one to three trips of the
// dense pass, and eight rows per wavefront keep eight chains (flags -> keys -> parents) in flight at the same occupancy
// (measured with the compacted rows: 4 rows 158 us per call, 8 rows 143 us; before the compaction 8 rows bought nothing).
#ifndef UM_ROWS
#define UM_ROWS 8
#endif
__global__ __launch_bounds__(64) void k_union_mutual(const uint32_t* __restrict__ used_ids, int64_t U, const uint64_t* __restrict__ adj_key,
                                                     const uint32_t* __restrict__ adj_cnt, int adj_stride,
                                                     const uint8_t* __restrict__ mutual, const int32_t* __restrict__ attach,
                                                     const uint8_t* __restrict__ owned, uint32_t* __restrict__ parent, int do_attach,
                                                     const uint8_t* __restrict__ skip, const uint32_t* __restrict__ work, int n_work, LcGate gate) {
  if (!lc_gate_open_early(gate)) return;
  constexpr int W = 64 / UM_ROWS;
  // plain order: neighbouring voxels on one XCD at the same time contend for the same roots (measured slower)
  int64_t u = (int64_t)blockIdx.x * UM_ROWS + (threadIdx.x / W);
  const int sub = threadIdx.x % W;
  if (work) { if (u >= n_work) return; u = (int64_t)work[u]; }   // the rows of a list (the second pass of crossValidation)
  if (u >= U) return;
  // the head of the row's chain in one wait: its skip flag, id and length, and the first batch of mutual flags (read without
  // knowing the length: the row's allocation, adj_stride, bounds the loads)
  constexpr int T = 8, CAP = MF_CAP_TRIPS * W;
  const uint64_t* row = adj_key + u * adj_stride;
  const uint8_t* mrow = mutual + u * adj_stride;
  const uint8_t skipped = skip ? skip[u] : (uint8_t)0;             // rows whose mutual flags are not final yet
  const uint32_t i = used_ids[u];
  const int n = (int)adj_cnt[u];
  uint8_t f[T];
  mf_load<W, T>(mrow, adj_stride, 0, sub, f);
  if (skipped) return;
  // after the first hook and the pointer jumping most neighbours already hang under the same node: equal parents mean
  // one tree, whatever other wavefronts do meanwhile (links are only ever added), and cost one load instead of two finds
  const uint32_t pi = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __shared__ uint16_t s_list[UM_ROWS][MF_CAP_TRIPS * W];
  const int lane = threadIdx.x, grp = lane / W;
  uint16_t* list = s_list[grp];
  const unsigned long long mine = (W == 64) ? ~0ull : (((1ull << W) - 1ull) << (grp * W));
  for (int k0 = 0; k0 < n;) {
    // flag pass: the positions of the mutual entries, as many trips as the list is sure to hold
    int cnt = 0;
    for (; k0 < n && cnt + T * W <= CAP; k0 += T * W) {
      if (k0 > 0) mf_load<W, T>(mrow, n, k0, sub, f);
      mf_append<W, T>(f, nullptr, n, k0, sub, mine, list, cnt);
    }
    mf_wave_sync();
    // dense pass: every lane carries a mutual entry
    for (int j = sub; j < cnt; j += W) {
      const uint32_t t = (uint32_t)row[list[j]];
      // tiled runs: a connection is trusted only if one endpoint is owned (both neighbourhoods are then complete)
      if (t > i && (!owned || owned[i] || owned[t])) {  // each mutual edge appears in both rows: union once
        if (__hip_atomic_load(&parent[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pi) continue;
        uf_union(parent, i, t);
      }
    }
    mf_wave_sync();   // the next round's fill overwrites the list
  }
  if (sub == 0 && do_attach) {
    const int32_t t = attach[i];
    if (t >= 0 && (!owned || owned[i])) uf_union(parent, i, (uint32_t)t);
  }
}

// the re-attachment edges on their own (closestCheck's candidates only): used when the mutual edges were united while the host
// was still fetching closestCheck's fixed-point flag
__global__ void k_union_attach(const uint32_t* __restrict__ cand, int n_cand, const uint32_t* __restrict__ used_ids, const int32_t* __restrict__ attach,
                               uint32_t* __restrict__ parent, const uint8_t* __restrict__ owned) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cand) return;
  const uint32_t i = used_ids[cand[j]];
  const int32_t t = attach[i];
  if (t >= 0 && (!owned || owned[i])) uf_union(parent, i, (uint32_t)t);   // (tiled runs: the owner of the isolated voxel decides its re-attachment)
}

// pointer jumping between the first hook and the union pass: every later find starts one hop from a root
__global__ void k_compress(uint32_t* __restrict__ parent, int64_t V) {
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const uint32_t r = uf_find(parent, (uint32_t)v);
  if (r != (uint32_t)v) __hip_atomic_store(&parent[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The unions are complete: every voxel gets its ROOT as parent, by the read-only walk of uf_root (unionfind.hpp says why it must not write).
__device__ __forceinline__ void k_flatten_body(uint32_t* __restrict__ parent, int64_t V, const uint8_t* __restrict__ owned, uint32_t* __restrict__ csz,
                                               uint32_t* s_root, unsigned int* s_cnt);
__global__ void k_flatten(uint32_t* __restrict__ parent, int64_t V, const uint8_t* __restrict__ owned, uint32_t* __restrict__ csz) {
  __shared__ uint32_t s_root[32];
  __shared__ unsigned int s_cnt[32];
  if (threadIdx.x < 32) { s_root[threadIdx.x] = 0xffffffffu; s_cnt[threadIdx.x] = 0u; }
  __syncthreads();
  k_flatten_body(parent, V, owned, csz, s_root, s_cnt);
  __syncthreads();
  if (threadIdx.x < 32 && s_cnt[threadIdx.x]) atomicAdd(&csz[s_root[threadIdx.x]], s_cnt[threadIdx.x]);
}
__device__ __forceinline__ void k_flatten_body(uint32_t* __restrict__ parent, int64_t V, const uint8_t* __restrict__ owned, uint32_t* __restrict__ csz,
                                               uint32_t* s_root, unsigned int* s_cnt) {
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const uint32_t r = uf_root(parent, (uint32_t)v);
  __hip_atomic_store(&parent[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // one atomic per distinct root per wavefront (large segments would otherwise serialise on one address).  A voxel that is its own
  // root counts itself on its own: half of a scanned scene's voxels are unused singletons, 64 distinct roots per wavefront, and
  // walked the loop below 64 times (round 5)
  const bool counted = !owned || owned[v];   // tiled runs count owned voxels only
  const bool self = r == (uint32_t)v;
  if (counted && self) atomicAdd(&csz[r], 1u);
  unsigned long long todo = __ballot(counted && !self);
  if (!counted || self) return;
  const int lane = threadIdx.x & 63;
  while (todo) {
    const int l0 = __ffsll((long long)todo) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)r, l0, 64);
    const unsigned long long same = __ballot(r == r0) & todo;
    if (lane == l0) {
      // (round 6) through a small table of the workgroup first: the ground of a scanned scene is one root for a fifth of the voxels, and
      // one global atomic per wavefront on that one address was most of this kernel's 100 us
      const unsigned int n = (unsigned int)__popcll(same);
      unsigned int h = (r0 * 2654435761u) >> 27;   // 32 slots
      bool put = false;
      for (int probe = 0; probe < 4 && !put; ++probe, h = (h + 1u) & 31u) {
        const uint32_t prev = atomicCAS(&s_root[h], 0xffffffffu, r0);
        if (prev == 0xffffffffu || prev == r0) { atomicAdd(&s_cnt[h], n); put = true; }
      }
      if (!put) atomicAdd(&csz[r0], n);
    }
    todo &= ~same;
    if ((same >> lane) & 1ull) break;
  }
}

__global__ __launch_bounds__(1024) void k_root_flags(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ csz, int64_t V, int voxels_min,
                                                     uint32_t* __restrict__ keep_flag, unsigned int* __restrict__ n_roots) {
  __shared__ unsigned int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool root = false;
  if (v < V) {
    root = parent[v] == (uint32_t)v;
    keep_flag[v] = (root && (int)csz[v] > voxels_min) ? 1u : 0u;  // clusters_voxel_idx_[m].size() > cluster_voxels_min_ (VS:969)
  }
  // one global atomic per 1024 voxels (same-address atomics serialise: one per wavefront cost 0.15 ms at 10^6 voxels)
  const unsigned long long m = __ballot(root);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt, (unsigned int)__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(n_roots, s_cnt);
}

__global__ void k_voxel_labels(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ keep_flag,
                               const uint32_t* __restrict__ keep_rank, int64_t V, int32_t* __restrict__ vox_label,
                               unsigned int* __restrict__ n_kept) {
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const uint32_t r = parent[v];
  vox_label[v] = keep_flag[r] ? (int32_t)keep_rank[r] : -1;
  if (v == V - 1) *n_kept = keep_rank[v] + keep_flag[v];   // number of kept segments, for the stage's one read-back
}

__global__ void k_point_labels(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pt_vox, const int32_t* __restrict__ vox_label,
                               int64_t N, int32_t* __restrict__ label) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const uint32_t v = pt_vox[j];
  label[perm[j]] = (v == 0xffffffffu) ? -1 : vox_label[v];
}

// the per-point labels of a context whose merge stage left them to be asked for (a tile between vgs_segment and the label hand-back)
vgs_status vgs_ensure_point_labels(vgs_ctx* c) {
  if (!c->pt_labels_pending) return VGS_OK;
  c->pt_labels_pending = false;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (c->d2h_open && c->d2h_src == c->pt_label.p) { VGS_HIP_TRY(c, hipEventSynchronize(c->ev_d2h)); c->d2h_open = false; }
  const int TB = 256;
  hipLaunchKernelGGL(k_point_labels, dim3((unsigned)((c->N + TB - 1) / TB)), dim3(TB), 0, c->stream, c->perm_b.p, c->pt_vox.p, c->vox_label.p,
                     c->N, c->pt_label.p);
  VGS_HIP_TRY(c, hipEventRecord(c->ev[EV_LABELS_END], c->stream));
  c->labels_event_valid = true;
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGS_OK;
}

static VgsWeightParams make_weight_params_m(const vgs_params& p) {
  VgsWeightParams W;
  W.inv_sig_p = 1.0f / p.sig_p; W.inv_sig_n = 1.0f / p.sig_n; W.inv_sig_o = 1.0f / p.sig_o;
  W.inv_sig_e = 1.0f / p.sig_e; W.inv_sig_c = 1.0f / p.sig_c;
  W.inv_sig_w2 = 1.0f / (p.sig_w * p.sig_w);
  W.svgs = (p.method == 3) ? 1 : 0;
  return W;
}

// ------------------------------------------------------------------ diagnostics: the affinity matrix of one local graph
// W[a * n + b] = distanceWeight(measuringDistance(row[a], row[b])) with row[a] as the FIRST argument (VS:1796-1910): the
// n x n matrix buildAdjacencyGraph fills for node i, over the entries of the stored adjacency row.
__global__ void k_local_weights(const uint64_t* __restrict__ row, int n, const NodeRec* __restrict__ node, VgsWeightParams W,
                                int32_t* __restrict__ ids, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) ids[t] = (int32_t)(uint32_t)row[t];
  if (t >= (int64_t)n * n) return;
  const int a = (int)(t / n), b = (int)(t % n);
  out[t] = vm_pair_weight(node[(uint32_t)row[a]], node[(uint32_t)row[b]], W);
}

extern "C" vgs_status vgs_get_local_weights(vgs_ctx* c, int32_t node_id, int32_t* n_out, int32_t* ids, float* weights) {
  if (!c || !n_out) return VGS_E_ARG;
  if (c->stage < ST_ADJACENCY) { c->err = "vgs_get_local_weights: adjacency first"; return VGS_E_STATE; }
  if (node_id < 0 || node_id >= c->V) { c->err = "vgs_get_local_weights: node id out of range"; return VGS_E_ARG; }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  uint32_t u = 0xffffffffu;
  VGS_HIP_TRY(c, hipMemcpy(&u, c->used_rank.p + node_id, 4, hipMemcpyDeviceToHost));
  if (u == 0xffffffffu) { *n_out = 0; return VGS_OK; }   // an unused voxel has no local graph (VS:384)
  uint32_t n = 0;
  VGS_HIP_TRY(c, hipMemcpy(&n, c->adj_cnt.p + u, 4, hipMemcpyDeviceToHost));
  *n_out = (int32_t)n;
  if (!ids || !weights || n == 0) return VGS_OK;
  DevBuf<float> d_w; DevBuf<int32_t> d_ids;
  VGS_HIP_TRY(c, d_w.ensure((size_t)n * n)); VGS_HIP_TRY(c, d_ids.ensure(n));
  const int64_t total = (int64_t)n * n;
  hipLaunchKernelGGL(k_local_weights, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->adj_key.p + (size_t)u * c->adj_stride, (int)n,
                     c->node.p, make_weight_params_m(c->P), d_ids.p, d_w.p);
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(weights, d_w.p, (size_t)total * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ids, d_ids.p, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { c->err = std::string("vgs_get_local_weights: ") + hipGetErrorString(e); return VGS_E_HIP; }
  return VGS_OK;
}

vgs_status vgs_stage_merge(vgs_ctx* c) {
  c->cl_valid = false;   // (clusters.hip: the cluster lists on the device belong to the labels of the last run)
  c->sd_valid = false;   // (segdesc.hip: so do the segment descriptors)
  c->sb_valid[0] = c->sb_valid[1] = false;   // (segbox.hip: and the oriented boxes)
  c->sg_valid = false; c->cmp_valid = false; c->rf_valid = false; c->lcc_valid = false; c->lg_valid = false; c->la_valid = false; c->lgt_own = c->lgt_valid = false; c->cmp_own_cells = -1; c->pso_K = -1; c->sg_halo_valid = false; c->sg_own_K = -1; c->rf_halo_valid = false; c->rf_band_n = -1;   // (seggraph.hip: and the segment graph)
  const int64_t V = c->V, U = c->U, N = c->N;
  c->bnd_unique = -1;  // tile protocol results belong to the previous segmentation
  c->counts[VGS_N_CLUSTERS] = 0; c->counts[VGS_N_KEPT] = 0; c->counts[VGS_N_ISOLATED] = 0; c->counts[VGS_N_REATTACHED] = 0;
  // an asynchronous download (vgs_get_point_labels_async) may still read the last labels: this run writes the other buffer
  if (c->d2h_open && c->d2h_src == c->pt_label.p) std::swap(c->pt_label, c->pt_label_alt);
  VGS_HIP_TRY(c, c->pt_label.ensure(N > 0 ? N : 1));
  if (V == 0) {
    if (N > 0) {
      VGS_HIP_TRY(c, hipMemsetAsync(c->pt_label.p, 0xff, N * sizeof(int32_t), c->stream));
      VGS_HIP_TRY(c, hipEventRecord(c->ev[EV_LABELS_END], c->stream));   // label downloads order themselves behind this fill, not behind an earlier cloud's kernel
      c->labels_event_valid = true;
    }
    c->pt_labels_pending = false;
    return VGS_OK;
  }
  MgParams MP;
  MP.W = make_weight_params_m(c->P);
  MP.adjacency_min = c->P.adjacency_min;
  MP.q7 = c->P.q7_count_as_index;
  MP.V = V;
  const int TB = 256;
  const unsigned nbV = (unsigned)((V + TB - 1) / TB);
  VGS_HIP_TRY(c, c->csize.ensure(V)); VGS_HIP_TRY(c, c->attach.ensure(V)); VGS_HIP_TRY(c, c->cc_flags.ensure(V));
  VGS_HIP_TRY(c, c->parent.ensure(V)); VGS_HIP_TRY(c, c->csz.ensure(V)); VGS_HIP_TRY(c, c->kept_rank.ensure(V + 1));
  VGS_HIP_TRY(c, c->vox_label.ensure(V));
  // this stage's own counter words (MG_W_*, zeroed here): the local cut's hand-over kernels may still be running on theirs (counter_words.hpp)
  VGS_HIP_TRY(c, c->counters.ensure(64));
  uint64_t* mcnt = c->counters.p + CW_MG_BASE;
  VGS_HIP_TRY(c, hipMemsetAsync(mcnt, 0, MG_W_COUNT * sizeof(uint64_t), c->stream));
  hipLaunchKernelGGL(k_merge_init, dim3(nbV), dim3(TB), 0, c->stream, c->parent.p, c->csize.p, c->attach.p, c->cc_flags.p, c->csz.p, V);
  uint8_t* mutual = nullptr;
  unsigned int n_cand = 0, n_succ = 0;
  bool compressed = false, united = false;   // k_compress / the mutual unions already ran behind a read-back of closestCheck
  if (U > 0) {
    if (c->conn.cap < 2 * (size_t)U * c->adj_stride) { c->err = "connect buffer missing (local cut stage not run)"; return VGS_E_STATE; }
    mutual = c->conn.p + (size_t)U * c->adj_stride;  // second half holds the mutual flags
    const uint16_t* gt = (c->P.method == 2 && c->adj_have_gtab) ? c->adj_gtab.p : nullptr;
    const float inv_res2 = 1.0f / (c->P.voxel_size * c->P.voxel_size);
    // Tiled runs: which voxels this rank owns depends on the voxel lattice, the region and the points' sources only, so it is known
    // NOW, not behind closestCheck -- the first hook is taken in k_cross under the ownership test and the unions of the final rows run
    // beside the hand-over kernels as in a single-context run.
    if (c->have_region) { vgs_status so = vgs_compute_owned(c); if (so != VGS_OK) return so; }
    const uint8_t* owned_early = c->have_region ? c->owned.p : (const uint8_t*)nullptr;
    unsigned int* d_ndefer = (unsigned int*)(c->counters.p + CW_MG_NDEFER);   // zeroed with the local cut's counters
    // runs whose hand-over kernels are still running: the unions of the final rows go beside them (see below)
    const bool early_union = c->lc_tail.open && !c->K.no_overlap;
    if (early_union) VGS_HIP_TRY(c, c->lc_defer_flag.ensure((size_t)U));
    // connect bits of the cuts (method 2, rows with lattice offsets): the lattice lookup of k_cross
    const bool use_bits = c->cb_enabled && c->P.method == 2 && c->adj_have_off;
    const uint16_t* cb_off = use_bits ? c->adj_off.p : (const uint16_t*)nullptr;
    const int cb_lut = c->cb_R;
    const uint32_t* cb_bits = use_bits ? c->conn_bits.p : (const uint32_t*)nullptr;
    // crossValidation starts while the hand-over kernels of the local cut still run (vgs_stage_localcut): rows that touch a
    // handed-over voxel are put off, ...
    // (When the hand-overs are MANY -- LcGate's word, written on the device by k_ho_lists -- this first pass would put off every row, one
    // atomic each, and the unions behind it would find nothing final: both return at once, and the plain pass over all rows follows
    // below, behind the hand-over kernels.)
    const LcGate g_first = {(c->lc_tail.open && c->lc_tail.gated) ? (const unsigned int*)(c->counters.p + CW_LC_GATE) : (const unsigned int*)nullptr, LC_FEW};
    const size_t first_lds = (c->lc_tail.open && c->K.cross_lds_kb > 0) ? (size_t)c->K.cross_lds_kb * 1024 : 0;
    hipLaunchKernelGGL(k_cross, dim3(vgs_xcd_grid((U + CX_ROWS - 1) / CX_ROWS)), dim3(64), first_lds, c->stream, c->used_ids.p, c->used_rank.p, U, c->adj_key.p, c->adj_cnt.p,
                       c->adj_stride, c->conn.p, mutual, c->csize.p, c->parent.p, gt, c->adj_gstride, c->adj_nrank.p, inv_res2,
                       c->lc_tail.open ? c->lc_pending.p : (const uint8_t*)nullptr, c->lc_defer.p, d_ndefer, (const uint32_t*)nullptr, 0,
                       cb_off, cb_lut, cb_bits, c->cb_words, early_union ? c->lc_defer_flag.p : (uint8_t*)nullptr, g_first, owned_early);
    // The fork (early_union only).  Behind crossValidation's first pass the stage splits in two chains that share no result until the join:
    //   main stream:  k_compress, k_union_mutual over the rows that are final -- they read the mutual flags of those rows, the put-off
    //                 flags and `parent`, and write `parent` only; then, behind an event of the side stream, k_union_mutual over the rows
    //                 put off, once their second crossValidation pass is through;
    //   side stream:  the local cut's finish (read-back, rest and extra-large launches, connect bits of the handed-over voxels),
    //                 crossValidation over the rows put off (no first hook: parent == nullptr), closestCheck with its read-backs -- they
    //                 write the mutual flags, csize and connect bits of put-off and handed-over rows, cc_flags, attach,
    //                 work_ids[0, n_cand) and the stage's own counter words (MG_W_*), and never touch `parent`.
    // Read from the kernels: k_union_mutual loads the first batch of a row's mutual flags together with its skip flag, so for a put-off
    // row that load may race with the second crossValidation pass -- the loaded bytes are dropped at `if (skipped) return` before any
    // use (a stale or torn byte of a skipped row decides nothing); `attach` is read only under do_attach, which is 0 here.  The skip flags
    // and the put-off list are written by the first pass alone.
    // The side stream is the hand-over kernels' own (stream3, high priority, idle once they end): their last event is stream order there.
    // The host blocks in the side chain's read-backs while the main stream's unions are already queued.
    hipStream_t s = c->stream;   // where the chain from the finish to closestCheck goes
    if (early_union) {
      VGS_HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
      VGS_HIP_TRY(c, hipStreamWaitEvent(c->stream3, c->ev_fork, 0));
      s = c->stream3;
      // (the finish's read-back is queued BEFORE the unions: its copy then runs beside k_compress, not behind k_union_mutual's workgroups)
      { vgs_status sq = vgs_localcut_finish_queue(c, s); if (sq != VGS_OK) return sq; }
      // The unions of the rows that are final go here, beside the hand-over kernels of the local cut (which leave most of the GPU
      // idle and end the critical path of the stage): pointer jumping over the first hooks, then every mutual edge of a row that
      // was not put off.  The rows put off follow behind their second crossValidation pass, without a first hook (their parents
      // may have moved by then).
      hipLaunchKernelGGL(k_compress, dim3(nbV), dim3(TB), 0, c->stream, c->parent.p, V);
      hipLaunchKernelGGL(k_union_mutual, dim3((unsigned)((U + UM_ROWS - 1) / UM_ROWS)), dim3(64), first_lds, c->stream, c->used_ids.p, U, c->adj_key.p, c->adj_cnt.p,
                         c->adj_stride, mutual, c->attach.p, owned_early, c->parent.p, 0, c->lc_defer_flag.p, (const uint32_t*)nullptr, 0, g_first);
      compressed = true; united = true;
    }
    // ... then the local cut is completed (its flags and list lengths read back) and the rows put off follow
    unsigned int n_defer = 0;
    {
      vgs_status sf = vgs_localcut_finish(c, s, &n_defer);
      if (sf != VGS_OK) return sf;
    }
    if (c->lc_tail.many) {
      // (forked: the main stream joins the side chain at once -- the finish's kernels wrote rows this pass reads -- and takes the rest)
      if (s != c->stream) {
        VGS_HIP_TRY(c, hipEventRecord(c->ev_join, s));
        VGS_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        s = c->stream;
      }
      // the first pass and its unions did not run (see above) -- or ran in part, for workgroups that started before the word was written:
      // whatever they left (hooks, unions of rows whose flags nobody wrote this run) goes, and crossValidation takes every row now
      hipLaunchKernelGGL(k_merge_init, dim3(nbV), dim3(TB), 0, c->stream, c->parent.p, c->csize.p, c->attach.p, c->cc_flags.p, c->csz.p, V);
      hipLaunchKernelGGL(k_cross, dim3(vgs_xcd_grid((U + CX_ROWS - 1) / CX_ROWS)), dim3(64), 0, c->stream, c->used_ids.p, c->used_rank.p, U, c->adj_key.p, c->adj_cnt.p,
                         c->adj_stride, c->conn.p, mutual, c->csize.p, c->parent.p, gt, c->adj_gstride, c->adj_nrank.p, inv_res2,
                         (const uint8_t*)nullptr, c->lc_defer.p, d_ndefer, (const uint32_t*)nullptr, 0, cb_off, cb_lut, cb_bits, c->cb_words, (uint8_t*)nullptr,
                         LcGate{nullptr, 0u}, owned_early);
      compressed = false; united = false;
      n_defer = 0;
    }
    if (n_defer > 0) {
      hipLaunchKernelGGL(k_cross, dim3((n_defer + CX_ROWS - 1) / CX_ROWS), dim3(64), 0, s, c->used_ids.p, c->used_rank.p, U, c->adj_key.p, c->adj_cnt.p,
                         c->adj_stride, c->conn.p, mutual, c->csize.p, early_union ? (uint32_t*)nullptr : c->parent.p, gt, c->adj_gstride, c->adj_nrank.p, inv_res2,
                         (const uint8_t*)nullptr, c->lc_defer.p, d_ndefer, c->lc_defer.p, (int)n_defer, cb_off, cb_lut, cb_bits, c->cb_words, (uint8_t*)nullptr, LcGate{nullptr, 0u});
      if (s != c->stream) {
        // The rows put off get their unions as soon as their flags are final, beside closestCheck: the main stream waits for this pass
        // only (it runs behind the first union pass there by stream order).  k_union_mutual with do_attach == 0 reads the mutual flags
        // and `parent`; closestCheck reads and writes neither.  (ev_fork is free again: the side stream's wait for it is queued.)
        VGS_HIP_TRY(c, hipEventRecord(c->ev_fork, s));
        VGS_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_fork, 0));
      }
      if (early_union)
        hipLaunchKernelGGL(k_union_mutual, dim3((n_defer + UM_ROWS - 1) / UM_ROWS), dim3(64), 0, c->stream, c->used_ids.p, U, c->adj_key.p, c->adj_cnt.p,
                           c->adj_stride, mutual, c->attach.p, owned_early, c->parent.p, 0, (const uint8_t*)nullptr, c->lc_defer.p, (int)n_defer, LcGate{nullptr, 0u});
    }
    // closestCheck
    VGS_HIP_TRY(c, c->work_ids.ensure((size_t)U + 16));
    unsigned int* d_ncand = (unsigned int*)(mcnt + MG_W_NCAND);
    unsigned int* d_changed = (unsigned int*)(mcnt + MG_W_CHANGED);
    // (256 threads also beside the union pass: one-wavefront workgroups were measured there and are slower, profiles/ab_merge_fork.txt)
    hipLaunchKernelGGL(k_cc_candidates, dim3((unsigned)((U + TB - 1) / TB)), dim3(TB), 0, s, c->used_ids.p, U, c->adj_mused.p,
                       c->csize.p, MP.adjacency_min, c->cc_flags.p, c->work_ids.p, d_ncand);
    // Two host round trips of closestCheck (the number of candidates, the fixed-point flag) hide behind work that does not depend
    // on it: the pointer jumping over the first hooks, and the unions of the mutual edges (single-context runs only)
    // (not with early_union: there the whole chain runs beside the first unions, on the side stream)
    const bool hide = !c->have_region && vgs_can_split_readback(c) && !early_union;
    if (hide) {
      vgs_status sb = vgs_readback_begin(c, d_ncand, 4);
      if (sb != VGS_OK) return sb;
      hipLaunchKernelGGL(k_compress, dim3(nbV), dim3(TB), 0, c->stream, c->parent.p, V);
      compressed = true;
      vgs_status se = vgs_readback_end(c, &n_cand, 4);
      if (se != VGS_OK) return se;
    } else {
      VGS_READBACK_ON(c, s, &n_cand, d_ncand, 4);
    }
    if (n_cand > 0) {
      // fixed point of "re-attachment succeeds": passes are queued four at a time, each with its own change counter, and
      // only the last counter is read back (a pass after the fixed point changes nothing and costs microseconds; a host
      // round trip per pass cost more than the passes)
      unsigned int* d_chg4 = (unsigned int*)(mcnt + MG_W_CHG4);   // two words: four 32-bit counters
      for (int round = 0; round < 1 << 18; ++round) {
        VGS_HIP_TRY(c, hipMemsetAsync(d_chg4, 0, 16, s));
        for (int q = 0; q < 4; ++q)
          hipLaunchKernelGGL((k_cc_pass<false>), dim3(n_cand), dim3(64), 0, s, c->work_ids.p, (int)n_cand, c->used_ids.p,
                             c->adj_key.p, c->adj_cnt.p, c->adj_mused.p, c->adj_stride, c->node.p, c->csize.p, c->cc_flags.p, MP, c->attach.p, d_chg4 + q);
        unsigned int ch = 0;
        if (hide && !united) {
          vgs_status sb = vgs_readback_begin(c, d_chg4 + 3, 4);
          if (sb != VGS_OK) return sb;
          hipLaunchKernelGGL(k_union_mutual, dim3((unsigned)((U + UM_ROWS - 1) / UM_ROWS)), dim3(64), 0, c->stream, c->used_ids.p, U, c->adj_key.p, c->adj_cnt.p,
                             c->adj_stride, mutual, c->attach.p, (const uint8_t*)nullptr, c->parent.p, 0, (const uint8_t*)nullptr, (const uint32_t*)nullptr, 0, LcGate{nullptr, 0u});
          united = true;
          vgs_status se = vgs_readback_end(c, &ch, 4);
          if (se != VGS_OK) return se;
        } else {
          VGS_READBACK_ON(c, s, &ch, d_chg4 + 3, 4);
        }
        if (!ch) break;
      }
      hipLaunchKernelGGL((k_cc_pass<true>), dim3(n_cand), dim3(64), 0, s, c->work_ids.p, (int)n_cand, c->used_ids.p, c->adj_key.p,
                         c->adj_cnt.p, c->adj_mused.p, c->adj_stride, c->node.p, c->csize.p, c->cc_flags.p, MP, c->attach.p, d_changed);
    }
    if (s != c->stream) {
      // The join: the main stream takes closestCheck's results (attach, the candidate list) from here.
      VGS_HIP_TRY(c, hipEventRecord(c->ev_join, s));
      VGS_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
  } else {
    VGS_HIP_TRY(c, c->conn.ensure(16));
  }
  // connected components
  // (with used voxels, ownership was computed at the head of the stage and k_cross took the first hooks; k_flatten needs it either way)
  if (c->have_region && U == 0) { vgs_status so = vgs_compute_owned(c); if (so != VGS_OK) return so; }
  if (U > 0 && !compressed) hipLaunchKernelGGL(k_compress, dim3(nbV), dim3(TB), 0, c->stream, c->parent.p, V);
  if (U > 0 && !united)
    hipLaunchKernelGGL(k_union_mutual, dim3((unsigned)((U + UM_ROWS - 1) / UM_ROWS)), dim3(64), 0, c->stream, c->used_ids.p, U, c->adj_key.p, c->adj_cnt.p,
                       c->adj_stride, mutual, c->attach.p, c->have_region ? c->owned.p : nullptr, c->parent.p, 1, (const uint8_t*)nullptr, (const uint32_t*)nullptr, 0, LcGate{nullptr, 0u});
  else if (U > 0 && n_cand > 0)
    hipLaunchKernelGGL(k_union_attach, dim3((n_cand + TB - 1) / TB), dim3(TB), 0, c->stream, c->work_ids.p, (int)n_cand, c->used_ids.p, c->attach.p, c->parent.p,
                       c->have_region ? c->owned.p : (const uint8_t*)nullptr);
  hipLaunchKernelGGL(k_flatten, dim3(nbV), dim3(TB), 0, c->stream, c->parent.p, V, c->have_region ? c->owned.p : nullptr, c->csz.p);
  // cluster filter + labels (VGS_T_LABELS: this tail of the stage, measured on its own; it is part of VGS_T_MERGE)
  VGS_HIP_TRY(c, hipEventRecord(c->ev[EV_LABELS_BEGIN], c->stream));   // EV_LABELS_BEGIN, EV_LABELS_END: this tail's own pair
  uint32_t* keep_flag = c->head_flag.p;  // >= N >= V entries, free after features
  VGS_HIP_TRY(c, c->head_flag.ensure(V + 1));
  keep_flag = c->head_flag.p;
  unsigned int* d_nroots = (unsigned int*)(mcnt + MG_W_NROOTS);
  hipLaunchKernelGGL(k_root_flags, dim3((unsigned)((V + 1023) / 1024)), dim3(1024), 0, c->stream, c->parent.p, c->csz.p, V, c->P.method == 3 ? -1 : c->P.voxels_min,
                     keep_flag, d_nroots);
  size_t bytes = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, keep_flag, c->kept_rank.p, 0u, (size_t)V, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, c->sort_tmp.ensure(bytes));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sort_tmp.p, bytes, keep_flag, c->kept_rank.p, 0u, (size_t)V, rocprim::plus<uint32_t>(), c->stream));
  hipLaunchKernelGGL(k_voxel_labels, dim3(nbV), dim3(TB), 0, c->stream, c->parent.p, keep_flag, c->kept_rank.p, V, c->vox_label.p,
                     (unsigned int*)(mcnt + MG_W_NKEPT));
  // (Round 4 measured the scatter-free alternative -- the point's octree key formed again from its coordinates, its voxel from the
  // brick table, label[p] written in input order: 0.26 ms against this kernel's 0.14 ms at 10 M points.  PCL's key arithmetic is
  // double precision -- three fp64 divisions per point -- and that costs more than the 4-byte scatter saves.)
  // A tile's labels are local names: the driver hands the global ones back (vgs_apply_tile_labels / vgs_apply_global_labels rewrite every
  // point's label), so the 40 MB scatter is left to whoever asks for point labels BEFORE that happens (vgs_ensure_point_labels; round 5)
  c->pt_labels_pending = c->have_region && N > 0;
  if (!c->pt_labels_pending)
    hipLaunchKernelGGL(k_point_labels, dim3((unsigned)((N + TB - 1) / TB)), dim3(TB), 0, c->stream, c->perm_b.p, c->pt_vox.p, c->vox_label.p,
                       N, c->pt_label.p);
  VGS_HIP_TRY(c, hipEventRecord(c->ev[EV_LABELS_END], c->stream));
  c->labels_event_valid = true;
  VGS_HIP_TRY(c, hipGetLastError());
  // one read-back: MG_W_CHANGED, MG_W_NROOTS, MG_W_NKEPT = re-attachments, roots, kept segments
  uint64_t hm[MG_W_NKEPT + 1] = {0, 0, 0, 0};
  VGS_READBACK(c, hm, mcnt, sizeof(hm));
  { float lms = 0.f; if (hipEventElapsedTime(&lms, c->ev[EV_LABELS_BEGIN], c->ev[EV_LABELS_END]) == hipSuccess) c->times[VGS_T_LABELS] = lms; }
  const unsigned int n_roots = (unsigned int)hm[MG_W_NROOTS];
  if (U > 0 && n_cand > 0) n_succ = (unsigned int)hm[MG_W_CHANGED];
  c->counts[VGS_N_REATTACHED] = n_succ;
  c->counts[VGS_N_CLUSTERS] = n_roots;
  c->counts[VGS_N_KEPT] = (int64_t)(unsigned int)hm[MG_W_NKEPT];
  c->counts[VGS_N_ISOLATED] = n_cand;
  return VGS_OK;
}
