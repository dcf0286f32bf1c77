// labelgraph_walk.hpp -- the row walk of the label graph, one copy for labelgraph.hip (k_lg_rows, one context) and labelgraph_tiles.hip
// (k_lgt_rows, a tile context of the tiled driver).  labelgraph.hip's header has the counting rule and what a proxy record is;
// include/vgs_tiles.h has the rule that places every record on one rank.
#ifndef VGS_LABELGRAPH_WALK_HPP_
#define VGS_LABELGRAPH_WALK_HPP_

#include <climits>

#include "vgs_context.hpp"
#include "wavefold.hpp"

#define LG_WAVES 4                 // wavefronts per workgroup of the row, chunk and edge kernels
#define LG_NONE 0xffffffffu
#define LG_CONTACT 1u
#define LG_SHARED 2u
enum { LG_HOLDS_ALWAYS = 0, LG_HOLDS_UNUSED = 1, LG_HOLDS_SEARCH = 2 };

#ifdef __HIPCC__
// first position of slab[b .. e) whose label is not below l
__device__ __forceinline__ uint32_t lg_lower(const uint32_t* __restrict__ slab, uint32_t b, uint32_t e, int32_t l) {
  while (b < e) { const uint32_t mid = (b + e) >> 1; if ((int32_t)slab[mid] < l) b = mid + 1; else e = mid; }
  return b;
}

// One wavefront per position t = vertex (A, u) of the list in (node, label) order.  urow == nullptr: the stored rows (a node without one has
// an empty row if no_row_is_empty -- SVGS -- and leaves otherwise); urow != nullptr: the rows built for the nodes row0 .. row0 + n_rows - 1
// of the unused list, every other vertex leaves.  WRITE = false: n_rec[t] = its records, and the proxies among them are added to meta[2];
// WRITE = true: the records at rec_off[t] ...
// TILE (a tile context; owned[v] = 1 where the rank owns node v): a vertex at an owned node walks in full, and writes only the proxies
// whose target node is owned; a vertex at a non-owned node walks a built row only, and only under LG_HOLDS_UNUSED (pruned stored rows:
// the one case with proxies) -- it writes the proxies whose target node is owned, no record of its own and no count.  Every other vertex
// leaves.  Whether a vertex leaves and in which mode it walks depends on its node alone: whole wavefronts decide, and no barrier
// follows.  The tiled path is VGS only: LG_HOLDS_SEARCH is not compiled in, and adj_key / adj_cnt are read for the stored rows alone.
template <bool WRITE, bool TILE>
__device__ __forceinline__ void lg_walk_body(uint32_t nv, const uint32_t* __restrict__ snode, const uint32_t* __restrict__ slab,
                                             const uint32_t* __restrict__ nbeg, const uint32_t* __restrict__ nend,
                                             const uint32_t* __restrict__ used_rank, const uint64_t* __restrict__ adj_key,
                                             const uint32_t* __restrict__ adj_cnt, int adj_stride, const uint32_t* __restrict__ urow,
                                             uint32_t row0, uint32_t n_rows, const uint64_t* __restrict__ rows,
                                             const uint32_t* __restrict__ rows_cnt, int no_row_is_empty, int holds,
                                             const NodeRec* __restrict__ node, VgsWeightParams W, uint32_t K, uint32_t R,
                                             uint32_t* __restrict__ n_rec, const uint64_t* __restrict__ rec_off, LgRec* __restrict__ rec,
                                             uint64_t* __restrict__ rkey, uint32_t* __restrict__ tkey, uint32_t* __restrict__ ridx,
                                             uint32_t* __restrict__ meta, const uint8_t* __restrict__ owned) {
  const uint32_t t = blockIdx.x * LG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= nv) return;   // (whole wavefronts; no barrier follows)
  const uint32_t u = snode[t];
  const int32_t A = (int32_t)slab[t];
  const uint32_t ru = used_rank[u];
  bool proxy_only = false;   // (TILE) the vertex speaks only for owned vertices of other nodes
  if (TILE) {
    proxy_only = owned[u] == 0;
    if (proxy_only && (urow == nullptr || holds != LG_HOLDS_UNUSED)) return;
  }
  const uint64_t* row = nullptr;
  uint32_t n = 0;
  if (urow == nullptr) {
    if (ru != LG_NONE) { row = adj_key + (int64_t)ru * adj_stride; n = min(adj_cnt[ru], (uint32_t)adj_stride); }
    else if (!no_row_is_empty) return;
  } else {
    const uint32_t j = urow[t];
    if (j == LG_NONE || j < row0 || j - row0 >= n_rows) return;
    row = rows + (int64_t)(j - row0) * adj_stride;
    n = min(rows_cnt[j - row0], (uint32_t)adj_stride);
  }
  const uint32_t ub = nbeg[u], ue = nend[u];
  uint32_t o = 0;   // (the host refuses 2^31 records and more: positions fit a word)
  if (WRITE) o = (uint32_t)rec_off[t];
  uint32_t k = 0, n_proxy = 0;
  int32_t cur = -1;   // the label this walk folds (none on the first walk)
  while (true) {
    int nxt = INT_MAX;
    int c_cnt = 0, c_fin = 0;
    bool seen = false, shared = false;
    double s = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    if (lane == 0 && !proxy_only) {   // u's own other labels
      uint32_t p = lg_lower(slab, ub, ue, cur);
      if (p < ue && (int32_t)slab[p] == cur) { shared = cur >= 0; ++p; }
      if (p < ue && (int32_t)slab[p] == A) ++p;
      if (p < ue) nxt = (int)slab[p];
    }
    for (uint32_t base = 0; base < n; base += 64) {
      const uint32_t j = base + lane;
      bool proxy = false;
      uint32_t px = 0;
      if (j < n) {
        const uint64_t e = row[j];
        const uint32_t x = (uint32_t)e;
        const uint32_t xb = nbeg[x], xe = nend[x];
        if (x != u && xb != xe) {   // (a stored row starts with its own node)
          uint32_t p = xe - xb == 1u ? xb + ((int32_t)slab[xb] < cur ? 1u : 0u) : lg_lower(slab, xb, xe, cur);
          const bool has = cur >= 0 && p < xe && (int32_t)slab[p] == cur;
          uint32_t q = has ? p + 1u : p;
          if (q < xe && (int32_t)slab[q] == A) ++q;
          if (q < xe) nxt = min(nxt, (int)slab[q]);
          if (has) {
            const uint32_t rx = used_rank[x];
            bool hx = true;
            if (holds == LG_HOLDS_UNUSED) hx = rx == LG_NONE;
            else if (!TILE && holds == LG_HOLDS_SEARCH)
              hx = rx != LG_NONE && sg_in_row(adj_key + (int64_t)rx * adj_stride, min(adj_cnt[rx], (uint32_t)adj_stride), (e & 0xffffffff00000000ull) | (uint64_t)u, u);
            if (!proxy_only) {
              seen = true;
              if (u < x || !hx) {
                ++c_cnt;
                if (ru != LG_NONE && rx != LG_NONE) {
                  // the lower id first: vgs_get_local_weights' entry of that ordered pair
                  const float w = u < x ? vm_pair_weight(node[u], node[x], W) : vm_pair_weight(node[x], node[u], W);
                  if (!isnan(w)) { ++c_fin; s += (double)w; mn = fminf(mn, w); mx = fmaxf(mx, w); }
                }
              }
            }
            if (!hx && (!TILE || owned[x] != 0)) { proxy = true; px = p; }
          }
        }
      }
      const unsigned long long pm = __ballot(proxy);
      if (pm != 0ull) {
        if (WRITE && proxy) {
          const uint32_t at = o + k + (uint32_t)__popcll(pm & ((1ull << lane) - 1ull));
          if (at < R) {   // (the count walk sized the range: the bound only guards the arrays)
            LgRec q;
            q.w_sum = 0.0; q.cnt = 0u; q.n_finite = 0u; q.a = cur; q.b = A; q.w_min = __builtin_huge_valf(); q.w_max = -__builtin_huge_valf();
            q.t = px; q.flags = LG_CONTACT;
            rec[at] = q;
            const uint64_t lo = (uint64_t)(A < cur ? A : cur), hi = (uint64_t)(A < cur ? cur : A);
            rkey[at] = lo * (uint64_t)K + hi;
            tkey[at] = px;
            ridx[at] = at;
          }
        }
        k += (uint32_t)__popcll(pm);
        n_proxy += (uint32_t)__popcll(pm);
      }
    }
    if (cur >= 0 && !proxy_only) {
      if (WRITE) {
        c_cnt = sg_wave_sum(c_cnt); c_fin = sg_wave_sum(c_fin);
        s = sg_wave_sum(s); mn = sg_wave_min(mn); mx = sg_wave_max(mx);
        const bool any_seen = __ballot(seen) != 0ull, any_shared = __ballot(shared) != 0ull;
        const uint32_t at = o + k;
        if (lane == 0 && at < R) {
          LgRec q;
          q.w_sum = s; q.cnt = (uint32_t)c_cnt; q.n_finite = (uint32_t)c_fin; q.a = A; q.b = cur; q.w_min = mn; q.w_max = mx;
          q.t = t; q.flags = (any_seen ? LG_CONTACT : 0u) | (any_shared ? LG_SHARED : 0u);
          rec[at] = q;
          const uint64_t lo = (uint64_t)(A < cur ? A : cur), hi = (uint64_t)(A < cur ? cur : A);
          rkey[at] = lo * (uint64_t)K + hi;
          tkey[at] = t;
          ridx[at] = at;
        }
      }
      ++k;
    }
    nxt = sg_wave_min(nxt);
    if (nxt == INT_MAX) break;
    cur = nxt;
  }
  if (!WRITE && lane == 0) {
    n_rec[t] = k;
    if (n_proxy) atomicAdd(&meta[2], n_proxy);   // (an integer count: the same whatever the order)
  }
}
#endif

#endif
