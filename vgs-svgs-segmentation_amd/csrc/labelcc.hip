// labelcc.hip -- the connected parts of a per-POINT labelling of the context's cloud that the CALLER supplies (include/vgs.h:
// vgs_point_label_components; no reference counterpart).  The tables of pointseg.hip, pointfield.hip and segcompare.hip treat a label
// as a set of points; this pass says whether that set is one object or several, over the scene's own neighbourhood graph.
//
// Definition (include/vgs.h states it in full).  Nodes: what pt_vox holds, voxels for VGS, supervoxels for SVGS.  Vertices: the distinct
// pairs (label l, node v) with a point of v carrying l.  (l, v) and (l, w) are joined when w is in the adjacency row of v OR v is in the
// row of w, the rows those of vgs_get_lists(which = 0).  A part is a connected component; parts are numbered in ascending (label,
// smallest node id of the part).
//
// Data flow (perm_b gives the input index of a sorted position, pt_vox its node):
//   1. k_ps_keys and the stable radix sort of pointseg.hip (ps_sort_points, the ps_* scratch): a label's points are one run, positions
//      ascending inside it -- and the positions are in leaf order, so inside a run the points of a node are adjacent and the nodes ascend
//   2. k_lc_heads     head flag of a sorted point: labelled, and the first of its label's run or of another node than its predecessor;
//                     an exclusive scan gives every sorted point its vertex, the total the number of vertices            -> read-back
//      k_lc_vertices  per vertex: node, label, first sorted point, parent = itself; and per node its lowest and highest vertex (integer
//                     atomicMin / atomicMax into nlo / nhi, V words each).  k_lc_vfirst: the first vertex of every label
//      The vertex list is in (label, node) order: label l's vertices are the run vfirst[l] .. vfirst[l + 1], sorted by node.
//   3. k_lc_link_short / k_lc_link_long: the row of a vertex's node -- the stored row of a used node (adj_key by used rank), or for VGS
//      the row of an unused voxel, which the hot path does not keep: those vertices are compacted into a list (k_lc_unused_flags, scan,
//      k_lc_unused_list) and their rows built with every neighbour (full = true) a chunk at a time by vgs_run_adjacency over the list of
//      their node ids, as refine.hip does, in refine.hip's row scratch.  For every neighbour w the vertex (l, w) is looked up (lc_lookup)
//      and united with (l, v): the equal-parent shortcut of k_union_mutual first, uf_union (unionfind.hpp, min-hooking) otherwise.
//      Rows of at most LC_SHORT entries go eight to a wavefront, eight lanes each; longer rows (adj_stride reaches 8192) get a whole
//      wavefront.  Both kernels run over the same list and each leaves the other's rows alone.
//   4. k_lc_compress (pointer jumping) behind the stored rows and behind every chunk; k_lc_roots: the root of every vertex by read-only
//      walks (uf_root: unionfind.hpp says why) into an array of its own, and the root flags; exclusive scan -> part ids    -> read-back
//   5. k_lc_parts: part of every vertex; per part the points and nodes (integer atomics), label and first node (its root's: the root is
//      the smallest vertex of the component, and inside a label the vertices ascend by node).  k_lc_label_first, k_lc_largest_fold (one
//      64-bit atomicMax of points << 32 | ~part per part: most points, lowest id on a tie), k_lc_largest.  k_lc_scatter: part_of_point
//      through the sorted positions and perm, after a fill of -1.
// The lookup of (l, w): the per-node index first -- w's lowest vertex is the one of its smallest label, its highest that of its largest, so
// a node with one or two labels, and any label outside a node's range, is settled by two dependent loads (nlo[w], the vertex's label) or
// four; only a label strictly between the two falls back to the binary search inside label l's run (about log2 of the run: 20 dependent
// loads at a million vertices).  Measured on the 10 M-point scene the index bought nothing over the search alone (the searches hit the
// L2); what did was uniting every edge from one side (LC_BACK_* below).  DESIGN.md 8 has the figures of all three versions.
// Why the symmetric closure costs nothing extra: an edge {v, w} between two nodes that both hold labelled points is in the row this pass
// reads for v or in the one it reads for w.  The rows of unused voxels are built in full.  A stored row may be pruned to used neighbours
// (adj_pruned), so it misses an unused w -- but then w's own full row has v, since the rows' predicate (float d2 between voxel centres
// below r2, adjacency.hip) is symmetric; two used nodes find each other in either stored row.  uf_union is symmetric, so honouring an
// edge from one side is honouring it.  For SVGS vgs_get_lists(0) gives the stored rows and nothing else, and so does this pass.
// Determinism: the partition is a function of the edge set, the root of a component is its smallest vertex whatever the order of the
// unions, and everything behind is integer sums and maxima: bit-identical from call to call and engine to engine.
// Buffers: the result (lcc_pop: N words; lcc_plabel, lcc_ppoints, lcc_pnodes, lcc_pfirst: C rows; lcc_lfirst, lcc_llargest: K + 1 and K
// rows) stays until the next call or the next run of the stages (lcc_valid).  Scratch: the sort's 16 B per finite point (ps_*), 8 B per
// finite point of head flags and their scan, 24 B per vertex (+ 4 B flags and 4 B scan per vertex), 8 B per node (nlo | nhi), 8 B per label,
// refine.hip's row chunk.
// Tile contexts: the calls of include/vgs.h refuse them (a tile holds part of the cloud and of the graph), but the pass itself runs over a
// tile's OWN points as step 1 of the parts across the ranks of the tiled driver (vgs_label_parts_on_device with the own point range;
// labelcc_tiles.hip reads the vertex arrays it leaves in lcc_vtx and adds the band, the cross links and the global ids).
// Steps 1 and 2 are a function of their own (vgs_label_vertices_on_device): labelgraph.hip builds the adjacency graph of a labelling on
// the same vertex list, in the same scratch.
// (The context's lc_* members belong to the local cut, hence lcc_*.)
#include <string.h>

#include <algorithm>
#include <string>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "unionfind.hpp"

#define LC_TB 256
#define LC_SHORT 64   // rows of at most so many entries share a wavefront
#define LC_NONE 0xffffffffu

// Step 2.  q <= nf: flag[nf] = 0 closes the scan, so that scan[nf] is the number of vertices.
__global__ __launch_bounds__(LC_TB) void k_lc_heads(const uint32_t* __restrict__ key, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ pt_vox,
                                                    int64_t nf, uint32_t K, uint32_t* __restrict__ flag) {
  const int64_t q = (int64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (q > nf) return;
  bool head = false;
  if (q < nf) {
    const uint32_t l = key[q];
    if (l < K) {
      const uint32_t v = pt_vox[pos[q]];
      head = v != LC_NONE && (q == 0 || key[q - 1] != l || pt_vox[pos[q - 1]] != v);
    }
  }
  flag[q] = head ? 1u : 0u;
}

__global__ __launch_bounds__(LC_TB) void k_lc_vertices(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ vex, const uint32_t* __restrict__ key,
                                                       const uint32_t* __restrict__ pos, const uint32_t* __restrict__ pt_vox, int64_t nf, uint32_t nv,
                                                       uint32_t* __restrict__ vnode, uint32_t* __restrict__ vlabel, uint32_t* __restrict__ vq,
                                                       uint32_t* __restrict__ parent, uint32_t* __restrict__ nlo, uint32_t* __restrict__ nhi) {
  const int64_t q = (int64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (q >= nf || !flag[q]) return;
  const uint32_t i = vex[q];
  if (i >= nv) return;   // (nv is the scan's own total: the bound only guards the arrays)
  const uint32_t v = pt_vox[pos[q]];
  vnode[i] = v;
  atomicMin(&nlo[v], i);   // (nlo filled with LC_NONE, nhi with 0: integer extrema, the same whatever the order)
  atomicMax(&nhi[v], i);
  vlabel[i] = key[q];
  vq[i] = (uint32_t)q;
  parent[i] = i;
}

// first vertex of every label (vfirst[K] = nv), and the end of the last vertex's points: the end of the labelled points
__global__ __launch_bounds__(LC_TB) void k_lc_vfirst(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ vex, uint32_t K, uint32_t nv,
                                                     uint32_t* __restrict__ vfirst, uint32_t* __restrict__ vq) {
  const uint64_t k = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (k > (uint64_t)K) return;
  const uint32_t s = seg_start[k];
  vfirst[k] = min(vex[s], nv);
  if (k == (uint64_t)K) vq[nv] = s;
}

// the vertices whose node has no stored row, as a flag (flag[nv] = 0 closes the scan) and behind the scan as a list (vertex, node id)
__global__ __launch_bounds__(LC_TB) void k_lc_unused_flags(const uint32_t* __restrict__ vnode, const uint32_t* __restrict__ used_rank, uint32_t nv,
                                                           uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (i > (uint64_t)nv) return;
  flag[i] = (i < (uint64_t)nv && used_rank[vnode[i]] == LC_NONE) ? 1u : 0u;
}
__global__ __launch_bounds__(LC_TB) void k_lc_unused_list(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ vnode,
                                                          uint32_t nv, uint32_t cap, uint32_t* __restrict__ uv_vtx, uint32_t* __restrict__ uv_node) {
  const uint64_t i = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (i >= (uint64_t)nv || !flag[i]) return;
  const uint32_t o = excl[i];
  if (o < cap) { uv_vtx[o] = (uint32_t)i; uv_node[o] = vnode[i]; }   // (cap = the number of flags: the bound only guards the list)
}

// Step 3.  W lanes per row, 64 / W rows per wavefront.  Item j: vertex items[j] (items == nullptr: vertex j).  used_rank != nullptr: the
// stored rows, row used_rank[node], a vertex of an unused node leaves; nullptr: the rows built for this list, row j.  W = 64 takes the
// rows above LC_SHORT entries, any other W those up to it.
// back: which edges to a LOWER vertex this side unites.  The lanes of a row that all hook the row's own root under different lower
// vertices succeed one per round (the root changes under the others, who find and try again): on the 10 M-point scene the link kernels
// took 27 - 30 ms that way and 17 - 20 ms this way.  An edge whose other row holds it too is therefore left to the lower vertex, whose lanes hook
// DIFFERENT roots under its own.  LC_BACK_NEVER: the other row always has the edge (the stored rows of VGS: a used neighbour's stored
// row keeps used nodes, an unused neighbour's row is built in full, and the predicate is symmetric).  LC_BACK_USED (the rows built for
// unused voxels when the stored rows are pruned): a used neighbour's row has dropped this node, so its edges are united from here; an
// unused neighbour's full row has it.  LC_BACK_ALWAYS: nothing is assumed about the other row (SVGS).
enum { LC_BACK_NEVER = 0, LC_BACK_USED = 1, LC_BACK_ALWAYS = 2 };
// the vertex (l, w), LC_NONE when no point of w carries l: the header says why in this order
__device__ __forceinline__ uint32_t lc_lookup(const uint32_t* __restrict__ vnode, const uint32_t* __restrict__ vlabel, const uint32_t* __restrict__ nlo,
                                              const uint32_t* __restrict__ nhi, uint32_t l, uint32_t w, uint32_t a, uint32_t b) {
  const uint32_t t = nlo[w];
  if (t == LC_NONE) return LC_NONE;   // no labelled point in w
  const uint32_t lt = vlabel[t];
  if (lt >= l) return lt == l ? t : LC_NONE;
  const uint32_t u = nhi[w];
  if (u == t) return LC_NONE;
  const uint32_t lu = vlabel[u];
  if (lu <= l) return lu == l ? u : LC_NONE;
  uint32_t lo = a, hi = b;   // label l's vertices are sorted by node
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (vnode[mid] < w) lo = mid + 1; else hi = mid; }
  return (lo < b && vnode[lo] == w) ? lo : LC_NONE;
}

template <int W>
__device__ __forceinline__ void lc_link_body(const uint32_t* __restrict__ items, uint32_t n_items, const uint32_t* __restrict__ vnode,
                                             const uint32_t* __restrict__ vlabel, const uint32_t* __restrict__ vfirst,
                                             const uint32_t* __restrict__ nlo, const uint32_t* __restrict__ nhi,
                                             const uint32_t* __restrict__ used_rank, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                             int stride, int back, const uint32_t* __restrict__ rank_of, uint32_t* __restrict__ parent) {
  const uint32_t j = blockIdx.x * (64 / W) + threadIdx.x / W;
  const uint32_t sub = threadIdx.x % W;
  if (j >= n_items) return;   // (whole row groups; no barrier follows)
  const uint32_t i = items ? items[j] : j;
  const uint32_t v = vnode[i];
  uint32_t r = j;
  if (used_rank) { r = used_rank[v]; if (r == LC_NONE) return; }
  const uint32_t m = min(cnt[r], (uint32_t)stride);
  if ((W == 64) != (m > LC_SHORT)) return;
  const uint32_t l = vlabel[i];
  const uint32_t a = vfirst[l], b = vfirst[l + 1];
  const uint64_t* row = rows + (size_t)r * stride;
  // equal parents mean one tree, whatever other wavefronts do meanwhile (links are only ever added): one load instead of two finds
  const uint32_t pi = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint32_t k = sub; k < m; k += W) {
    const uint32_t w = (uint32_t)row[k];
    if (w == v) continue;   // (a stored row starts with its own node)
    const uint32_t lo = lc_lookup(vnode, vlabel, nlo, nhi, l, w, a, b);
    if (lo == LC_NONE) continue;
    if (lo < i && (back == LC_BACK_NEVER || (back == LC_BACK_USED && rank_of[w] == LC_NONE))) continue;
    if (__hip_atomic_load(&parent[lo], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pi) continue;
    uf_union(parent, i, lo);
  }
}

__global__ __launch_bounds__(64) void k_lc_link_short(const uint32_t* __restrict__ items, uint32_t n_items, const uint32_t* __restrict__ vnode,
                                                      const uint32_t* __restrict__ vlabel, const uint32_t* __restrict__ vfirst,
                                                      const uint32_t* __restrict__ nlo, const uint32_t* __restrict__ nhi,
                                                      const uint32_t* __restrict__ used_rank, const uint64_t* __restrict__ rows,
                                                      const uint32_t* __restrict__ cnt, int stride, int back,
                                                      const uint32_t* __restrict__ rank_of, uint32_t* __restrict__ parent) {
  lc_link_body<8>(items, n_items, vnode, vlabel, vfirst, nlo, nhi, used_rank, rows, cnt, stride, back, rank_of, parent);
}
__global__ __launch_bounds__(64) void k_lc_link_long(const uint32_t* __restrict__ items, uint32_t n_items, const uint32_t* __restrict__ vnode,
                                                     const uint32_t* __restrict__ vlabel, const uint32_t* __restrict__ vfirst,
                                                     const uint32_t* __restrict__ nlo, const uint32_t* __restrict__ nhi,
                                                     const uint32_t* __restrict__ used_rank, const uint64_t* __restrict__ rows,
                                                     const uint32_t* __restrict__ cnt, int stride, int back,
                                                     const uint32_t* __restrict__ rank_of, uint32_t* __restrict__ parent) {
  lc_link_body<64>(items, n_items, vnode, vlabel, vfirst, nlo, nhi, used_rank, rows, cnt, stride, back, rank_of, parent);
}

// Step 4.  Pointer jumping between the passes: every later find starts one hop from a root.
__global__ __launch_bounds__(LC_TB) void k_lc_compress(uint32_t* __restrict__ parent, uint32_t nv) {
  const uint64_t i = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (i >= (uint64_t)nv) return;
  const uint32_t r = uf_find(parent, (uint32_t)i);
  if (r != (uint32_t)i) __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the unions are complete: read-only walks, the roots into an array of their own (flag[nv] = 0 closes the scan)
__global__ __launch_bounds__(LC_TB) void k_lc_roots(const uint32_t* __restrict__ parent, uint32_t nv, uint32_t* __restrict__ vroot, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (i > (uint64_t)nv) return;
  if (i == (uint64_t)nv) { flag[i] = 0u; return; }
  const uint32_t r = uf_root(parent, (uint32_t)i);
  vroot[i] = r;
  flag[i] = r == (uint32_t)i ? 1u : 0u;
}

// Step 5.  A wavefront whose vertices all lie in one part (the common case inside a large part) adds once; integer sums either way.
__global__ __launch_bounds__(LC_TB) void k_lc_parts(const uint32_t* __restrict__ vroot, const uint32_t* __restrict__ rex, const uint32_t* __restrict__ vnode,
                                                    const uint32_t* __restrict__ vlabel, const uint32_t* __restrict__ vq, uint32_t nv, uint32_t C,
                                                    uint32_t* __restrict__ vpart, int32_t* __restrict__ p_label, unsigned long long* __restrict__ p_points,
                                                    uint32_t* __restrict__ p_nodes, int32_t* __restrict__ p_first) {
  const uint64_t i64 = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  const bool in = i64 < (uint64_t)nv;
  const unsigned long long live = __ballot(in);
  if (live == 0ull) return;   // (whole wavefronts; no barrier follows)
  const uint32_t i = (uint32_t)i64;
  uint32_t p = 0, one = 0;
  unsigned long long npts = 0;
  if (in) {
    const uint32_t r = vroot[i];
    p = min(rex[r], C - 1);   // (C is the scan's own total: the bound only guards the rows)
    vpart[i] = p;
    npts = (unsigned long long)(vq[i + 1] - vq[i]);
    one = 1;
    if (r == i) { p_label[p] = (int32_t)vlabel[i]; p_first[p] = (int32_t)vnode[i]; }
  }
  const int first = __ffsll((long long)live) - 1;
  const uint32_t pf = __shfl(p, first, 64);
  if (__ballot(in && p != pf) == 0ull) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { npts += __shfl_xor(npts, m, 64); one += __shfl_xor(one, m, 64); }
    if ((int)(threadIdx.x & 63) == first) { atomicAdd(&p_points[pf], npts); atomicAdd(&p_nodes[pf], one); }
  } else if (in) {
    atomicAdd(&p_points[p], npts);
    atomicAdd(&p_nodes[p], 1u);
  }
}

__global__ __launch_bounds__(LC_TB) void k_lc_label_first(const uint32_t* __restrict__ vfirst, const uint32_t* __restrict__ rex, uint32_t K,
                                                          int64_t* __restrict__ l_first) {
  const uint64_t k = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (k <= (uint64_t)K) l_first[k] = (int64_t)rex[vfirst[k]];   // (rex[nv] = C)
}
// most points first, the lowest part id on a tie: the maximum of points << 32 | ~part (a part holds a point, so the key is not 0)
__global__ __launch_bounds__(LC_TB) void k_lc_largest_fold(const int32_t* __restrict__ p_label, const unsigned long long* __restrict__ p_points, uint32_t C,
                                                           uint32_t K, unsigned long long* __restrict__ lmax) {
  const uint64_t p = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (p >= (uint64_t)C) return;
  const uint32_t l = (uint32_t)p_label[p];
  if (l < K) atomicMax(&lmax[l], (p_points[p] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)p));
}
__global__ __launch_bounds__(LC_TB) void k_lc_largest(const unsigned long long* __restrict__ lmax, uint32_t K, int32_t* __restrict__ l_largest) {
  const uint64_t k = (uint64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (k >= (uint64_t)K) return;
  const unsigned long long m = lmax[k];
  l_largest[k] = m == 0ull ? -1 : (int32_t)(0xffffffffu - (uint32_t)m);
}

__global__ __launch_bounds__(LC_TB) void k_lc_scatter(const uint32_t* __restrict__ vex, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ perm,
                                                      const uint32_t* __restrict__ vpart, const uint32_t* __restrict__ vq, uint32_t nv,
                                                      int32_t* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * LC_TB + threadIdx.x;
  if (q >= (int64_t)vq[nv]) return;   // the labelled points are the front of the sorted order
  const uint32_t i = vex[q + 1] - 1u;   // inclusive scan of the head flags - 1
  if (i < nv) out[perm[pos[q]]] = (int32_t)vpart[i];   // (every labelled point has a head at or in front of it; the bound only guards the array)
}

// ---------------------------------------------------------------------------------------------------------------------- host
static unsigned lc_grid(uint64_t n) { return (unsigned)((n + LC_TB - 1) / LC_TB); }

// exclusive scan of n words on the context's stream, rocprim's storage in ps_tmp
static vgs_status lc_scan(vgs_ctx* c, uint32_t* in, uint32_t* out, size_t n) {
  size_t bytes = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, c->ps_tmp.ensure(bytes));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->ps_tmp.p, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
  return VGS_OK;
}

// both link kernels over one list of n items (items == nullptr: all vertices against the stored rows)
static vgs_status lc_link(vgs_ctx* c, const LcVtx& X, const uint32_t* items, uint32_t n, const uint32_t* used_rank, const uint64_t* rows,
                          const uint32_t* cnt, int back) {
  if (n == 0) return VGS_OK;
  hipLaunchKernelGGL(k_lc_link_short, dim3((n + 7) / 8), dim3(64), 0, c->stream, items, n, X.node, X.label, c->lcc_vfirst.p, c->lcc_nidx.p,
                     c->lcc_nidx.p + c->V, used_rank, rows, cnt, c->adj_stride, back, c->used_rank.p, X.parent);
  hipLaunchKernelGGL(k_lc_link_long, dim3(n), dim3(64), 0, c->stream, items, n, X.node, X.label, c->lcc_vfirst.p, c->lcc_nidx.p, c->lcc_nidx.p + c->V,
                     used_rank, rows, cnt, c->adj_stride, back, c->used_rank.p, X.parent);
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}

static vgs_status lc_check(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t n, int64_t K) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of the cloud and of its neighbourhood graph; the connected parts of a labelling across the ranks of the tiled driver are not computed";
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

// Steps 1 and 2 for this pass and for labelgraph.hip: the sort (S; n_skipped as ps_sort_points counts it), the vertices in (label, node)
// order (nv of them, X: six arrays of nv + 1 words in lcc_vtx, of which node, label, q and parent = itself are written), nlo | nhi in
// lcc_nidx and the first vertex of every label in lcc_vfirst, all left on the context's stream.  nv = 0: nothing behind the sort is built.
vgs_status vgs_label_vertices_on_device(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t own_first, int64_t n_lab, int64_t K,
                                        int64_t* n_skipped, PsSort& S, uint32_t* n_vertices, LcVtx& X) {
  const int64_t nf = c->Nf, V = c->V;
  const size_t k = (size_t)K;
  *n_vertices = 0;
  X = LcVtx{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  vgs_status s = ps_sort_points(c, fn, labels_dev, own_first, n_lab, K, 0, n_skipped, S);
  if (s != VGS_OK) return s;
  uint32_t nv = 0;
  if (S.sorted && nf > 0 && V > 0) {
    VGS_HIP_TRY(c, c->lcc_flag.ensure((size_t)nf + 1)); VGS_HIP_TRY(c, c->lcc_vex.ensure((size_t)nf + 1));
    hipLaunchKernelGGL(k_lc_heads, dim3(lc_grid((uint64_t)nf + 1)), dim3(LC_TB), 0, c->stream, S.key, S.pos, c->pt_vox.p, nf, (uint32_t)K, c->lcc_flag.p);
    if ((s = lc_scan(c, c->lcc_flag.p, c->lcc_vex.p, (size_t)nf + 1)) != VGS_OK) return s;
    VGS_READBACK(c, &nv, c->lcc_vex.p + nf, 4);
  }
  if (nv == 0) return VGS_OK;
  const size_t w = (size_t)nv + 1;
  VGS_HIP_TRY(c, c->lcc_vtx.ensure(6 * w)); VGS_HIP_TRY(c, c->lcc_vfirst.ensure(k + 1)); VGS_HIP_TRY(c, c->lcc_vscan.ensure(w));
  X.node = c->lcc_vtx.p; X.label = X.node + w; X.q = X.label + w; X.parent = X.q + w; X.root = X.parent + w; X.part = X.root + w;
  VGS_HIP_TRY(c, c->lcc_nidx.ensure(2 * (size_t)V));   // nlo | nhi
  VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_nidx.p, 0xff, (size_t)V * sizeof(uint32_t), c->stream));
  VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_nidx.p + V, 0, (size_t)V * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_lc_vertices, dim3(lc_grid((uint64_t)nf)), dim3(LC_TB), 0, c->stream, c->lcc_flag.p, c->lcc_vex.p, S.key, S.pos, c->pt_vox.p, nf, nv,
                     X.node, X.label, X.q, X.parent, c->lcc_nidx.p, c->lcc_nidx.p + V);
  hipLaunchKernelGGL(k_lc_vfirst, dim3(lc_grid(k + 1)), dim3(LC_TB), 0, c->stream, S.seg_start, c->lcc_vex.p, (uint32_t)K, nv, c->lcc_vfirst.p, X.q);
  VGS_HIP_TRY(c, hipGetLastError());
  *n_vertices = nv;
  return VGS_OK;
}

// The pass over labels_dev: n_lab entries for the input indices own_first .. own_first + n_lab - 1 (one context: 0 and N; a tile context, for
// labelcc_tiles.hip: its own point range -- k_ps_keys gives every other position the key K, so the vertices are those of own points only).
// The vertex arrays stay in lcc_vtx (lcc_nv vertices, six arrays of lcc_nv + 1 words: LcVtx) until the next call.
vgs_status vgs_label_parts_on_device(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t own_first, int64_t n_lab, int64_t K, int64_t* n_parts,
                                     int64_t* n_skipped) {
  const int64_t N = c->N, nf = c->Nf, V = c->V, U = c->U;
  const size_t k = (size_t)K;
  c->lcc_valid = false; c->lcc_nv = 0; c->lct_own = c->lct_linked = c->lct_applied = false; c->lgt_own = c->lgt_valid = false;
  VGS_HIP_TRY(c, c->lcc_pop.ensure(N > 0 ? (size_t)N : 1)); VGS_HIP_TRY(c, c->lcc_lfirst.ensure(k + 1)); VGS_HIP_TRY(c, c->lcc_llargest.ensure(k + 1));
  PsSort S;
  LcVtx X;
  uint32_t nv = 0, C = 0;
  vgs_status s = vgs_label_vertices_on_device(c, fn, labels_dev, own_first, n_lab, K, n_skipped, S, &nv, X);
  if (s != VGS_OK) return s;
  if (N > 0) VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_pop.p, 0xff, (size_t)N * sizeof(int32_t), c->stream));
  if (nv > 0) {
    const size_t w = (size_t)nv + 1;
    // the stored rows: every vertex of a used node
    const bool vgs = c->P.method == 2;
    if (U > 0 && (s = lc_link(c, X, nullptr, nv, c->used_rank.p, c->adj_key.p, c->adj_cnt.p, vgs ? LC_BACK_NEVER : LC_BACK_ALWAYS)) != VGS_OK) return s;
    // VGS: the vertices of unused voxels, their rows built in full a chunk at a time (the head flags are spent: lcc_flag takes these)
    if (vgs && V - U > 0) {
      uint32_t n_un = 0;
      hipLaunchKernelGGL(k_lc_unused_flags, dim3(lc_grid(w)), dim3(LC_TB), 0, c->stream, X.node, c->used_rank.p, nv, c->lcc_flag.p);
      if ((s = lc_scan(c, c->lcc_flag.p, c->lcc_vscan.p, w)) != VGS_OK) return s;
      VGS_READBACK(c, &n_un, c->lcc_vscan.p + nv, 4);
      if (n_un > 0) {
        VGS_HIP_TRY(c, c->lcc_uv.ensure(2 * (size_t)n_un));
        uint32_t *uv_vtx = c->lcc_uv.p, *uv_node = uv_vtx + n_un;
        hipLaunchKernelGGL(k_lc_unused_list, dim3(lc_grid(nv)), dim3(LC_TB), 0, c->stream, c->lcc_flag.p, c->lcc_vscan.p, X.node, nv, n_un, uv_vtx, uv_node);
        VGS_HIP_TRY(c, hipGetLastError());
        const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_un, ((int64_t)32 << 20) / std::max(1, c->adj_stride)));   // at most 256 MB of keys
        VGS_HIP_TRY(c, c->rf_rows.ensure((size_t)chunk * c->adj_stride)); VGS_HIP_TRY(c, c->rf_cnt.ensure((size_t)chunk)); VGS_HIP_TRY(c, c->rf_nall.ensure((size_t)chunk));
        for (int64_t o = 0; o < (int64_t)n_un; o += chunk) {
          const int64_t m = std::min(chunk, (int64_t)n_un - o);
          hipLaunchKernelGGL(k_lc_compress, dim3(lc_grid(nv)), dim3(LC_TB), 0, c->stream, X.parent, nv);
          if ((s = vgs_run_adjacency(c, true, c->rf_rows.p, c->rf_cnt.p, c->rf_nall.p, c->adj_r2, uv_node + o, m)) != VGS_OK) return s;
          if ((s = lc_link(c, X, uv_vtx + o, (uint32_t)m, nullptr, c->rf_rows.p, c->rf_cnt.p, c->adj_pruned ? LC_BACK_USED : LC_BACK_NEVER)) != VGS_OK) return s;
        }
      }
    }
    hipLaunchKernelGGL(k_lc_compress, dim3(lc_grid(nv)), dim3(LC_TB), 0, c->stream, X.parent, nv);
    hipLaunchKernelGGL(k_lc_roots, dim3(lc_grid(w)), dim3(LC_TB), 0, c->stream, X.parent, nv, X.root, c->lcc_flag.p);
    if ((s = lc_scan(c, c->lcc_flag.p, c->lcc_vscan.p, w)) != VGS_OK) return s;
    VGS_READBACK(c, &C, c->lcc_vscan.p + nv, 4);
    VGS_HIP_TRY(c, c->lcc_plabel.ensure(C)); VGS_HIP_TRY(c, c->lcc_ppoints.ensure(C)); VGS_HIP_TRY(c, c->lcc_pnodes.ensure(C));
    VGS_HIP_TRY(c, c->lcc_pfirst.ensure(C)); VGS_HIP_TRY(c, c->lcc_lmax.ensure(k));
    VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_ppoints.p, 0, (size_t)C * sizeof(int64_t), c->stream));
    VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_pnodes.p, 0, (size_t)C * sizeof(int32_t), c->stream));
    VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_lmax.p, 0, k * sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_lc_parts, dim3(lc_grid(nv)), dim3(LC_TB), 0, c->stream, X.root, c->lcc_vscan.p, X.node, X.label, X.q, nv, C, X.part, c->lcc_plabel.p,
                       (unsigned long long*)c->lcc_ppoints.p, (uint32_t*)c->lcc_pnodes.p, c->lcc_pfirst.p);
    hipLaunchKernelGGL(k_lc_label_first, dim3(lc_grid(k + 1)), dim3(LC_TB), 0, c->stream, c->lcc_vfirst.p, c->lcc_vscan.p, (uint32_t)K, c->lcc_lfirst.p);
    hipLaunchKernelGGL(k_lc_largest_fold, dim3(lc_grid(C)), dim3(LC_TB), 0, c->stream, c->lcc_plabel.p, (const unsigned long long*)c->lcc_ppoints.p, C,
                       (uint32_t)K, (unsigned long long*)c->lcc_lmax.p);
    hipLaunchKernelGGL(k_lc_largest, dim3(lc_grid(k)), dim3(LC_TB), 0, c->stream, (const unsigned long long*)c->lcc_lmax.p, (uint32_t)K, c->lcc_llargest.p);
    hipLaunchKernelGGL(k_lc_scatter, dim3(lc_grid((uint64_t)nf)), dim3(LC_TB), 0, c->stream, c->lcc_vex.p, S.pos, c->perm_b.p, X.part, X.q, nv, c->lcc_pop.p);
    VGS_HIP_TRY(c, hipGetLastError());
  } else {
    // no vertex (no point, no finite point, no node, K = 0, all labels negative): no part, every label empty
    VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_lfirst.p, 0, (k + 1) * sizeof(int64_t), c->stream));
    if (k > 0) VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_llargest.p, 0xff, k * sizeof(int32_t), c->stream));
  }
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the tables are complete, and a labelling read in place is the caller's again
  c->lcc_C = (int64_t)C; c->lcc_K = K; c->lcc_nv = nv; c->lcc_valid = true;
  if (n_parts) *n_parts = (int64_t)C;
  return VGS_OK;
}

static vgs_status lc_components(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t n, int64_t K, int64_t* n_parts,
                                int64_t* n_skipped) {
  if (!c) return VGS_E_ARG;
  if (n_parts) *n_parts = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = lc_check(c, fn, labels, n, K);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  c->lcc_valid = false;
  if (!on_device && (s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK) return s;
  return vgs_label_parts_on_device(c, fn, labels, 0, c->N, K, n_parts, n_skipped);
}

extern "C" vgs_status vgs_point_label_components(vgs_ctx* c, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_skipped) {
  return lc_components(c, "vgs_point_label_components", labels_host, false, n, K, n_parts, n_skipped);
}

extern "C" vgs_status vgs_point_label_components_device(vgs_ctx* c, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_parts,
                                                        int64_t* n_skipped) {
  return lc_components(c, "vgs_point_label_components_device", labels_dev, true, n, K, n_parts, n_skipped);
}

static vgs_status lc_result(vgs_ctx* c, const char* fn) {
  if (!c) return VGS_E_ARG;
  if (c->stage < ST_SEGMENTED || !c->lcc_valid) {
    c->err = std::string(fn) + ": no label components since the last run of the stages (vgs_point_label_components first)";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

#define LC_COPY(dst, src, count) \
  if ((dst) && (count) > 0) VGS_HIP_TRY(c, hipMemcpy((dst), (src), (size_t)(count) * sizeof(*(dst)), hipMemcpyDeviceToHost))

extern "C" vgs_status vgs_get_point_label_components(vgs_ctx* c, int32_t* part_of_point, int32_t* part_label, int64_t* part_points, int32_t* part_nodes,
                                                     int32_t* part_first_node, int64_t* label_first, int32_t* label_largest) {
  vgs_status s = lc_result(c, "vgs_get_point_label_components");
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  LC_COPY(part_of_point, c->lcc_pop.p, c->N);
  LC_COPY(part_label, c->lcc_plabel.p, c->lcc_C); LC_COPY(part_points, c->lcc_ppoints.p, c->lcc_C); LC_COPY(part_nodes, c->lcc_pnodes.p, c->lcc_C);
  LC_COPY(part_first_node, c->lcc_pfirst.p, c->lcc_C);
  LC_COPY(label_first, c->lcc_lfirst.p, c->lcc_K + 1); LC_COPY(label_largest, c->lcc_llargest.p, c->lcc_K);
  return VGS_OK;
}

extern "C" vgs_status vgs_get_point_label_components_device(vgs_ctx* c, const int32_t** part_of_point, const int32_t** part_label,
                                                            const int64_t** part_points, const int32_t** part_nodes, const int32_t** part_first_node,
                                                            const int64_t** label_first, const int32_t** label_largest) {
  vgs_status s = lc_result(c, "vgs_get_point_label_components_device");
  if (s != VGS_OK) return s;
  const bool rows = c->lcc_C > 0;
  if (part_of_point) *part_of_point = c->N > 0 ? c->lcc_pop.p : nullptr;
  if (part_label) *part_label = rows ? c->lcc_plabel.p : nullptr;
  if (part_points) *part_points = rows ? c->lcc_ppoints.p : nullptr;
  if (part_nodes) *part_nodes = rows ? c->lcc_pnodes.p : nullptr;
  if (part_first_node) *part_first_node = rows ? c->lcc_pfirst.p : nullptr;
  if (label_first) *label_first = c->lcc_lfirst.p;
  if (label_largest) *label_largest = c->lcc_K > 0 ? c->lcc_llargest.p : nullptr;
  return VGS_OK;
}
