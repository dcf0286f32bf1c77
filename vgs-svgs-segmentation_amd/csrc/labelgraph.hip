// labelgraph.hip -- the adjacency graph of a per-POINT labelling of the context's cloud that the CALLER supplies (include/vgs.h:
// vgs_point_label_graph; no reference counterpart).  seggraph.hip describes labels that are constant on a node; this pass describes any
// labelling: which labels touch, across how many node pairs, how strongly the local cut's weight links them, and how many nodes they share.
//
// Definition (include/vgs.h states it in full).  Nodes, vertices (label, node) and rows are those of labelcc.hip.  A contact of labels
// a < b is an unordered pair of vertices {(a, v), (b, w)}, v != w, with w in the row of v or v in the row of w; a shared node of a, b
// carries both.  Edge {a < b}: at least one contact or one shared node.
//
// Data flow:
//   1. labelcc.hip's steps 1 and 2 (vgs_label_vertices_on_device): the point sort and the vertices in (label, node) order
//   2. one stable radix sort of the vertex list by node, nv keys: position t of the sorted list is vertex (slab[t], snode[t]), and the
//      labels of node x are the ascending run slab[nbeg[x] .. nend[x]) (k_lg_node_runs)
//   3. k_lg_rows<false>: one wavefront per vertex (A, u) = position t walks u's row -- the stored row by used rank, or for VGS the row of an
//      unused voxel, built with every neighbour a chunk at a time by vgs_run_adjacency in refine.hip's row scratch (k_lg_unused_flags, scan,
//      k_lg_unused_list give the distinct unused nodes and every vertex its row) -- and counts its records; exclusive scan -> first record
//      k_lg_rows<true>: the same walk writes them.  Per distinct other label B, ascending, ONE record (A, B, contacts counted from this
//      side, n_finite, w_sum, w_min, w_max, flags): B is found among the neighbours' labels (two dependent loads per entry, nbeg / nend
//      then slab, and a binary search inside a node with many labels) and among u's own other labels (LG_SHARED).  The walk is
//      k_sg_rows': fold the label found by the previous walk, find the next larger one by a wave-wide min; no per-entry state, rows of
//      any length up to adj_stride in chunks of 64 entries.
//   4. - 6. seggraph.hip's pipeline restated over these records: stable radix sort by min * K + max, heads, starts, chunk partials of
//      LG_CHUNK records, final fold (k_lg_heads, k_lg_starts, k_lg_nchunk, k_lg_chunks, k_lg_final).
//
// The walk itself is labelgraph_walk.hpp's lg_walk_body, which labelgraph_tiles.hip's kernel calls in tile mode; step 2 and steps 3 to 6
// are host functions of their own (vgs_lg_vertices_by_node, vgs_lg_table_from_walk) that the tile context runs with its walk in place of
// the plain one.
//
// Every contact is counted once.  Let R(x) be the row this pass reads for node x and "x holds y" mean y in R(x); {v, w} is adjacent when
// v holds w or w holds v.  Both endpoints of a contact carry a vertex, so both rows are walked.  The walker of u, at entry x, counts the
// contact when  u < x  or  x does not hold u.  If both rows hold the pair only the lower id has u < x; if only one row holds it, that
// row's walker counts it whichever id is lower (lower: first clause; higher: second) and the other row never sees it.  So: exactly once.
// Whether x holds u (LG_HOLDS_*):
//   ALWAYS  VGS stored rows, and the built rows when the stored rows are not pruned: a used neighbour's stored row keeps every node this
//           walker can be (used nodes if pruned, all otherwise), an unused neighbour's row is built in full, the predicate is symmetric
//   UNUSED  the rows built for unused voxels when the stored rows are pruned (adj_pruned): a used x has dropped u, an unused x holds it
//   SEARCH  SVGS: nothing is assumed; x's stored row is searched (sg_in_row), a node without a stored row holds nothing
// which gives the four cases of the issue: two used nodes from the lower id; pruned rows and one unused endpoint from the unused
// endpoint's full row; two unused nodes from the lower id; SVGS from the lower id when its row holds the pair, else from the other row.
// nodes_ab counts the vertices that are in a contact, counted or not.  A vertex sees its contacts in its own row (LG_CONTACT on its
// record) except those whose other endpoint alone holds the pair: for each of them the walker that counts it writes a PROXY record for
// the other vertex (a = that vertex's label, t = its position, no counts).  The fold counts a vertex once per edge: the records of an
// edge are in ascending t, a vertex's records adjacent, and the first of them counts the vertex when it has LG_CONTACT or a successor
// (a vertex writes one record per edge itself, so a second one is a proxy).  Without proxies the records leave step 3 in ascending t
// already; with them (counted in step 3, lg_meta[2]) one more stable sort by t runs in front of the sort by edge.
// A shared node gives a record with LG_SHARED from each of its two vertices; the fold counts the one whose own label is the lower.
// Determinism: integer fields and extrema are functions of the contact set.  w_sum: a record's sum is folded by the lane that reads the
// entry (row chunk, lane) and the fixed xor butterfly; an edge's records are folded in ascending (node, label) -- t -- in chunks of
// LG_CHUNK, lane stride then butterfly, the partials the same way.  No float atomics (one integer atomicAdd counts the proxies).
// With one label per node on used kept nodes the records are seggraph.hip's in its order and the fold has its shape: the table is
// vgs_get_segment_graph's, w_sum included.
// Buffers: the result (lg_ab, lg_nshared, lg_npairs, lg_nfin, lg_nodes, lg_wsum, lg_wmin, lg_wmax: E rows) stays until the next call or
// the next run of the stages (lg_valid).  Scratch: labelcc.hip's for steps 1 and 2 (16 B per finite point of sort, 8 B of head flags and
// scan, 24 B per vertex, 8 B per node, 8 B per label) -- the arrays parent | root | part of lcc_vtx hold the sort by node, lcc_nidx the
// node runs, lcc_flag / lcc_vscan / lcc_uv the unused list -- plus 12 B per vertex (record count and first record) and per record 40 B
// (LgRec) + 16 B keys + 8 B indices + 8 B keys by vertex + 16 B edge work, 48 B per chunk partial; refine.hip's row chunk.
#include <climits>
#include <cmath>
#include <string.h>

#include <algorithm>
#include <string>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "wavefold.hpp"
#include "labelgraph_walk.hpp"   // LG_WAVES, LG_NONE, the record flags, LG_HOLDS_*, lg_lower and the walk itself

#define LG_TB 256
#define LG_PPL 4                   // records per lane of a chunk
#define LG_CHUNK (64 * LG_PPL)     // records per chunk (seggraph.hip's SG_CHUNK: the same fold shape)

// Step 2.  iota for the sort's values; behind the sort the label of every position and the run of every node
__global__ __launch_bounds__(LG_TB) void k_lg_iota(uint32_t nv, uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * LG_TB + threadIdx.x;
  if (i < (uint64_t)nv) out[i] = (uint32_t)i;
}
__global__ __launch_bounds__(LG_TB) void k_lg_node_runs(const uint32_t* __restrict__ snode, const uint32_t* __restrict__ sperm, const uint32_t* __restrict__ vlabel,
                                                        uint32_t nv, uint32_t* __restrict__ slab, uint32_t* __restrict__ nbeg, uint32_t* __restrict__ nend) {
  const uint64_t t = (uint64_t)blockIdx.x * LG_TB + threadIdx.x;
  if (t >= (uint64_t)nv) return;
  const uint32_t v = snode[t];
  slab[t] = vlabel[sperm[t]];
  if (t == 0 || snode[t - 1] != v) nbeg[v] = (uint32_t)t;           // (nbeg = nend = 0 for a node without a vertex)
  if (t + 1 == (uint64_t)nv || snode[t + 1] != v) nend[v] = (uint32_t)t + 1u;
}

// the distinct nodes without a stored row: flag of the first position of such a node (flag[nv] = 0 closes the scan); behind the scan the
// list of their ids and, for every position, the row of its node in that list (LG_NONE: the node has a stored row)
__global__ __launch_bounds__(LG_TB) void k_lg_unused_flags(const uint32_t* __restrict__ snode, const uint32_t* __restrict__ used_rank, uint32_t nv,
                                                           uint32_t* __restrict__ flag) {
  const uint64_t t = (uint64_t)blockIdx.x * LG_TB + threadIdx.x;
  if (t > (uint64_t)nv) return;
  flag[t] = (t < (uint64_t)nv && used_rank[snode[t]] == LG_NONE && (t == 0 || snode[t - 1] != snode[t])) ? 1u : 0u;
}
__global__ __launch_bounds__(LG_TB) void k_lg_unused_list(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ snode,
                                                          const uint32_t* __restrict__ used_rank, uint32_t nv, uint32_t cap, uint32_t* __restrict__ un_node,
                                                          uint32_t* __restrict__ urow) {
  const uint64_t t = (uint64_t)blockIdx.x * LG_TB + threadIdx.x;
  if (t >= (uint64_t)nv) return;
  const uint32_t v = snode[t];
  if (used_rank[v] != LG_NONE) { urow[t] = LG_NONE; return; }
  const uint32_t o = excl[t] + flag[t] - 1u;   // the node's head is at or in front of t
  urow[t] = o;
  if (flag[t] && o < cap) un_node[o] = v;      // (cap = the number of flags: the bound only guards the list)
}

// Step 3.  One wavefront per position t = vertex (A, u).  urow == nullptr: the stored rows (a node without one has an empty row if
// no_row_is_empty -- SVGS -- and leaves otherwise); urow != nullptr: the rows built for the unused nodes row0 .. row0 + n_rows - 1 of the
// list, every other vertex leaves.  WRITE = false: n_rec[t] = its records, and the proxies among them are added to meta[2]; WRITE =
// true: the records at rec_off[t] ...  The file header has the counting rule and what a proxy is; the walk is labelgraph_walk.hpp's.
template <bool WRITE>
__global__ __launch_bounds__(64 * LG_WAVES) void k_lg_rows(uint32_t nv, const uint32_t* __restrict__ snode, const uint32_t* __restrict__ slab,
                                                           const uint32_t* __restrict__ nbeg, const uint32_t* __restrict__ nend,
                                                           const uint32_t* __restrict__ used_rank, const uint64_t* __restrict__ adj_key,
                                                           const uint32_t* __restrict__ adj_cnt, int adj_stride, const uint32_t* __restrict__ urow,
                                                           uint32_t row0, uint32_t n_rows, const uint64_t* __restrict__ rows,
                                                           const uint32_t* __restrict__ rows_cnt, int no_row_is_empty, int holds,
                                                           const NodeRec* __restrict__ node, VgsWeightParams W, uint32_t K, uint32_t R,
                                                           uint32_t* __restrict__ n_rec, const uint64_t* __restrict__ rec_off, LgRec* __restrict__ rec,
                                                           uint64_t* __restrict__ rkey, uint32_t* __restrict__ tkey, uint32_t* __restrict__ ridx,
                                                           uint32_t* __restrict__ meta) {
  lg_walk_body<WRITE, false>(nv, snode, slab, nbeg, nend, used_rank, adj_key, adj_cnt, adj_stride, urow, row0, n_rows, rows, rows_cnt, no_row_is_empty, holds, node,
                             W, K, R, n_rec, rec_off, rec, rkey, tkey, ridx, meta, nullptr);
}

// with proxies: the edge keys in the order of the sort by vertex
__global__ __launch_bounds__(LG_TB) void k_lg_gather_keys(const uint64_t* __restrict__ rkey, const uint32_t* __restrict__ idx, uint32_t R, uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * LG_TB + threadIdx.x;
  if (i < R) out[i] = rkey[idx[i]];
}

// Steps 5 and 6: seggraph.hip's, over LgRec.  head[i] = 1 where sorted record i starts an edge
__global__ __launch_bounds__(LG_TB) void k_lg_heads(const uint64_t* __restrict__ key, uint32_t R, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * LG_TB + threadIdx.x;
  if (i >= R) return;
  head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
// inc = inclusive scan of head: estart[edge] = its first sorted record, estart[E] = R; meta[1] = E
__global__ __launch_bounds__(LG_TB) void k_lg_starts(const uint32_t* __restrict__ head, const uint32_t* __restrict__ inc, uint32_t R, uint32_t* __restrict__ estart,
                                                     uint32_t* __restrict__ meta) {
  const uint32_t i = blockIdx.x * LG_TB + threadIdx.x;
  if (i >= R) return;
  if (head[i]) estart[inc[i] - 1] = i;
  if (i == R - 1) { estart[inc[i]] = R; meta[1] = inc[i]; }
}
// chunks of edge e (nch[E] = 0 closes the scan)
__global__ __launch_bounds__(LG_TB) void k_lg_nchunk(const uint32_t* __restrict__ estart, uint32_t E, uint32_t* __restrict__ nch) {
  const uint32_t e = blockIdx.x * LG_TB + threadIdx.x;
  if (e > E) return;
  nch[e] = e == E ? 0u : (estart[e + 1] - estart[e] + LG_CHUNK - 1) / LG_CHUNK;
}

// One wavefront per chunk of <= LG_CHUNK sorted records of one edge [a, b) inside the edge's records [ea, eb).  Grid: an upper bound of the
// chunks; wavefronts past the real number leave at once.  A vertex is counted at the first of its records (the header says when).
__global__ __launch_bounds__(64 * LG_WAVES) void k_lg_chunks(const uint32_t* __restrict__ ridx, const LgRec* __restrict__ rec,
                                                             const uint32_t* __restrict__ estart, const uint32_t* __restrict__ echunk, uint32_t E,
                                                             LgPart* __restrict__ part) {
  const uint32_t c = blockIdx.x * LG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= echunk[E]) return;
  // edge of chunk c: the last e with echunk[e] <= c (every edge has at least one chunk)
  uint32_t lo = 0, hi = E - 1;
  while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (echunk[mid] <= c) lo = mid; else hi = mid - 1; }
  const uint32_t e = lo;
  const uint32_t ea = estart[e], eb = estart[e + 1];
  const uint32_t a = ea + (c - echunk[e]) * LG_CHUNK;
  const uint32_t b = min(a + LG_CHUNK, eb);
  long long np = 0, nf = 0, ns = 0;
  int na = 0, nb = 0;
  double s = 0.0;
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
#pragma unroll
  for (int it = 0; it < LG_PPL; ++it) {
    const uint32_t i = a + (uint32_t)it * 64 + lane;
    if (i < b) {
      const LgRec q = rec[ridx[i]];
      np += q.cnt; nf += q.n_finite;
      s += q.w_sum; mn = fminf(mn, q.w_min); mx = fmaxf(mx, q.w_max);
      if ((q.flags & LG_SHARED) && q.a < q.b) ++ns;
      if (i == ea || rec[ridx[i - 1]].t != q.t) {
        if ((q.flags & LG_CONTACT) || (i + 1 < eb && rec[ridx[i + 1]].t == q.t)) { if (q.a < q.b) ++na; else ++nb; }
      }
    }
  }
  np = sg_wave_sum(np); nf = sg_wave_sum(nf); ns = sg_wave_sum(ns); na = sg_wave_sum(na); nb = sg_wave_sum(nb);
  s = sg_wave_sum(s); mn = sg_wave_min(mn); mx = sg_wave_max(mx);
  if (lane == 0) {
    LgPart p;
    p.w_sum = s; p.n_pairs = np; p.n_finite = nf; p.n_shared = ns; p.nodes_a = na; p.nodes_b = nb; p.w_min = mn; p.w_max = mx;
    part[c] = p;
  }
}

// one wavefront per edge: fold its partials (lane stride, then butterfly), write the row on lane 0
__global__ __launch_bounds__(64 * LG_WAVES) void k_lg_final(const uint32_t* __restrict__ ridx, const LgRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ estart, const uint32_t* __restrict__ echunk,
                                                            const LgPart* __restrict__ part, uint32_t E, int32_t* __restrict__ o_ab,
                                                            int64_t* __restrict__ o_ns, int64_t* __restrict__ o_np, int64_t* __restrict__ o_nf,
                                                            int32_t* __restrict__ o_nodes, double* __restrict__ o_sum, float* __restrict__ o_min,
                                                            float* __restrict__ o_max) {
  const uint32_t e = blockIdx.x * LG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (e >= E) return;
  long long np = 0, nf = 0, ns = 0;
  int na = 0, nb = 0;
  double s = 0.0;
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
  for (uint32_t c = echunk[e] + lane; c < echunk[e + 1]; c += 64) {
    const LgPart p = part[c];
    np += p.n_pairs; nf += p.n_finite; ns += p.n_shared; na += p.nodes_a; nb += p.nodes_b;
    s += p.w_sum; mn = fminf(mn, p.w_min); mx = fmaxf(mx, p.w_max);
  }
  np = sg_wave_sum(np); nf = sg_wave_sum(nf); ns = sg_wave_sum(ns); na = sg_wave_sum(na); nb = sg_wave_sum(nb);
  s = sg_wave_sum(s); mn = sg_wave_min(mn); mx = sg_wave_max(mx);
  if (lane != 0) return;
  const LgRec q = rec[ridx[estart[e]]];
  o_ab[2 * (size_t)e] = q.a < q.b ? q.a : q.b;
  o_ab[2 * (size_t)e + 1] = q.a < q.b ? q.b : q.a;
  o_ns[e] = ns;
  o_np[e] = np;
  o_nf[e] = nf;
  o_nodes[2 * (size_t)e] = na;
  o_nodes[2 * (size_t)e + 1] = nb;
  o_sum[e] = s;
  o_min[e] = nf > 0 ? mn : __builtin_nanf("");
  o_max[e] = nf > 0 ? mx : __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------------------------------------- host
static unsigned lg_grid(uint64_t n) { return (unsigned)((n + LG_TB - 1) / LG_TB); }

static VgsWeightParams lg_weight_params(const vgs_params& p) {   // (seggraph.hip: sg_weight_params, the local cut's own parameters)
  VgsWeightParams W;
  W.inv_sig_p = 1.0f / p.sig_p; W.inv_sig_n = 1.0f / p.sig_n; W.inv_sig_o = 1.0f / p.sig_o;
  W.inv_sig_e = 1.0f / p.sig_e; W.inv_sig_c = 1.0f / p.sig_c;
  W.inv_sig_w2 = 1.0f / (p.sig_w * p.sig_w);
  W.svgs = (p.method == 3) ? 1 : 0;
  return W;
}

static vgs_status lg_scan(vgs_ctx* c, uint32_t* in, uint32_t* out, size_t n) {
  size_t bytes = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, c->lg_tmp.ensure(bytes));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->lg_tmp.p, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
  return VGS_OK;
}

// the row kernel over the stored rows (urow == nullptr) or over the built rows row0 .. row0 + n_rows - 1
template <bool WRITE>
static void lg_launch_rows(vgs_ctx* c, const LgWalk& G, const uint32_t* urow, uint32_t row0, uint32_t n_rows, int holds) {
  hipLaunchKernelGGL(k_lg_rows<WRITE>, dim3((G.nv + LG_WAVES - 1) / LG_WAVES), dim3(64 * LG_WAVES), 0, c->stream, G.nv, G.snode, G.slab, G.nbeg, G.nend,
                     c->used_rank.p, c->adj_key.p, c->adj_cnt.p, c->adj_stride, urow, row0, n_rows, c->rf_rows.p, c->rf_cnt.p, c->P.method == 2 ? 0 : 1,
                     holds, c->node.p, G.W, G.K, G.R, c->lg_nrec.p, c->lg_roff.p, c->lg_rec.p, G.rkey, G.tkey, G.ridx, c->lg_meta.p);
}

// one walk of every vertex: the stored rows, then for VGS the rows of the unused nodes, built chunk by chunk (built == true: the one chunk
// in rf_rows is the whole list and still holds the rows of the walk before)
template <bool WRITE>
static vgs_status lg_walk(vgs_ctx* c, const LgWalk& G, const uint32_t* urow, const uint32_t* un_node, uint32_t n_un, int64_t chunk, bool built) {
  const bool vgs = c->P.method == 2;
  lg_launch_rows<WRITE>(c, G, nullptr, 0, 0, vgs ? LG_HOLDS_ALWAYS : LG_HOLDS_SEARCH);
  for (int64_t o = 0; o < (int64_t)n_un; o += chunk) {
    const int64_t m = std::min(chunk, (int64_t)n_un - o);
    if (!built) {
      const vgs_status s = vgs_run_adjacency(c, true, c->rf_rows.p, c->rf_cnt.p, c->rf_nall.p, c->adj_r2, un_node + o, m);
      if (s != VGS_OK) return s;
    }
    lg_launch_rows<WRITE>(c, G, urow, (uint32_t)o, (uint32_t)m, c->adj_pruned ? LG_HOLDS_UNUSED : LG_HOLDS_ALWAYS);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}

// the unused nodes with a vertex and every vertex's row among them: what the plain walk needs besides LgWalk
struct LgPlainRows { const uint32_t *urow, *un_node; uint32_t n_un; int64_t chunk; };
static vgs_status lg_walk_plain(vgs_ctx* c, const LgWalk& G, bool write, void* arg) {
  const LgPlainRows& P = *(const LgPlainRows*)arg;
  if (write) return lg_walk<true>(c, G, P.urow, P.un_node, P.n_un, P.chunk, (int64_t)P.n_un <= P.chunk);
  return lg_walk<false>(c, G, P.urow, P.un_node, P.n_un, P.chunk, false);
}

// Step 2: the vertices X (nv of them, in (label, node) order) by node.  parent = iota, root = nodes sorted, part = vertices sorted;
// afterwards parent = the labels in that order
vgs_status vgs_lg_vertices_by_node(vgs_ctx* c, const LcVtx& X, uint32_t nv, int64_t K, LgWalk& G) {
  const int64_t V = c->V;
  VGS_HIP_TRY(c, c->lcc_nidx.ensure(2 * (size_t)V));
  uint32_t *snode = X.root, *sperm = X.part, *slab = X.parent, *nbeg = c->lcc_nidx.p, *nend = c->lcc_nidx.p + V;
  unsigned vbits = 1;
  while (vbits < 32 && (1ull << vbits) < (unsigned long long)V) ++vbits;
  hipLaunchKernelGGL(k_lg_iota, dim3(lg_grid(nv)), dim3(LG_TB), 0, c->stream, nv, X.parent);
  size_t t_vs = 0;
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_vs, X.node, snode, X.parent, sperm, (size_t)nv, 0, vbits, c->stream));
  VGS_HIP_TRY(c, c->lg_tmp.ensure(t_vs));
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->lg_tmp.p, t_vs, X.node, snode, X.parent, sperm, (size_t)nv, 0, vbits, c->stream));
  VGS_HIP_TRY(c, hipMemsetAsync(c->lcc_nidx.p, 0, 2 * (size_t)V * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_lg_node_runs, dim3(lg_grid(nv)), dim3(LG_TB), 0, c->stream, snode, sperm, X.label, nv, slab, nbeg, nend);
  VGS_HIP_TRY(c, hipGetLastError());
  G.nv = nv; G.K = (uint32_t)K; G.R = 0; G.snode = snode; G.slab = slab; G.nbeg = nbeg; G.nend = nend; G.W = lg_weight_params(c->P);
  G.rkey = nullptr; G.tkey = nullptr; G.ridx = nullptr;
  return VGS_OK;
}

// Steps 3 to 6 behind a walk of the caller's choice (the plain one, or labelgraph_tiles.hip's): count, scan, write; the sorts; heads,
// starts, chunk partials, fold.  The table is in lg_ab ... lg_wmax, lg_E rows, when the stream has been waited for -- which it has.
vgs_status vgs_lg_table_from_walk(vgs_ctx* c, const char* fn, LgWalk& G, LgWalkFn walk, void* arg) {
  const uint32_t nv = G.nv;
  const int64_t K = (int64_t)G.K;
  const size_t w = (size_t)nv + 1;
  vgs_status s;
  c->lg_E = 0;
  // step 3: count, scan, write
  VGS_HIP_TRY(c, c->lg_nrec.ensure(w)); VGS_HIP_TRY(c, c->lg_roff.ensure(w)); VGS_HIP_TRY(c, c->lg_meta.ensure(4));
  VGS_HIP_TRY(c, hipMemsetAsync(c->lg_meta.p, 0, 4 * sizeof(uint32_t), c->stream));
  VGS_HIP_TRY(c, hipMemsetAsync(c->lg_nrec.p, 0, w * sizeof(uint32_t), c->stream));
  if ((s = walk(c, G, false, arg)) != VGS_OK) return s;
  size_t t_scan0 = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_scan0, c->lg_nrec.p, c->lg_roff.p, (uint64_t)0, w, rocprim::plus<uint64_t>(), c->stream));
  VGS_HIP_TRY(c, c->lg_tmp.ensure(t_scan0));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->lg_tmp.p, t_scan0, c->lg_nrec.p, c->lg_roff.p, (uint64_t)0, w, rocprim::plus<uint64_t>(), c->stream));
  uint64_t R64 = 0;
  uint32_t meta[4] = {0, 0, 0, 0};
  VGS_READBACK(c, &R64, c->lg_roff.p + nv, 8);   // read-back: the number of records ...
  VGS_READBACK(c, meta, c->lg_meta.p, sizeof(meta));   // ... and of the proxies among them
  if (R64 == 0) return VGS_OK;
  // (this refusal is what lets lg_walk_body keep a record's position in one 32-bit word, in k_lg_rows and k_lgt_rows alike)
  if (R64 >= (1ull << 31)) { c->err = std::string(fn) + ": more than 2^31 (vertex, neighbour label) records"; return VGS_E_UNSUPPORTED; }
  const uint32_t R = (uint32_t)R64;
  const bool proxies = meta[2] != 0;
  VGS_HIP_TRY(c, c->lg_rec.ensure(R));
  VGS_HIP_TRY(c, c->lg_rkey.ensure(2 * (size_t)R)); VGS_HIP_TRY(c, c->lg_ridx.ensure(2 * (size_t)R)); VGS_HIP_TRY(c, c->lg_tkey.ensure(2 * (size_t)R));
  VGS_HIP_TRY(c, c->lg_ework.ensure(4 * ((size_t)R + 1)));   // head, inc, estart, chunk counts / starts (E <= R)
  uint64_t *key_a = c->lg_rkey.p, *key_b = key_a + R;
  uint32_t *idx_a = c->lg_ridx.p, *idx_b = idx_a + R;
  uint32_t *head = c->lg_ework.p, *inc = head + (R + 1), *estart = inc + (R + 1), *nch = estart + (R + 1);
  G.R = R; G.rkey = key_a; G.tkey = c->lg_tkey.p; G.ridx = idx_a;
  if ((s = walk(c, G, true, arg)) != VGS_OK) return s;
  // step 4: (with proxies) the stable sort by vertex, then the stable sort by edge
  unsigned bits = 1, tbits = 1;
  const unsigned long long kk = (unsigned long long)K * (unsigned long long)K;   // keys 0 .. K^2 - 1
  while (bits < 64 && (1ull << bits) < kk) ++bits;
  while (tbits < 32 && (1ull << tbits) < (unsigned long long)nv) ++tbits;
  uint64_t *key_in = key_a, *key_out = key_b;
  uint32_t *idx_in = idx_a, *idx_out = idx_b;
  size_t t_sort = 0, t_tsort = 0, t_inc = 0, t_ex = 0;
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, key_in, key_out, idx_in, idx_out, (size_t)R, 0, bits, c->stream));
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_tsort, c->lg_tkey.p, c->lg_tkey.p + R, idx_a, idx_b, (size_t)R, 0, tbits, c->stream));
  VGS_HIP_TRY(c, rocprim::inclusive_scan(nullptr, t_inc, head, inc, (size_t)R, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_ex, nch, nch, 0u, (size_t)R + 1, rocprim::plus<uint32_t>(), c->stream));   // (E + 1 <= R + 1)
  VGS_HIP_TRY(c, c->lg_tmp.ensure(std::max(std::max(t_sort, t_tsort), std::max(t_inc, t_ex))));
  if (proxies) {
    VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->lg_tmp.p, t_tsort, c->lg_tkey.p, c->lg_tkey.p + R, idx_a, idx_b, (size_t)R, 0, tbits, c->stream));
    hipLaunchKernelGGL(k_lg_gather_keys, dim3(lg_grid(R)), dim3(LG_TB), 0, c->stream, key_a, idx_b, R, key_b);
    key_in = key_b; key_out = key_a; idx_in = idx_b; idx_out = idx_a;
  }
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->lg_tmp.p, t_sort, key_in, key_out, idx_in, idx_out, (size_t)R, 0, bits, c->stream));
  // steps 5 and 6
  hipLaunchKernelGGL(k_lg_heads, dim3(lg_grid(R)), dim3(LG_TB), 0, c->stream, key_out, R, head);
  VGS_HIP_TRY(c, rocprim::inclusive_scan(c->lg_tmp.p, t_inc, head, inc, (size_t)R, rocprim::plus<uint32_t>(), c->stream));
  hipLaunchKernelGGL(k_lg_starts, dim3(lg_grid(R)), dim3(LG_TB), 0, c->stream, head, inc, R, estart, c->lg_meta.p);
  VGS_READBACK(c, meta, c->lg_meta.p, sizeof(meta));   // read-back: E
  const uint32_t E = meta[1];
  VGS_HIP_TRY(c, c->lg_ab.ensure(2 * (size_t)E)); VGS_HIP_TRY(c, c->lg_nodes.ensure(2 * (size_t)E)); VGS_HIP_TRY(c, c->lg_nshared.ensure(E));
  VGS_HIP_TRY(c, c->lg_npairs.ensure(E)); VGS_HIP_TRY(c, c->lg_nfin.ensure(E)); VGS_HIP_TRY(c, c->lg_wsum.ensure(E));
  VGS_HIP_TRY(c, c->lg_wmin.ensure(E)); VGS_HIP_TRY(c, c->lg_wmax.ensure(E));
  uint32_t* echunk = head;   // (head is free once estart is written; E + 1 <= R + 1 entries)
  hipLaunchKernelGGL(k_lg_nchunk, dim3(lg_grid((uint64_t)E + 1)), dim3(LG_TB), 0, c->stream, estart, E, nch);
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->lg_tmp.p, t_ex, nch, echunk, 0u, (size_t)E + 1, rocprim::plus<uint32_t>(), c->stream));
  // sum over edges of ceil(n_e / LG_CHUNK) <= R / LG_CHUNK + E: launched without reading the real number back
  const uint32_t n_chunks_max = R / LG_CHUNK + E + 1;
  VGS_HIP_TRY(c, c->lg_part.ensure(n_chunks_max));
  hipLaunchKernelGGL(k_lg_chunks, dim3((n_chunks_max + LG_WAVES - 1) / LG_WAVES), dim3(64 * LG_WAVES), 0, c->stream, idx_out, c->lg_rec.p, estart, echunk, E,
                     c->lg_part.p);
  hipLaunchKernelGGL(k_lg_final, dim3((E + LG_WAVES - 1) / LG_WAVES), dim3(64 * LG_WAVES), 0, c->stream, idx_out, c->lg_rec.p, estart, echunk, c->lg_part.p,
                     E, c->lg_ab.p, c->lg_nshared.p, c->lg_npairs.p, c->lg_nfin.p, c->lg_nodes.p, c->lg_wsum.p, c->lg_wmin.p, c->lg_wmax.p);
  VGS_HIP_TRY(c, hipGetLastError());
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the table is complete, and a labelling read in place is the caller's again
  c->lg_E = E;
  return VGS_OK;
}

static vgs_status lg_build(vgs_ctx* c, const char* fn, const int32_t* labels_dev, int64_t K, int64_t* n_skipped) {
  const int64_t V = c->V, U = c->U;
  c->lg_valid = false; c->lg_E = 0; c->lgt_own = c->lgt_valid = false;
  c->lcc_nv = 0; c->lct_own = c->lct_linked = c->lct_applied = false;   // (the vertex arrays of the last parts pass are overwritten)
  PsSort S;
  LcVtx X;
  uint32_t nv = 0;
  vgs_status s = vgs_label_vertices_on_device(c, fn, labels_dev, 0, c->N, K, n_skipped, S, &nv, X);
  if (s != VGS_OK) return s;
  if (nv == 0 || K <= 1) { VGS_HIP_TRY(c, hipStreamSynchronize(c->stream)); c->lg_valid = true; return VGS_OK; }
  LgWalk G;
  if ((s = vgs_lg_vertices_by_node(c, X, nv, K, G)) != VGS_OK) return s;
  const size_t w = (size_t)nv + 1;
  const uint32_t* snode = G.snode;
  // VGS: the distinct unused nodes with a vertex, and every vertex's row among them (the head flags are spent: lcc_flag takes these)
  const bool vgs = c->P.method == 2;
  uint32_t n_un = 0;
  uint32_t *urow = nullptr, *un_node = nullptr;
  int64_t chunk = 1;
  if (vgs && V - U > 0) {
    hipLaunchKernelGGL(k_lg_unused_flags, dim3(lg_grid(w)), dim3(LG_TB), 0, c->stream, snode, c->used_rank.p, nv, c->lcc_flag.p);
    if ((s = lg_scan(c, c->lcc_flag.p, c->lcc_vscan.p, w)) != VGS_OK) return s;
    VGS_READBACK(c, &n_un, c->lcc_vscan.p + nv, 4);
    if (n_un > 0) {
      VGS_HIP_TRY(c, c->lcc_uv.ensure((size_t)nv + n_un));
      urow = c->lcc_uv.p; un_node = urow + nv;
      hipLaunchKernelGGL(k_lg_unused_list, dim3(lg_grid(nv)), dim3(LG_TB), 0, c->stream, c->lcc_flag.p, c->lcc_vscan.p, snode, c->used_rank.p, nv, n_un,
                         un_node, urow);
      VGS_HIP_TRY(c, hipGetLastError());
      chunk = std::max<int64_t>(1, std::min<int64_t>(n_un, ((int64_t)32 << 20) / std::max(1, c->adj_stride)));   // at most 256 MB of keys
      VGS_HIP_TRY(c, c->rf_rows.ensure((size_t)chunk * c->adj_stride)); VGS_HIP_TRY(c, c->rf_cnt.ensure((size_t)chunk)); VGS_HIP_TRY(c, c->rf_nall.ensure((size_t)chunk));
    }
  }
  LgPlainRows P{urow, un_node, n_un, chunk};
  if ((s = vgs_lg_table_from_walk(c, fn, G, lg_walk_plain, &P)) != VGS_OK) return s;
  c->lg_valid = true;
  return VGS_OK;
}

static vgs_status lg_check(vgs_ctx* c, const char* fn, const int32_t* labels, int64_t n, int64_t K) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of the cloud and of its neighbourhood graph; the adjacency graph of a labelling across the ranks of the tiled driver is not computed by this call: vgs_tiles_point_label_graph";
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

static vgs_status lg_graph(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped) {
  if (!c) return VGS_E_ARG;
  if (n_edges) *n_edges = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = lg_check(c, fn, labels, n, K);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  c->lg_valid = false;
  if (!on_device && (s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK) return s;
  if ((s = lg_build(c, fn, labels, K, n_skipped)) != VGS_OK) return s;
  if (n_edges) *n_edges = c->lg_E;
  return VGS_OK;
}

extern "C" vgs_status vgs_point_label_graph(vgs_ctx* c, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped) {
  return lg_graph(c, "vgs_point_label_graph", labels_host, false, n, K, n_edges, n_skipped);
}

extern "C" vgs_status vgs_point_label_graph_device(vgs_ctx* c, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped) {
  return lg_graph(c, "vgs_point_label_graph_device", labels_dev, true, n, K, n_edges, n_skipped);
}

static vgs_status lg_result(vgs_ctx* c, const char* fn) {
  if (!c) return VGS_E_ARG;
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context holds only part of the cloud; the adjacency graph of a labelling across the ranks of the tiled driver is not computed by this call: vgs_tiles_point_label_graph";
    return VGS_E_STATE;
  }
  if (c->stage < ST_SEGMENTED || !c->lg_valid) {
    c->err = std::string(fn) + ": no label graph since the last run of the stages (vgs_point_label_graph first)";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

#define LG_COPY(dst, src, count) \
  if ((dst) && (count) > 0) VGS_HIP_TRY(c, hipMemcpy((dst), (src), (size_t)(count) * sizeof(*(dst)), hipMemcpyDeviceToHost))

extern "C" vgs_status vgs_get_point_label_graph(vgs_ctx* c, int32_t* seg_ab, int64_t* n_shared, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                                double* w_sum, float* w_min, float* w_max) {
  vgs_status s = lg_result(c, "vgs_get_point_label_graph");
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const int64_t E = c->lg_E;
  LG_COPY(seg_ab, c->lg_ab.p, 2 * E); LG_COPY(n_shared, c->lg_nshared.p, E); LG_COPY(n_pairs, c->lg_npairs.p, E); LG_COPY(n_finite, c->lg_nfin.p, E);
  LG_COPY(nodes_ab, c->lg_nodes.p, 2 * E); LG_COPY(w_sum, c->lg_wsum.p, E); LG_COPY(w_min, c->lg_wmin.p, E); LG_COPY(w_max, c->lg_wmax.p, E);
  return VGS_OK;
}

extern "C" vgs_status vgs_get_point_label_graph_device(vgs_ctx* c, int64_t* n_edges, const int32_t** seg_ab, const int64_t** n_shared,
                                                       const int64_t** n_pairs, const int64_t** n_finite, const int32_t** nodes_ab,
                                                       const double** w_sum, const float** w_min, const float** w_max) {
  if (n_edges) *n_edges = 0;
  vgs_status s = lg_result(c, "vgs_get_point_label_graph_device");
  if (s != VGS_OK) return s;
  const bool rows = c->lg_E > 0;
  if (n_edges) *n_edges = c->lg_E;
  if (seg_ab) *seg_ab = rows ? c->lg_ab.p : nullptr;
  if (n_shared) *n_shared = rows ? c->lg_nshared.p : nullptr;
  if (n_pairs) *n_pairs = rows ? c->lg_npairs.p : nullptr;
  if (n_finite) *n_finite = rows ? c->lg_nfin.p : nullptr;
  if (nodes_ab) *nodes_ab = rows ? c->lg_nodes.p : nullptr;
  if (w_sum) *w_sum = rows ? c->lg_wsum.p : nullptr;
  if (w_min) *w_min = rows ? c->lg_wmin.p : nullptr;
  if (w_max) *w_max = rows ? c->lg_wmax.p : nullptr;
  return VGS_OK;
}
