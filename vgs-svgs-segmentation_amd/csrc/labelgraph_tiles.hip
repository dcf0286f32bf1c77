// labelgraph_tiles.hip -- a tile context's share of the adjacency graph of a per-point labelling across the ranks of the tiled driver
// (include/vgs.h: vgs_own_point_label_band, vgs_own_point_label_graph; include/vgs_tiles.h states the counting rule and the protocol,
// csrc/tiles.cpp runs it: vgs_tiles_point_label_graph).  VGS only, as the tiled path.
//
// The rule: every record of labelgraph.hip lives on the rank that OWNS the node of the vertex it speaks for (owned[]: the voxel's centre
// lies in the rank's region; every voxel of the shared grid has one owner).  A vertex's own records and the proxy records written on its
// behalf are then on one rank, a contact is counted by the walker of its counting side on that side's owner, a shared node by its owner.
//
// Step 1 (vgs_own_point_label_band).  labelcc.hip's steps 1 and 2 over the rank's OWN points (vgs_label_vertices_on_device with the own
// point range) give the own vertices; labelcc_tiles.hip's band step (vgs_lt_band_on_device) compacts those within graph_size + voxel_size
// of a border line as (code, label).
// Step 3 (vgs_own_point_label_graph) over the other ranks' records:
//   vgs_lt_find_on_device   code -> local node, key = label << 32 | node, all ones for a code this rank does not hold
//   k_lgt_merge_keys        ... also for a label outside 0 .. K-1; the own vertices' keys behind them
//   radix sort, unique      the merged list in (label, node) order; a vertex two ranks publish is one vertex.  All ones sort last.
//   k_lgt_split_keys        node | label of every merged vertex: the list labelgraph.hip's step 2 takes (vgs_lg_vertices_by_node)
//   k_lgt_unused_flags / k_lgt_unused_list  the distinct unused nodes of the merged list that walk a built row: the owned ones, and with
//                           pruned stored rows the non-owned ones too
//   k_lgt_rows<false / true>  labelgraph_walk.hpp's walk in tile mode; vgs_lg_table_from_walk runs the rest of labelgraph.hip's pipeline
// What the walk reads is complete: the labels of an owned node and of every node in its row come from this rank's points or from the
// band records of the rank that holds the points (DESIGN.md 8 has the argument), the rows of owned nodes end inside the halo, and node
// records of halo voxels equal their owner's.
// Everything but w_sum is integer or an extremum; w_sum is folded in the fixed order of labelgraph.hip.  No float atomics; the one integer
// atomic is the walk's proxy count.
#include <string.h>

#include <algorithm>
#include <string>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "labelgraph_walk.hpp"

#define LGT_TB 256

// key[0 .. nf): the looked-up records (a label outside 0 .. K-1 drops out); key[nf .. nf + nv): the own vertices
__global__ __launch_bounds__(LGT_TB) void k_lgt_merge_keys(uint64_t* __restrict__ key, uint32_t nf, uint32_t K, const uint32_t* __restrict__ vnode,
                                                           const uint32_t* __restrict__ vlabel, uint32_t nv) {
  const uint64_t i = (uint64_t)blockIdx.x * LGT_TB + threadIdx.x;
  if (i < (uint64_t)nf) {
    const uint64_t k = key[i];
    if (k != ~0ull && (uint32_t)(k >> 32) >= K) key[i] = ~0ull;
  } else if (i - nf < (uint64_t)nv) {
    const uint32_t j = (uint32_t)(i - nf);
    key[i] = ((uint64_t)vlabel[j] << 32) | (uint64_t)vnode[j];
  }
}
__global__ __launch_bounds__(LGT_TB) void k_lgt_split_keys(const uint64_t* __restrict__ key, uint32_t m, uint32_t* __restrict__ vnode, uint32_t* __restrict__ vlabel) {
  const uint64_t i = (uint64_t)blockIdx.x * LGT_TB + threadIdx.x;
  if (i >= (uint64_t)m) return;
  const uint64_t k = key[i];
  vnode[i] = (uint32_t)k; vlabel[i] = (uint32_t)(k >> 32);
}

// labelgraph.hip's unused list over the merged list in (node, label) order, for the nodes whose vertices walk a built row in tile mode:
// unused and owned, or unused and not owned when the stored rows are pruned (flag[nv] = 0 closes the scan)
__device__ __forceinline__ bool lgt_walks_built(uint32_t v, const uint32_t* __restrict__ used_rank, const uint8_t* __restrict__ owned, int pruned) {
  return used_rank[v] == LG_NONE && (owned[v] != 0 || pruned != 0);
}
__global__ __launch_bounds__(LGT_TB) void k_lgt_unused_flags(const uint32_t* __restrict__ snode, const uint32_t* __restrict__ used_rank,
                                                             const uint8_t* __restrict__ owned, int pruned, uint32_t nv, uint32_t* __restrict__ flag) {
  const uint64_t t = (uint64_t)blockIdx.x * LGT_TB + threadIdx.x;
  if (t > (uint64_t)nv) return;
  flag[t] = (t < (uint64_t)nv && lgt_walks_built(snode[t], used_rank, owned, pruned) && (t == 0 || snode[t - 1] != snode[t])) ? 1u : 0u;
}
__global__ __launch_bounds__(LGT_TB) void k_lgt_unused_list(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ snode,
                                                            const uint32_t* __restrict__ used_rank, const uint8_t* __restrict__ owned, int pruned, uint32_t nv,
                                                            uint32_t cap, uint32_t* __restrict__ un_node, uint32_t* __restrict__ urow) {
  const uint64_t t = (uint64_t)blockIdx.x * LGT_TB + threadIdx.x;
  if (t >= (uint64_t)nv) return;
  const uint32_t v = snode[t];
  if (!lgt_walks_built(v, used_rank, owned, pruned)) { urow[t] = LG_NONE; return; }
  const uint32_t o = excl[t] + flag[t] - 1u;   // the node's head is at or in front of t
  urow[t] = o;
  if (flag[t] && o < cap) un_node[o] = v;      // (cap = the number of flags: the bound only guards the list)
}

// the walk in tile mode (labelgraph_walk.hpp): one wavefront per merged vertex.  rows / rows_cnt: the stored rows (urow == nullptr) or the
// built ones -- a launch reads one of the two
template <bool WRITE>
__global__ __launch_bounds__(64 * LG_WAVES) void k_lgt_rows(uint32_t nv, const uint32_t* __restrict__ snode, const uint32_t* __restrict__ slab,
                                                            const uint32_t* __restrict__ nbeg, const uint32_t* __restrict__ nend,
                                                            const uint32_t* __restrict__ used_rank, int adj_stride, const uint32_t* __restrict__ urow,
                                                            uint32_t row0, uint32_t n_rows, const uint64_t* __restrict__ rows,
                                                            const uint32_t* __restrict__ rows_cnt, int holds, const NodeRec* __restrict__ node,
                                                            VgsWeightParams W, uint32_t K, uint32_t R, uint32_t* __restrict__ n_rec,
                                                            const uint64_t* __restrict__ rec_off, LgRec* __restrict__ rec, uint64_t* __restrict__ rkey,
                                                            uint32_t* __restrict__ tkey, uint32_t* __restrict__ ridx, uint32_t* __restrict__ meta,
                                                            const uint8_t* __restrict__ owned) {
  lg_walk_body<WRITE, true>(nv, snode, slab, nbeg, nend, used_rank, rows, rows_cnt, adj_stride, urow, row0, n_rows, rows, rows_cnt, 0, holds, node, W, K, R, n_rec,
                            rec_off, rec, rkey, tkey, ridx, meta, owned);
}

// ---------------------------------------------------------------------------------------------------------------------- host
static unsigned lgt_grid(uint64_t n) { return (unsigned)((n + LGT_TB - 1) / LGT_TB); }

static vgs_status lgt_check(vgs_ctx* c, const char* fn) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (!c->have_region || c->n_own < 0) {
    c->err = std::string(fn) + ": a tile context (vgs_set_owned_region and vgs_set_own_point_range) only";
    return VGS_E_STATE;
  }
  if (c->P.method != 2) { c->err = std::string(fn) + ": the tiled path is VGS only"; return VGS_E_UNSUPPORTED; }
  return VGS_OK;
}

static vgs_status lgt_band(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t n, int64_t K, int64_t* n_band, int64_t* n_skipped) {
  if (!c) return VGS_E_ARG;
  if (n_band) *n_band = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = lgt_check(c, fn);
  if (s != VGS_OK) return s;
  // the own pass overwrites the vertex arrays of the parts pass and of the single-context graph
  c->lgt_own = c->lgt_valid = false; c->lg_valid = false; c->lg_E = 0;
  c->lcc_nv = 0; c->lct_own = c->lct_linked = c->lct_applied = false;
  if (n != c->n_own) {
    c->err = std::string(fn) + ": n = " + std::to_string(n) + " must equal the number of own points of the context, " + std::to_string(c->n_own);
    return VGS_E_ARG;
  }
  if (!labels && n > 0) { c->err = std::string(fn) + ": labels is NULL"; return VGS_E_ARG; }
  if (K < 0 || K > (int64_t)0x7fffffff) { c->err = std::string(fn) + ": K = " + std::to_string(K) + " is out of range"; return VGS_E_ARG; }
  if (c->own_first < 0 || c->own_first + n > c->N) {
    c->err = std::string(fn) + ": the own point range ends at " + std::to_string(c->own_first + n) + ", the cloud holds " + std::to_string(c->N) + " points";
    return VGS_E_ARG;
  }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  if (!on_device && (s = vgs_upload_point_labels(c, labels, n, &labels)) != VGS_OK) return s;
  PsSort S;
  LcVtx X;
  uint32_t nv = 0, nb = 0;
  if ((s = vgs_label_vertices_on_device(c, fn, labels, c->own_first, n, K, n_skipped, S, &nv, X)) != VGS_OK) return s;
  if (K <= 1) nv = 0;   // no two labels: no edge, nothing to publish
  if ((s = vgs_lt_band_on_device(c, X.node, X.label, nullptr, nv, &nb)) != VGS_OK) return s;   // (code and label only)
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // a labelling read in place is the caller's again
  c->lgt_nv = nv; c->lgt_K = K; c->lgt_band = (int64_t)nb; c->lgt_hits = 0; c->lgt_own = true;
  if (n_band) *n_band = (int64_t)nb;
  return VGS_OK;
}

extern "C" vgs_status vgs_own_point_label_band(vgs_ctx* c, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_band, int64_t* n_skipped) {
  return lgt_band(c, "vgs_own_point_label_band", labels_host, false, n, K, n_band, n_skipped);
}
extern "C" vgs_status vgs_own_point_label_band_device(vgs_ctx* c, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_band, int64_t* n_skipped) {
  return lgt_band(c, "vgs_own_point_label_band_device", labels_dev, true, n, K, n_band, n_skipped);
}

static vgs_status lgt_have_own(vgs_ctx* c, const char* fn) {
  if (!c) return VGS_E_ARG;
  vgs_status s = lgt_check(c, fn);
  if (s != VGS_OK) return s;
  if (!c->lgt_own) {
    c->err = std::string(fn) + ": no own band since the last run of the stages or the last parts pass (vgs_own_point_label_band first)";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

#define LGT_COPY(dst, src, count) \
  if ((dst) && (count) > 0) VGS_HIP_TRY(c, hipMemcpy((dst), (src), (size_t)(count) * sizeof(*(dst)), hipMemcpyDeviceToHost))

extern "C" vgs_status vgs_get_own_point_label_band(vgs_ctx* c, uint64_t* code, int32_t* label) {
  vgs_status s = lgt_have_own(c, "vgs_get_own_point_label_band");
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  LGT_COPY(code, c->lct_bcode.p, c->lgt_band); LGT_COPY(label, c->lct_blabel.p, c->lgt_band);
  return VGS_OK;
}

// the unused nodes that walk a built row and every vertex's row among them: what the tile walk needs besides LgWalk
struct LgtRows { const uint32_t *urow, *un_node; uint32_t n_un; int64_t chunk; };

template <bool WRITE>
static void lgt_launch_rows(vgs_ctx* c, const LgWalk& G, const uint32_t* urow, uint32_t row0, uint32_t n_rows, int holds) {
  hipLaunchKernelGGL(k_lgt_rows<WRITE>, dim3((G.nv + LG_WAVES - 1) / LG_WAVES), dim3(64 * LG_WAVES), 0, c->stream, G.nv, G.snode, G.slab, G.nbeg, G.nend,
                     c->used_rank.p, c->adj_stride, urow, row0, n_rows, urow ? c->rf_rows.p : c->adj_key.p, urow ? c->rf_cnt.p : c->adj_cnt.p, holds, c->node.p, G.W,
                     G.K, G.R, c->lg_nrec.p, c->lg_roff.p, c->lg_rec.p, G.rkey, G.tkey, G.ridx, c->lg_meta.p, c->owned.p);
}

// one walk of every merged vertex: the stored rows of the owned used nodes, then the rows built chunk by chunk (the write walk finds the
// one chunk of the count walk still in rf_rows when the whole list fits it)
template <bool WRITE>
static vgs_status lgt_walk_t(vgs_ctx* c, const LgWalk& G, const LgtRows& P) {
  const bool built = WRITE && (int64_t)P.n_un <= P.chunk;
  if (c->U > 0) lgt_launch_rows<WRITE>(c, G, nullptr, 0, 0, LG_HOLDS_ALWAYS);
  for (int64_t o = 0; o < (int64_t)P.n_un; o += P.chunk) {
    const int64_t m = std::min(P.chunk, (int64_t)P.n_un - o);
    if (!built) {
      const vgs_status s = vgs_run_adjacency(c, true, c->rf_rows.p, c->rf_cnt.p, c->rf_nall.p, c->adj_r2, P.un_node + o, m);
      if (s != VGS_OK) return s;
    }
    lgt_launch_rows<WRITE>(c, G, P.urow, (uint32_t)o, (uint32_t)m, c->adj_pruned ? LG_HOLDS_UNUSED : LG_HOLDS_ALWAYS);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}
static vgs_status lgt_walk(vgs_ctx* c, const LgWalk& G, bool write, void* arg) {
  const LgtRows& P = *(const LgtRows*)arg;
  return write ? lgt_walk_t<true>(c, G, P) : lgt_walk_t<false>(c, G, P);
}

extern "C" vgs_status vgs_own_point_label_graph(vgs_ctx* c, const uint64_t* code, const int32_t* label, int64_t n, int64_t* n_edges) {
  const char* fn = "vgs_own_point_label_graph";
  if (n_edges) *n_edges = 0;
  vgs_status s = lgt_have_own(c, fn);
  if (s != VGS_OK) return s;
  c->lgt_valid = false; c->lg_E = 0; c->lgt_hits = 0;
  if (n < 0 || n > (int64_t)0x3fffffff || (n > 0 && (!code || !label))) {
    c->err = std::string(fn) + ": n records need two arrays, n at most 2^30 - 1";
    return VGS_E_ARG;
  }
  const int64_t V = c->V, K = c->lgt_K;
  const uint32_t nv = c->lgt_nv, nf = (K > 1 && V > 0) ? (uint32_t)n : 0u;
  const size_t m_in = (size_t)nf + nv;
  if (m_in == 0 || m_in > (size_t)0x7fffffff) {
    if (m_in > 0) { c->err = std::string(fn) + ": more than 2^31 - 1 vertices"; return VGS_E_UNSUPPORTED; }
    c->lgt_valid = true;
    return VGS_OK;
  }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  // the own vertices (lcc_vtx: node | label, nv + 1 words each) and the other ranks' records, looked up, as one key list
  const size_t w_own = (size_t)nv + 1;
  const uint32_t *own_node = c->lcc_vtx.p, *own_label = nv > 0 ? c->lcc_vtx.p + w_own : nullptr;
  VGS_HIP_TRY(c, c->lct_key.ensure(m_in)); VGS_HIP_TRY(c, c->lct_key2.ensure(m_in)); VGS_HIP_TRY(c, c->lct_val.ensure(std::max<size_t>(nf, 1)));
  VGS_HIP_TRY(c, c->lct_count.ensure(4));
  unsigned long long* counts = (unsigned long long*)c->lct_count.p;
  VGS_HIP_TRY(c, hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), c->stream));
  if (nf > 0) {
    VGS_HIP_TRY(c, c->lct_fcode.ensure(nf)); VGS_HIP_TRY(c, c->lct_flabel.ensure(nf));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->lct_fcode.p, code, (size_t)nf * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->lct_flabel.p, label, (size_t)nf * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((s = vgs_lt_find_on_device(c, c->lct_fcode.p, c->lct_flabel.p, (int64_t)nf, c->lct_key.p, c->lct_val.p, counts)) != VGS_OK) return s;
  }
  hipLaunchKernelGGL(k_lgt_merge_keys, dim3(lgt_grid(m_in)), dim3(LGT_TB), 0, c->stream, c->lct_key.p, nf, (uint32_t)K, own_node, own_label, nv);
  VGS_HIP_TRY(c, hipGetLastError());
  size_t t_sort = 0, t_un = 0;
  VGS_HIP_TRY(c, rocprim::radix_sort_keys(nullptr, t_sort, c->lct_key.p, c->lct_key2.p, m_in, 0, 64, c->stream));
  VGS_HIP_TRY(c, rocprim::unique(nullptr, t_un, c->lct_key2.p, c->lct_key.p, counts + 1, m_in, rocprim::equal_to<uint64_t>(), c->stream));
  VGS_HIP_TRY(c, c->ps_tmp.ensure(std::max(t_sort, t_un)));
  VGS_HIP_TRY(c, rocprim::radix_sort_keys(c->ps_tmp.p, t_sort, c->lct_key.p, c->lct_key2.p, m_in, 0, 64, c->stream));
  VGS_HIP_TRY(c, rocprim::unique(c->ps_tmp.p, t_un, c->lct_key2.p, c->lct_key.p, counts + 1, m_in, rocprim::equal_to<uint64_t>(), c->stream));
  unsigned long long hc[2] = {0, 0};
  VGS_READBACK(c, hc, counts, sizeof(hc));   // (also: the upload has read the caller's arrays)
  c->lgt_hits = (int64_t)std::min<unsigned long long>(hc[0], nf);
  uint32_t M = (uint32_t)std::min<unsigned long long>(hc[1], m_in);
  if (M > 0) {   // the records that dropped out are one key at the end
    uint64_t last = 0;
    VGS_READBACK(c, &last, c->lct_key.p + (M - 1), sizeof(last));
    if (last == ~0ull) --M;
  }
  if (M == 0) { c->lgt_valid = true; return VGS_OK; }
  // the merged vertices in (label, node) order, then labelgraph.hip's step 2
  const size_t w = (size_t)M + 1;
  VGS_HIP_TRY(c, c->lgt_vtx.ensure(5 * w));
  LcVtx X;
  X.node = c->lgt_vtx.p; X.label = X.node + w; X.parent = X.label + w; X.root = X.parent + w; X.part = X.root + w; X.q = nullptr;
  hipLaunchKernelGGL(k_lgt_split_keys, dim3(lgt_grid(M)), dim3(LGT_TB), 0, c->stream, c->lct_key.p, M, X.node, X.label);
  LgWalk G;
  if ((s = vgs_lg_vertices_by_node(c, X, M, K, G)) != VGS_OK) return s;
  // the unused nodes whose vertices walk a built row
  LgtRows P{nullptr, nullptr, 0u, 1};
  if (V - c->U > 0) {
    uint32_t n_un = 0;
    VGS_HIP_TRY(c, c->lgt_flag.ensure(w)); VGS_HIP_TRY(c, c->lgt_scan.ensure(w));
    hipLaunchKernelGGL(k_lgt_unused_flags, dim3(lgt_grid(w)), dim3(LGT_TB), 0, c->stream, G.snode, c->used_rank.p, c->owned.p, c->adj_pruned ? 1 : 0, M, c->lgt_flag.p);
    size_t t_scan = 0;
    VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_scan, c->lgt_flag.p, c->lgt_scan.p, 0u, w, rocprim::plus<uint32_t>(), c->stream));
    VGS_HIP_TRY(c, c->ps_tmp.ensure(t_scan));
    VGS_HIP_TRY(c, rocprim::exclusive_scan(c->ps_tmp.p, t_scan, c->lgt_flag.p, c->lgt_scan.p, 0u, w, rocprim::plus<uint32_t>(), c->stream));
    VGS_READBACK(c, &n_un, c->lgt_scan.p + M, 4);
    if (n_un > 0) {
      VGS_HIP_TRY(c, c->lcc_uv.ensure((size_t)M + n_un));
      uint32_t *urow = c->lcc_uv.p, *un_node = urow + M;
      hipLaunchKernelGGL(k_lgt_unused_list, dim3(lgt_grid(M)), dim3(LGT_TB), 0, c->stream, c->lgt_flag.p, c->lgt_scan.p, G.snode, c->used_rank.p, c->owned.p,
                         c->adj_pruned ? 1 : 0, M, n_un, un_node, urow);
      VGS_HIP_TRY(c, hipGetLastError());
      P.urow = urow; P.un_node = un_node; P.n_un = n_un;
      P.chunk = std::max<int64_t>(1, std::min<int64_t>(n_un, ((int64_t)32 << 20) / std::max(1, c->adj_stride)));   // at most 256 MB of keys
      VGS_HIP_TRY(c, c->rf_rows.ensure((size_t)P.chunk * c->adj_stride)); VGS_HIP_TRY(c, c->rf_cnt.ensure((size_t)P.chunk)); VGS_HIP_TRY(c, c->rf_nall.ensure((size_t)P.chunk));
    }
  }
  if ((s = vgs_lg_table_from_walk(c, fn, G, lgt_walk, &P)) != VGS_OK) return s;
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->lgt_valid = true;
  if (n_edges) *n_edges = c->lg_E;
  return VGS_OK;
}

extern "C" vgs_status vgs_get_own_point_label_graph(vgs_ctx* c, int32_t* seg_ab, int64_t* n_shared, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                                    double* w_sum, float* w_min, float* w_max) {
  const char* fn = "vgs_get_own_point_label_graph";
  vgs_status s = lgt_have_own(c, fn);
  if (s != VGS_OK) return s;
  if (!c->lgt_valid) { c->err = std::string(fn) + ": no partial table since the last own band (vgs_own_point_label_graph first)"; return VGS_E_STATE; }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const int64_t E = c->lg_E;
  LGT_COPY(seg_ab, c->lg_ab.p, 2 * E); LGT_COPY(n_shared, c->lg_nshared.p, E); LGT_COPY(n_pairs, c->lg_npairs.p, E); LGT_COPY(n_finite, c->lg_nfin.p, E);
  LGT_COPY(nodes_ab, c->lg_nodes.p, 2 * E); LGT_COPY(w_sum, c->lg_wsum.p, E); LGT_COPY(w_min, c->lg_wmin.p, E); LGT_COPY(w_max, c->lg_wmax.p, E);
  return VGS_OK;
}

extern "C" vgs_status vgs_get_own_point_label_graph_counts(vgs_ctx* c, int64_t* n_band, int64_t* n_hits, int64_t* n_edges) {
  vgs_status s = lgt_have_own(c, "vgs_get_own_point_label_graph_counts");
  if (s != VGS_OK) return s;
  if (n_band) *n_band = c->lgt_band;
  if (n_hits) *n_hits = c->lgt_hits;
  if (n_edges) *n_edges = c->lgt_valid ? c->lg_E : 0;
  return VGS_OK;
}
