// seggraph.hip -- the segment adjacency graph of the kept segments (no reference counterpart: which segments touch, and how strongly the
// local cut's own weight links them across the boundary).  Edge {a < b} exists when a used node u of label a holds a used node v of label b
// in its stored adjacency row (include/vgs.h gives the definition and the fields).
//
// Data flow (the rows, labels and node records already sit in HBM after a run: adj_key / adj_cnt per used node, vox_label, node):
//   1. k_sg_labels: per node its effective label (the kept label of a used node, -1 otherwise)
//   2. k_sg_rows<false>: one wavefront per used row counts the distinct boundary labels B (B >= 0, B != the row's label A) of its row;
//      exclusive scan -> every row's first record
//   3. k_sg_rows<true>: the same wavefront writes one record per (u, B), B ascending: cnt_lt / n_finite / w_sum / w_min / w_max over the
//      neighbours v > u of label B (each unordered node pair is counted once, from the row of its lower id), and checks that u is in v's row
//   4. one stable radix sort of the records by the unordered label pair min(A, B) * K + max(A, B)
//   5. k_sg_heads + an inclusive scan + k_sg_starts: the first record of every edge and E (read back once)
//   6. k_sg_nchunk + an exclusive scan: every edge ceil(records / SG_CHUNK) chunks; k_sg_chunks: one wavefront per chunk writes a partial;
//      k_sg_final: one wavefront per edge folds its partials
// A row is walked once per distinct boundary label, plus once: the wave-uniform loop folds the label found by the previous walk and finds
// the next larger one (a wave-wide min), so no per-entry state is kept and a row of any length is read in chunks of 64 entries.
// Determinism: which entry or record a lane reads depends on (row or chunk, lane, step) only; lanes fold by a fixed xor butterfly, a
// chunk's records in sorted order, an edge's partials by lane stride then the same butterfly; the records enter the stable sort in (row,
// label) order.  No atomics.  Scratch: own buffers only (sg_*).  Computed on request and cached until the next run (sg_valid).
//
// Tile contexts (the tiled driver, include/vgs_tiles.h): vgs_get_own_segment_graph is the same pipeline over GLOBAL labels with key space
// K = kept_global, restricted to what this rank counts -- the rows of its OWNED used voxels (k_sg_rows<*, true>: one byte load per row
// decides).  Such a row holds halo voxels; their labels come from the other ranks' boundary records (vgs_set_halo_labels: k_sg_halo_find
// looks every code up in vox_code and fills sg_halo), never from vox_label.  A used halo voxel without a record is SG_UNKNOWN; the count
// walk adds up the unknown neighbours of owned rows and the call fails when there is one.
#include <climits>
#include <cmath>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "wavefold.hpp"

#define SG_WAVES 4                 // wavefronts per workgroup of the row, chunk and edge kernels
#define SG_PPL 4                   // records per lane of a chunk
#define SG_CHUNK (64 * SG_PPL)     // records per chunk
#define SG_UNKNOWN (-2)            // tile contexts: a voxel of another rank whose label no record has brought (-1 = dropped or unused)

// effective label of node v: its kept label if it is used, -1 otherwise (unused voxels and dropped clusters take no part)
__global__ void k_sg_labels(const int32_t* __restrict__ vox_label, const uint32_t* __restrict__ used_rank, int64_t V, int32_t* __restrict__ lab) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  lab[v] = used_rank[v] == 0xffffffffu ? -1 : vox_label[v];
}

// tile contexts: the effective label of an owned used voxel is its (global) vox_label, of any other used voxel its entry of the halo table
// (all SG_UNKNOWN without one); meta[3] = 1 if a label is not below K
__global__ void k_sg_tile_labels(const int32_t* __restrict__ vox_label, const uint32_t* __restrict__ used_rank, const uint8_t* __restrict__ owned,
                                 const int32_t* __restrict__ halo, int64_t V, int32_t K, int32_t* __restrict__ lab, uint32_t* __restrict__ meta) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  int32_t l = -1;
  if (used_rank[v] != 0xffffffffu) {
    l = owned[v] ? vox_label[v] : (halo ? halo[v] : SG_UNKNOWN);
    if (l >= K) { meta[3] = 1u; l = -1; }   // (every writer stores the same value)
  }
  lab[v] = l;
}

// halo[v] = label[k] for the voxel v whose code is code[k], if this rank holds it and does not own it (vox_code is sorted, descending;
// records of one code carry one label: the boundary merge unites them)
__global__ void k_sg_halo_find(const uint64_t* __restrict__ code, const int32_t* __restrict__ label, int64_t n, const uint64_t* __restrict__ vox_code,
                               int64_t V, const uint8_t* __restrict__ owned, int32_t* __restrict__ halo) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t v = vgs_find_voxel(vox_code, V, code[k]);
  if (v < V && !owned[v]) halo[v] = label[k];
}

// One wavefront per used row r (node u = used_ids[r], label A).  WRITE = false: n_rec[r] = its distinct boundary labels; WRITE = true: one
// record per boundary label, ascending, at rec_off[r] ...  TILE: only the rows of owned voxels count (a row of another rank's voxel leaves
// at once), and WRITE = false also gives n_unk[r] = the row's neighbours of label SG_UNKNOWN.
template <bool WRITE, bool TILE = false>
__global__ __launch_bounds__(64 * SG_WAVES) void k_sg_rows(const uint32_t* __restrict__ used_ids, int64_t U, const uint64_t* __restrict__ adj_key,
                                                           const uint32_t* __restrict__ adj_cnt, int adj_stride, const uint32_t* __restrict__ used_rank,
                                                           const int32_t* __restrict__ lab, const NodeRec* __restrict__ node, VgsWeightParams W,
                                                           uint32_t K, uint32_t* __restrict__ n_rec, const uint64_t* __restrict__ rec_off,
                                                           SgRec* __restrict__ rec, uint64_t* __restrict__ rkey, uint32_t* __restrict__ ridx,
                                                           uint32_t* __restrict__ asym, const uint8_t* __restrict__ owned = nullptr,
                                                           uint32_t* __restrict__ n_unk = nullptr) {
  const int64_t r = (int64_t)blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= U) return;   // (whole wavefronts; no barrier follows)
  const uint32_t u = used_ids[r];
  const int32_t A = lab[u];
  uint32_t n = A < 0 ? 0u : adj_cnt[r];
  if (TILE) { if (!owned[u]) n = 0u; }
  int unk = 0;
  const uint64_t* row = adj_key + r * (int64_t)adj_stride;
  uint64_t o = 0;
  if (WRITE) o = rec_off[r];
  uint32_t k = 0;
  int32_t cur = -1;   // the label this walk folds (none on the first walk)
  while (true) {
    int nxt = INT_MAX;
    int c_lt = 0, c_fin = 0;
    double s = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    for (uint32_t base = 0; base < n; base += 64) {
      const uint32_t j = base + lane;
      if (j >= n) continue;
      const uint64_t e = row[j];
      const uint32_t v = (uint32_t)e;
      const int32_t B = lab[v];
      if (TILE && !WRITE) { if (B == SG_UNKNOWN && cur < 0) ++unk; }
      if (B < 0 || B == A) continue;
      if (B > cur) { nxt = min(nxt, (int)B); continue; }
      if (!WRITE || B != cur) continue;
      const uint32_t rv = used_rank[v];
      if (!sg_in_row(adj_key + (int64_t)rv * adj_stride, adj_cnt[rv], (e & 0xffffffff00000000ull) | (uint64_t)u, u)) *asym = 1u;
      if (v > u) {
        ++c_lt;
        const float w = vm_pair_weight(node[u], node[v], W);   // the lower id first: vgs_get_local_weights' entry of that ordered pair
        if (!isnan(w)) { ++c_fin; s += (double)w; mn = fminf(mn, w); mx = fmaxf(mx, w); }
      }
    }
    if (WRITE && cur >= 0) {
      c_lt = sg_wave_sum(c_lt); c_fin = sg_wave_sum(c_fin);
      s = sg_wave_sum(s); mn = sg_wave_min(mn); mx = sg_wave_max(mx);
      if (lane == 0) {
        const uint64_t at = o + k;
        SgRec q;
        q.w_sum = s; q.cnt_lt = (uint32_t)c_lt; q.n_finite = (uint32_t)c_fin; q.a = A; q.b = cur; q.w_min = mn; q.w_max = mx;
        rec[at] = q;
        const uint64_t lo = (uint64_t)(A < cur ? A : cur), hi = (uint64_t)(A < cur ? cur : A);
        rkey[at] = lo * (uint64_t)K + hi;
        ridx[at] = (uint32_t)at;
      }
      ++k;
    }
    nxt = sg_wave_min(nxt);
    if (nxt == INT_MAX) break;
    if (!WRITE) ++k;
    cur = nxt;
  }
  if (TILE && !WRITE) unk = sg_wave_sum(unk);
  if (!WRITE && lane == 0) { n_rec[r] = k; if (TILE) n_unk[r] = (uint32_t)unk; }
}

// head[i] = 1 where sorted record i starts an edge
__global__ void k_sg_heads(const uint64_t* __restrict__ key, uint32_t R, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// inc = inclusive scan of head: estart[edge] = its first sorted record, estart[E] = R; meta[1] = E
__global__ void k_sg_starts(const uint32_t* __restrict__ head, const uint32_t* __restrict__ inc, uint32_t R, uint32_t* __restrict__ estart,
                            uint32_t* __restrict__ meta) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  if (head[i]) estart[inc[i] - 1] = i;
  if (i == R - 1) { estart[inc[i]] = R; meta[1] = inc[i]; }
}

// chunks of edge e (nch[E] = 0 closes the scan)
__global__ void k_sg_nchunk(const uint32_t* __restrict__ estart, uint32_t E, uint32_t* __restrict__ nch) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e > E) return;
  nch[e] = e == E ? 0u : (estart[e + 1] - estart[e] + SG_CHUNK - 1) / SG_CHUNK;
}

// One wavefront per chunk of <= SG_CHUNK sorted records of one edge.  Grid: an upper bound of the chunks (R / SG_CHUNK + E + 1 wavefronts);
// wavefronts past the real number leave at once.
__global__ __launch_bounds__(64 * SG_WAVES) void k_sg_chunks(const uint32_t* __restrict__ ridx, const SgRec* __restrict__ rec,
                                                             const uint32_t* __restrict__ estart, const uint32_t* __restrict__ echunk, uint32_t E,
                                                             SgPart* __restrict__ part) {
  const uint32_t c = blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= echunk[E]) return;
  // edge of chunk c: the last e with echunk[e] <= c (every edge has at least one chunk)
  uint32_t lo = 0, hi = E - 1;
  while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (echunk[mid] <= c) lo = mid; else hi = mid - 1; }
  const uint32_t e = lo;
  const uint32_t a = estart[e] + (c - echunk[e]) * SG_CHUNK;
  const uint32_t b = min(a + SG_CHUNK, estart[e + 1]);
  long long np = 0, nf = 0;
  int na = 0, nb = 0;
  double s = 0.0;
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
#pragma unroll
  for (int it = 0; it < SG_PPL; ++it) {
    const uint32_t i = a + (uint32_t)it * 64 + lane;
    if (i < b) {
      const SgRec q = rec[ridx[i]];
      np += q.cnt_lt; nf += q.n_finite;
      if (q.a < q.b) ++na; else ++nb;
      s += q.w_sum; mn = fminf(mn, q.w_min); mx = fmaxf(mx, q.w_max);
    }
  }
  np = sg_wave_sum(np); nf = sg_wave_sum(nf); na = sg_wave_sum(na); nb = sg_wave_sum(nb);
  s = sg_wave_sum(s); mn = sg_wave_min(mn); mx = sg_wave_max(mx);
  if (lane == 0) {
    SgPart p;
    p.w_sum = s; p.n_pairs = np; p.n_finite = nf; p.nodes_a = na; p.nodes_b = nb; p.w_min = mn; p.w_max = mx;
    part[c] = p;
  }
}

// one wavefront per edge: fold its partials (lane stride, then butterfly), write the row on lane 0
__global__ __launch_bounds__(64 * SG_WAVES) void k_sg_final(const uint32_t* __restrict__ ridx, const SgRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ estart, const uint32_t* __restrict__ echunk,
                                                            const SgPart* __restrict__ part, uint32_t E, int32_t* __restrict__ o_ab,
                                                            int64_t* __restrict__ o_np, int64_t* __restrict__ o_nf, int32_t* __restrict__ o_nodes,
                                                            double* __restrict__ o_sum, float* __restrict__ o_min, float* __restrict__ o_max) {
  const uint32_t e = blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (e >= E) return;
  long long np = 0, nf = 0;
  int na = 0, nb = 0;
  double s = 0.0;
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
  for (uint32_t c = echunk[e] + lane; c < echunk[e + 1]; c += 64) {
    const SgPart p = part[c];
    np += p.n_pairs; nf += p.n_finite; na += p.nodes_a; nb += p.nodes_b;
    s += p.w_sum; mn = fminf(mn, p.w_min); mx = fmaxf(mx, p.w_max);
  }
  np = sg_wave_sum(np); nf = sg_wave_sum(nf); na = sg_wave_sum(na); nb = sg_wave_sum(nb);
  s = sg_wave_sum(s); mn = sg_wave_min(mn); mx = sg_wave_max(mx);
  if (lane != 0) return;
  const SgRec q = rec[ridx[estart[e]]];
  o_ab[2 * (size_t)e] = q.a < q.b ? q.a : q.b;
  o_ab[2 * (size_t)e + 1] = q.a < q.b ? q.b : q.a;
  o_np[e] = np;
  o_nf[e] = nf;
  o_nodes[2 * (size_t)e] = na;
  o_nodes[2 * (size_t)e + 1] = nb;
  o_sum[e] = s;
  o_min[e] = nf > 0 ? mn : __builtin_nanf("");
  o_max[e] = nf > 0 ? mx : __builtin_nanf("");
}


static VgsWeightParams sg_weight_params(const vgs_params& p) {   // (merge.hip: make_weight_params_m, the local cut's own parameters)
  VgsWeightParams W;
  W.inv_sig_p = 1.0f / p.sig_p; W.inv_sig_n = 1.0f / p.sig_n; W.inv_sig_o = 1.0f / p.sig_o;
  W.inv_sig_e = 1.0f / p.sig_e; W.inv_sig_c = 1.0f / p.sig_c;
  W.inv_sig_w2 = 1.0f / (p.sig_w * p.sig_w);
  W.svgs = (p.method == 3) ? 1 : 0;
  return W;
}

// The table of key space K in HBM, c->sg_E rows.  tile = false: the whole context, labels from vox_label.  tile = true: the rows of the
// owned voxels, labels from vox_label (owned) and sg_halo (others); `fn` names the caller in messages.
static vgs_status sg_build(vgs_ctx* c, int64_t K, bool tile, const char* fn) {
  const int64_t V = c->V, U = c->U;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  c->sg_E = 0;
  if (K <= 1 || U == 0 || V == 0) return VGS_OK;
  VGS_HIP_TRY(c, c->sg_lab.ensure((size_t)V));
  VGS_HIP_TRY(c, c->sg_nrec.ensure((size_t)U + 1)); VGS_HIP_TRY(c, c->sg_roff.ensure((size_t)U + 1));
  VGS_HIP_TRY(c, c->sg_meta.ensure(4));
  VGS_HIP_TRY(c, hipMemsetAsync(c->sg_meta.p, 0, 4 * sizeof(uint32_t), c->stream));
  VGS_HIP_TRY(c, hipMemsetAsync(c->sg_nrec.p + U, 0, sizeof(uint32_t), c->stream));
  const VgsWeightParams W = sg_weight_params(c->P);
  const int TB = 256;
  const unsigned rows_grid = (unsigned)((U + SG_WAVES - 1) / SG_WAVES);
  if (tile) {
    VGS_HIP_TRY(c, c->sg_nunk.ensure((size_t)U));
    hipLaunchKernelGGL(k_sg_tile_labels, dim3((unsigned)((V + TB - 1) / TB)), dim3(TB), 0, c->stream, c->vox_label.p, c->used_rank.p, c->owned.p,
                       c->sg_halo_valid ? c->sg_halo.p : (const int32_t*)nullptr, V, (int32_t)K, c->sg_lab.p, c->sg_meta.p);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sg_rows<false, true>), dim3(rows_grid), dim3(64 * SG_WAVES), 0, c->stream, c->used_ids.p, U, c->adj_key.p,
                       c->adj_cnt.p, c->adj_stride, c->used_rank.p, c->sg_lab.p, c->node.p, W, (uint32_t)K, c->sg_nrec.p, (const uint64_t*)nullptr,
                       (SgRec*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, c->sg_meta.p, c->owned.p, c->sg_nunk.p);
    size_t t_red = 0;
    VGS_HIP_TRY(c, rocprim::reduce(nullptr, t_red, c->sg_nunk.p, c->sg_meta.p + 2, 0u, (size_t)U, rocprim::plus<uint32_t>(), c->stream));
    VGS_HIP_TRY(c, c->sg_tmp.ensure(t_red));
    VGS_HIP_TRY(c, rocprim::reduce(c->sg_tmp.p, t_red, c->sg_nunk.p, c->sg_meta.p + 2, 0u, (size_t)U, rocprim::plus<uint32_t>(), c->stream));
  } else {
    hipLaunchKernelGGL(k_sg_labels, dim3((unsigned)((V + TB - 1) / TB)), dim3(TB), 0, c->stream, c->vox_label.p, c->used_rank.p, V, c->sg_lab.p);
    hipLaunchKernelGGL(k_sg_rows<false>, dim3(rows_grid), dim3(64 * SG_WAVES), 0, c->stream, c->used_ids.p, U, c->adj_key.p, c->adj_cnt.p, c->adj_stride,
                       c->used_rank.p, c->sg_lab.p, c->node.p, W, (uint32_t)K, c->sg_nrec.p, (const uint64_t*)nullptr, (SgRec*)nullptr, (uint64_t*)nullptr,
                       (uint32_t*)nullptr, c->sg_meta.p);
  }
  size_t t_scan0 = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_scan0, c->sg_nrec.p, c->sg_roff.p, (uint64_t)0, (size_t)U + 1, rocprim::plus<uint64_t>(), c->stream));
  VGS_HIP_TRY(c, c->sg_tmp.ensure(t_scan0));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sg_tmp.p, t_scan0, c->sg_nrec.p, c->sg_roff.p, (uint64_t)0, (size_t)U + 1, rocprim::plus<uint64_t>(), c->stream));
  uint64_t R64 = 0;
  VGS_READBACK(c, &R64, c->sg_roff.p + U, 8);   // read-back 1: the number of (node, neighbour label) records
  if (tile) {
    uint32_t chk[4] = {0, 0, 0, 0};
    VGS_READBACK(c, chk, c->sg_meta.p, sizeof(chk));   // (tile contexts) the label checks, before any record is written
    if (chk[3]) { c->err = std::string(fn) + ": a voxel carries a label that is not below K"; return VGS_E_ARG; }
    if (chk[2]) {
      c->err = std::string(fn) + ": " + std::to_string(chk[2]) + " entries of owned rows name a used voxel of another rank whose label no halo record brought (vgs_set_halo_labels)";
      return VGS_E_UNSUPPORTED;
    }
  }
  if (R64 == 0) return VGS_OK;
  if (R64 >= (1ull << 31)) { c->err = std::string(fn) + ": more than 2^31 (node, neighbour segment) records"; return VGS_E_UNSUPPORTED; }
  const uint32_t R = (uint32_t)R64;
  VGS_HIP_TRY(c, c->sg_rec.ensure(R));
  VGS_HIP_TRY(c, c->sg_rkey.ensure(2 * (size_t)R)); VGS_HIP_TRY(c, c->sg_ridx.ensure(2 * (size_t)R));
  VGS_HIP_TRY(c, c->sg_ework.ensure(4 * ((size_t)R + 1)));   // head, inc, estart, chunk counts / starts (E <= R)
  uint64_t *key_in = c->sg_rkey.p, *key_out = key_in + R;
  uint32_t *idx_in = c->sg_ridx.p, *idx_out = idx_in + R;
  uint32_t *head = c->sg_ework.p, *inc = head + (R + 1), *estart = inc + (R + 1), *nch = estart + (R + 1);
  if (tile)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sg_rows<true, true>), dim3(rows_grid), dim3(64 * SG_WAVES), 0, c->stream, c->used_ids.p, U, c->adj_key.p,
                       c->adj_cnt.p, c->adj_stride, c->used_rank.p, c->sg_lab.p, c->node.p, W, (uint32_t)K, (uint32_t*)nullptr, c->sg_roff.p, c->sg_rec.p,
                       key_in, idx_in, c->sg_meta.p, c->owned.p, (uint32_t*)nullptr);
  else
    hipLaunchKernelGGL(k_sg_rows<true>, dim3(rows_grid), dim3(64 * SG_WAVES), 0, c->stream, c->used_ids.p, U, c->adj_key.p, c->adj_cnt.p, c->adj_stride,
                       c->used_rank.p, c->sg_lab.p, c->node.p, W, (uint32_t)K, (uint32_t*)nullptr, c->sg_roff.p, c->sg_rec.p, key_in, idx_in, c->sg_meta.p);
  unsigned bits = 1;
  const unsigned long long kk = (unsigned long long)K * (unsigned long long)K;   // keys 0 .. K^2 - 1
  while (bits < 64 && (1ull << bits) < kk) ++bits;
  size_t t_sort = 0, t_inc = 0, t_ex = 0;
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, key_in, key_out, idx_in, idx_out, (size_t)R, 0, bits, c->stream));
  VGS_HIP_TRY(c, rocprim::inclusive_scan(nullptr, t_inc, head, inc, (size_t)R, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, t_ex, nch, nch, 0u, (size_t)R + 1, rocprim::plus<uint32_t>(), c->stream));   // (E + 1 <= R + 1)
  size_t t_max = t_sort > t_inc ? t_sort : t_inc;
  if (t_ex > t_max) t_max = t_ex;
  VGS_HIP_TRY(c, c->sg_tmp.ensure(t_max));
  VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->sg_tmp.p, t_sort, key_in, key_out, idx_in, idx_out, (size_t)R, 0, bits, c->stream));
  hipLaunchKernelGGL(k_sg_heads, dim3((R + TB - 1) / TB), dim3(TB), 0, c->stream, key_out, R, head);
  VGS_HIP_TRY(c, rocprim::inclusive_scan(c->sg_tmp.p, t_inc, head, inc, (size_t)R, rocprim::plus<uint32_t>(), c->stream));
  hipLaunchKernelGGL(k_sg_starts, dim3((R + TB - 1) / TB), dim3(TB), 0, c->stream, head, inc, R, estart, c->sg_meta.p);
  uint32_t meta[2] = {0, 0};
  VGS_READBACK(c, meta, c->sg_meta.p, sizeof(meta));   // read-back 2: the row check, E
  if (meta[0]) { c->err = std::string(fn) + ": an adjacency row holds a node whose own row lacks it (the rows are not symmetric)"; return VGS_E_UNSUPPORTED; }
  const uint32_t E = meta[1];
  VGS_HIP_TRY(c, c->sg_ab.ensure(2 * (size_t)E)); VGS_HIP_TRY(c, c->sg_nodes.ensure(2 * (size_t)E));
  VGS_HIP_TRY(c, c->sg_npairs.ensure(E)); VGS_HIP_TRY(c, c->sg_nfin.ensure(E)); VGS_HIP_TRY(c, c->sg_wsum.ensure(E));
  VGS_HIP_TRY(c, c->sg_wmin.ensure(E)); VGS_HIP_TRY(c, c->sg_wmax.ensure(E));
  uint32_t* echunk = head;   // (head is free once estart is written; E + 1 <= R + 1 entries)
  hipLaunchKernelGGL(k_sg_nchunk, dim3((E + 1 + TB - 1) / TB), dim3(TB), 0, c->stream, estart, E, nch);
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sg_tmp.p, t_ex, nch, echunk, 0u, (size_t)E + 1, rocprim::plus<uint32_t>(), c->stream));
  // sum over edges of ceil(n_e / SG_CHUNK) <= R / SG_CHUNK + E: launched without reading the real number back
  const uint32_t n_chunks_max = R / SG_CHUNK + E + 1;
  VGS_HIP_TRY(c, c->sg_part.ensure(n_chunks_max));
  hipLaunchKernelGGL(k_sg_chunks, dim3((n_chunks_max + SG_WAVES - 1) / SG_WAVES), dim3(64 * SG_WAVES), 0, c->stream, idx_out, c->sg_rec.p, estart, echunk, E,
                     c->sg_part.p);
  hipLaunchKernelGGL(k_sg_final, dim3((E + SG_WAVES - 1) / SG_WAVES), dim3(64 * SG_WAVES), 0, c->stream, idx_out, c->sg_rec.p, estart, echunk, c->sg_part.p,
                     E, c->sg_ab.p, c->sg_npairs.p, c->sg_nfin.p, c->sg_nodes.p, c->sg_wsum.p, c->sg_wmin.p, c->sg_wmax.p);
  VGS_HIP_TRY(c, hipGetLastError());
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->sg_E = E;
  return VGS_OK;
}

// The table in HBM, c->sg_E rows; valid until the next run of the stages.
vgs_status vgs_seggraph_on_device(vgs_ctx* c) {
  if (c->sg_valid) return VGS_OK;
  const vgs_status s = sg_build(c, c->counts[VGS_N_KEPT], false, "vgs_get_segment_graph");
  if (s == VGS_OK) c->sg_valid = true;
  return s;
}

// copies of the table's E rows to the caller's arrays (any may be NULL)
static vgs_status sg_download(vgs_ctx* c, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab, double* w_sum, float* w_min,
                              float* w_max) {
  const size_t E = (size_t)c->sg_E;
  if (E == 0) return VGS_OK;
  if (seg_ab) VGS_HIP_TRY(c, hipMemcpy(seg_ab, c->sg_ab.p, 2 * E * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (n_pairs) VGS_HIP_TRY(c, hipMemcpy(n_pairs, c->sg_npairs.p, E * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (n_finite) VGS_HIP_TRY(c, hipMemcpy(n_finite, c->sg_nfin.p, E * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (nodes_ab) VGS_HIP_TRY(c, hipMemcpy(nodes_ab, c->sg_nodes.p, 2 * E * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (w_sum) VGS_HIP_TRY(c, hipMemcpy(w_sum, c->sg_wsum.p, E * sizeof(double), hipMemcpyDeviceToHost));
  if (w_min) VGS_HIP_TRY(c, hipMemcpy(w_min, c->sg_wmin.p, E * sizeof(float), hipMemcpyDeviceToHost));
  if (w_max) VGS_HIP_TRY(c, hipMemcpy(w_max, c->sg_wmax.p, E * sizeof(float), hipMemcpyDeviceToHost));
  return VGS_OK;
}

static vgs_status sg_check(vgs_ctx* c, const char* fn) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of its segments; the segment graph needs the whole cloud in one context";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

extern "C" vgs_status vgs_get_segment_graph(vgs_ctx* c, int64_t* n_edges, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                            double* w_sum, float* w_min, float* w_max) {
  if (!c || !n_edges) return VGS_E_ARG;
  *n_edges = 0;
  vgs_status s = sg_check(c, "vgs_get_segment_graph");
  if (s != VGS_OK) return s;
  if ((s = vgs_seggraph_on_device(c)) != VGS_OK) return s;
  *n_edges = c->sg_E;
  return sg_download(c, seg_ab, n_pairs, n_finite, nodes_ab, w_sum, w_min, w_max);
}

extern "C" vgs_status vgs_get_segment_graph_device(vgs_ctx* c, int64_t* n_edges, const int32_t** seg_ab, const int64_t** n_pairs, const int64_t** n_finite,
                                                   const int32_t** nodes_ab, const double** w_sum, const float** w_min, const float** w_max) {
  if (!c || !n_edges) return VGS_E_ARG;
  *n_edges = 0;
  vgs_status s = sg_check(c, "vgs_get_segment_graph_device");
  if (s != VGS_OK) return s;
  if ((s = vgs_seggraph_on_device(c)) != VGS_OK) return s;
  *n_edges = c->sg_E;
  if (seg_ab) *seg_ab = c->sg_ab.p;
  if (n_pairs) *n_pairs = c->sg_npairs.p;
  if (n_finite) *n_finite = c->sg_nfin.p;
  if (nodes_ab) *nodes_ab = c->sg_nodes.p;
  if (w_sum) *w_sum = c->sg_wsum.p;
  if (w_min) *w_min = c->sg_wmin.p;
  if (w_max) *w_max = c->sg_wmax.p;
  return VGS_OK;
}

// ---- tile contexts ---------------------------------------------------------------------------------------------------------------
vgs_status vgs_halo_find(vgs_ctx* c, const uint64_t* code_dev, const int32_t* label_dev, int64_t n, int32_t* halo_dev) {
  if (n <= 0 || c->V == 0) return VGS_OK;
  hipLaunchKernelGGL(k_sg_halo_find, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, code_dev, label_dev, n, c->vox_code.p, c->V, c->owned.p,
                     halo_dev);
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}

static vgs_status sg_tile_check(vgs_ctx* c, const char* fn) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (!c->have_region || c->n_own < 0) {
    c->err = std::string(fn) + ": a tile context (vgs_set_owned_region and vgs_set_own_point_range) only";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

extern "C" vgs_status vgs_set_halo_labels(vgs_ctx* c, const uint64_t* code, const int32_t* label, int64_t n) {
  if (!c || n < 0 || (n > 0 && (!code || !label))) return VGS_E_ARG;
  vgs_status s = sg_tile_check(c, "vgs_set_halo_labels");
  if (s != VGS_OK) return s;
  for (int64_t k = 0; k < n; ++k)
    if (label[k] < -1) { c->err = "vgs_set_halo_labels: a label below -1"; return VGS_E_ARG; }
  c->sg_halo_valid = false; c->sg_own_K = -1;
  const int64_t V = c->V;
  if (V == 0) { c->sg_halo_valid = true; return VGS_OK; }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  VGS_HIP_TRY(c, c->sg_halo.ensure((size_t)V));
  VGS_HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)c->sg_halo.p, SG_UNKNOWN, (size_t)V, c->stream));
  if (n > 0) {
    VGS_HIP_TRY(c, c->sg_hcode.ensure((size_t)n)); VGS_HIP_TRY(c, c->sg_hlab.ensure((size_t)n));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->sg_hcode.p, code, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->sg_hlab.p, label, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((s = vgs_halo_find(c, c->sg_hcode.p, c->sg_hlab.p, n, c->sg_halo.p)) != VGS_OK) return s;
  }
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the upload reads the caller's arrays)
  c->sg_halo_valid = true;
  return VGS_OK;
}

extern "C" vgs_status vgs_get_own_segment_graph(vgs_ctx* c, int64_t K, int64_t* n_edges, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite,
                                                int32_t* nodes_ab, double* w_sum, float* w_min, float* w_max) {
  if (!c || !n_edges || K < 0 || K >= (int64_t)0x7fffffffLL) return VGS_E_ARG;
  *n_edges = 0;
  vgs_status s = sg_tile_check(c, "vgs_get_own_segment_graph");
  if (s != VGS_OK) return s;
  const bool query = !seg_ab && !n_pairs && !n_finite && !nodes_ab && !w_sum && !w_min && !w_max;
  if (query || c->sg_own_K != K) {   // two-call protocol: the size query computes, the call with arrays copies that table
    c->sg_own_K = -1;
    if ((s = sg_build(c, K, true, "vgs_get_own_segment_graph")) != VGS_OK) return s;
    c->sg_own_K = K;
  }
  *n_edges = c->sg_E;
  return sg_download(c, seg_ab, n_pairs, n_finite, nodes_ab, w_sum, w_min, w_max);
}
