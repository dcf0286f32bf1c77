// refine.hip -- point-level label refinement at segment boundaries (include/vgs.h: vgs_refine_point_labels; no reference counterpart).
//
// A point's label is the label of its node, so segment boundaries are staircases of whole nodes and the points of unused voxels and of
// dropped clusters are -1.  The rule of include/vgs.h gives every point of a node v the label of the candidate node -- v itself or one
// of its adjacency row, used, labelled, with a valid position and normal -- whose planar patch (vm_refine_cost, csrc/vgs_math.h) lies
// nearest, if that beats v's own label by switch_ratio; an unlabelled point takes the nearest candidate's label outright (fill).
//
// Data flow, everything from what vgs_segment left in HBM:
//   1. k_rf_init: every point takes A of its node (vox_label for a used node, -1 otherwise and outside every node), written through the
//      engine's permutation into rf_label in input order.  Interior nodes -- all candidates carry the node's own label -- are done.
//   2. k_rf_mark, one wavefront per listed node: does the row hold a candidate of another label (for an unlabelled node: any candidate)?
//      Such a WORKING node gets ceil(points / RF_BATCH) batches, the others none; an exclusive scan turns the batch counts into the first
//      work item of every node, so a ground voxel of thousands of points spreads over workgroups like any other.
//   3. k_rf_refine, one wavefront per item (node, batch): the node's candidates (centroid, normal, label, id) go through LDS in chunks
//      of RF_CH -- a row may hold 8192 entries -- every lane reads each staged candidate at the same address (a broadcast) and keeps the
//      running (best cost, best id, best label, c_own) of its RF_PPT points across the chunks; the result overwrites rf_label.
// The listed nodes and their rows: the used nodes with the stored rows (adj_key / adj_cnt by used rank; pruned to used neighbours or not,
// both are fine since candidates are used) -- and, for VGS with fill, the unused voxels, whose rows the hot path does not keep: they are
// compacted into a list and their rows built a chunk at a time by the adjacency stage's own pass (vgs_run_adjacency over a list of ids).
// Every supervoxel is used (SS:1288), so SVGS has no second list.
//
// Determinism: every point is written by exactly one lane of one item (after k_rf_init, in stream order), minima over (cost, id) do not
// depend on the order of the candidates, and the four counts are integer sums: bit-identical from call to call.
//
// Tile contexts: the rule over the whole scene, this rank's share (include/vgs_tiles.h: vgs_tiles_refine_point_labels).  A rank refines the
// nodes that hold points of its own load and whose centre lies at most RF reach = max(graph_size, 0.5001 voxel_size) outside its region,
// per axis -- the nodes it owns, those whose cube crosses its border, and those of objects that reach over a tile's edge
// (scenes.tiled_urban_scene hands a rank points up to 0.4 m beyond its region).  Their rows are complete here and carry the owner's node
// records: the candidates lie within graph_size of the centre, so their cubes end within 2 graph_size + 0.5 voxel_size of the border,
// inside the halo of 2 graph_size + voxel_size.  What differs from the single context:
//   * labels come from a table of EFFECTIVE labels (k_rf_tile_labels): vox_label for an owned used voxel, the refinement's own halo table
//     (vgs_set_refine_halo_labels; RF_UNKNOWN without a record) for a used voxel of another rank, -1 for an unused one;
//   * a point takes part only when it is of the rank's own load; points of other ranks' strips are left to their ranks;
//   * a working node is counted by its owner, so the mark pass also looks at owned nodes without own points (no batches for them);
//   * own points of any other node (loaded further beyond the region than that) keep their point label and are counted.
// The mark kernel, the refine kernel, the pass and the fill driver are each written once; that list is what their TILE branches do, and
// k_rf_mark / k_rf_tile_mark and k_rf_refine / k_rf_tile_refine are the two entry points of one body each.  The single context reads
// vox_label directly and has neither the table of effective labels nor the mask.
#include <string.h>

#include <algorithm>
#include <cmath>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "tile_region.hpp"

#define RF_TB 64                      // one wavefront per work item
#define RF_PPT 4                      // points per lane
#define RF_BATCH (RF_TB * RF_PPT)     // points per work item
#define RF_CH 256                     // candidates staged per chunk (two float4 each: 8 KB of LDS)
#define RF_UNKNOWN (-2)               // effective label of a used voxel of another rank whose label no record brought
#define RF_M_REFINE 1u   // mask bit 0: holds own points and lies within reach of the region: this rank refines it
#define RF_M_OWNED 2u    // mask bit 1: owned: this rank counts it when it is a working node

// A of the rule: the kept label of a used node, -1 otherwise
__device__ __forceinline__ int32_t rf_node_label(const NodeRec* __restrict__ node, const int32_t* __restrict__ vox_label, uint32_t v) {
  return (node[v].flags & VGS_F_EIG) ? vox_label[v] : -1;
}
// the label w brings as a candidate, -1 when it is none; lab is vox_label, or the effective labels of a tile, where a candidate whose
// label no record brought answers RF_UNKNOWN
template <bool TILE>
__device__ __forceinline__ int32_t rf_cand_label(uint32_t flags, const int32_t* __restrict__ lab, uint32_t w) {
  const uint32_t need = VGS_F_EIG | VGS_F_POS | VGS_F_NRM;
  if ((flags & need) != need) return -1;
  const int32_t l = lab[w];
  return (l >= 0 || (TILE && l == RF_UNKNOWN)) ? l : -1;
}

__global__ void k_rf_init(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pt_vox, const NodeRec* __restrict__ node,
                          const int32_t* __restrict__ vox_label, int64_t N, int32_t* __restrict__ label) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const uint32_t v = pt_vox[j];
  label[perm[j]] = (v == 0xffffffffu) ? -1 : rf_node_label(node, vox_label, v);
}

// the voxels without a stored row, as a flag per voxel and (behind the scan) as a list; with a mask (a tile) only those the mark pass
// lists with fill: refinable or owned (an owned one without own points is only counted)
__global__ void k_rf_unused_flags(const uint32_t* __restrict__ used_rank, const uint8_t* __restrict__ mask, int64_t V, uint32_t* __restrict__ flag) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V) flag[v] = (used_rank[v] == 0xffffffffu && (!mask || mask[v] != 0)) ? 1u : 0u;
}
__global__ void k_rf_unused_list(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, int64_t V, uint32_t cap,
                                 uint32_t* __restrict__ ids) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V && flag[v] && excl[v] < cap) ids[excl[v]] = (uint32_t)v;   // (cap = the number of flags: the bound only guards the list)
}

// one wavefront per listed node i: node ids[i], row rows + i * stride of cnt[i] entries.  lab: vox_label, or the effective labels of a
// tile (TILE), where counts[0] is the owner's, batches are made for refinable nodes only and counts[5] = candidates of unknown label
template <bool TILE>
__device__ __forceinline__ void rf_mark_body(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                             uint32_t n, int stride, const NodeRec* __restrict__ node, const int32_t* __restrict__ lab,
                                             const uint8_t* __restrict__ mask, const uint32_t* __restrict__ vox_start, int fill,
                                             uint32_t* __restrict__ batches, unsigned long long* __restrict__ counts) {
  const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n) return;   // (whole wavefronts; no barrier follows)
  const uint32_t v = ids[i];
  uint32_t mk = RF_M_REFINE | RF_M_OWNED;
  if (TILE) {
    mk = mask[v];
    if (mk == 0) { if (lane == 0) batches[i] = 0u; return; }   // a voxel of the halo that this rank neither refines nor counts
  }
  const int32_t A = TILE ? lab[v] : rf_node_label(node, lab, v);
  bool hit = false;
  uint32_t unk = 0;
  if (A >= 0 || fill) {
    const uint32_t m = min(cnt[i], (uint32_t)stride);
    const uint64_t* row = rows + (size_t)i * stride;
    for (uint32_t k = lane; k <= m; k += 64) {   // entry m: the node itself
      const uint32_t w = k < m ? (uint32_t)row[k] : v;
      const int32_t L = rf_cand_label<TILE>(node[w].flags, lab, w);
      if (TILE) unk += (L == RF_UNKNOWN || (k == m && A == RF_UNKNOWN)) ? 1u : 0u;   // (the node's own label, whatever its flags)
      hit = hit || (L >= 0 && L != A);
    }
  } else if (TILE && lane == 0 && A == RF_UNKNOWN) unk = 1u;   // (not -1: a used node of another rank without a record)
  const bool work = __ballot(hit) != 0ull;
  if (TILE) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) unk += __shfl_xor(unk, o, 64);
  }
  if (lane != 0) return;
  const uint32_t npts = vox_start[v + 1] - vox_start[v];
  batches[i] = (work && (mk & RF_M_REFINE)) ? (npts + RF_BATCH - 1) / RF_BATCH : 0u;
  if (work && (mk & RF_M_OWNED)) atomicAdd(&counts[0], 1ull);
  if (!TILE && work) atomicAdd(&counts[1], (unsigned long long)npts);   // (a tile counts the points it examines: rf_refine_body)
  if (TILE && unk) atomicAdd(&counts[5], (unsigned long long)unk);
}

__global__ __launch_bounds__(256) void k_rf_mark(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                                 uint32_t n, int stride, const NodeRec* __restrict__ node, const int32_t* __restrict__ vox_label,
                                                 const uint32_t* __restrict__ vox_start, int fill, uint32_t* __restrict__ batches,
                                                 unsigned long long* __restrict__ counts) {
  rf_mark_body<false>(ids, rows, cnt, n, stride, node, vox_label, nullptr, vox_start, fill, batches, counts);
}

__global__ __launch_bounds__(256) void k_rf_tile_mark(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                                      uint32_t n, int stride, const NodeRec* __restrict__ node, const int32_t* __restrict__ eff,
                                                      const uint8_t* __restrict__ mask, const uint32_t* __restrict__ vox_start, int fill,
                                                      uint32_t* __restrict__ batches, unsigned long long* __restrict__ counts) {
  rf_mark_body<true>(ids, rows, cnt, n, stride, node, eff, mask, vox_start, fill, batches, counts);
}

// one wavefront per work item (node, batch).  lab: vox_label, or the effective labels of a tile (TILE), where a lane's point takes part
// only if it is of the rank's own load [own_first, own_first + n_own) and the points that do are counted here (counts[1])
template <bool TILE>
__device__ __forceinline__ void rf_refine_body(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                               uint32_t n, int stride, const uint32_t* __restrict__ start, const NodeRec* __restrict__ node,
                                               const int32_t* __restrict__ lab, const uint32_t* __restrict__ vox_start,
                                               const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                               const uint32_t* __restrict__ perm, int64_t own_first, int64_t n_own, float patch_radius,
                                               float switch_ratio, int32_t* __restrict__ label, unsigned long long* __restrict__ counts) {
  __shared__ float4 s_a[RF_CH];   // centroid | label
  __shared__ float4 s_b[RF_CH];   // normal | node id
  const uint32_t t = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (t >= start[n]) return;   // (the whole workgroup)
  // the node of item t: the last i with start[i] <= t (a node without batches shares its start with the next one)
  uint32_t lo = 0, hi = n - 1;
  while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (start[mid] <= t) lo = mid; else hi = mid - 1; }
  const uint32_t i = lo;
  const uint32_t v = ids[i];
  const int32_t A = TILE ? max(lab[v], -1) : rf_node_label(node, lab, v);
  const uint32_t p0 = vox_start[v] + (t - start[i]) * RF_BATCH;
  const uint32_t p1 = min(vox_start[v + 1], p0 + RF_BATCH);
  float p[RF_PPT][3], best[RF_PPT], cown[RF_PPT];
  uint32_t bid[RF_PPT];
  int32_t blab[RF_PPT];
  const float inf = vm_from_bits(0x7f800000u);
#pragma unroll
  for (int k = 0; k < RF_PPT; ++k) {
    const uint32_t j = p0 + k * RF_TB + lane;
    const bool in = j < p1;
    p[k][0] = in ? xs[j] : 0.f; p[k][1] = in ? ys[j] : 0.f; p[k][2] = in ? zs[j] : 0.f;
    best[k] = inf; cown[k] = inf; bid[k] = 0xffffffffu; blab[k] = -1;
  }
  const uint32_t m = min(cnt[i], (uint32_t)stride);
  const uint64_t* row = rows + (size_t)i * stride;
  // m + 1 entries: the row, then the node itself.  A stored row of VGS and SVGS already starts with its own node, so a used node is
  // evaluated twice -- the same (cost, id), harmless to the minima, one candidate of wasted work per item; the row of an unused voxel
  // (used neighbours only) and the rule's "v itself" for any row layout are why the entry is there.  Every batch of a node stages the
  // row again: a voxel of 5 000 points stages it 20 times (rows are a few hundred entries; not measured as a cost worth a second level)
  for (uint32_t c0 = 0; c0 <= m; c0 += RF_CH) {
    const uint32_t nc = min((uint32_t)RF_CH, m + 1 - c0);
    __syncthreads();
    for (uint32_t e = lane; e < nc; e += RF_TB) {
      const uint32_t k = c0 + e;
      const uint32_t w = k < m ? (uint32_t)row[k] : v;
      const NodeRec* r = node + w;
      const int32_t L = max(rf_cand_label<TILE>(r->flags, lab, w), -1);   // (an unknown label fails the call: rf_mark_body counted it)
      s_a[e] = make_float4(r->c[0], r->c[1], r->c[2], __int_as_float(L));
      s_b[e] = make_float4(r->n[0], r->n[1], r->n[2], __uint_as_float(w));
    }
    __syncthreads();
    for (uint32_t e = 0; e < nc; ++e) {
      const float4 a = s_a[e];
      const int32_t L = __float_as_int(a.w);
      if (L < 0) continue;   // (the same for every lane)
      const float4 b = s_b[e];
      const uint32_t w = __float_as_uint(b.w);
      const float cc[3] = {a.x, a.y, a.z}, nn[3] = {b.x, b.y, b.z};
#pragma unroll
      for (int k = 0; k < RF_PPT; ++k) {
        const float cost = vm_refine_cost(p[k], cc, nn, patch_radius);
        if (!vm_isfinite(cost)) continue;
        if (cost < best[k] || (cost == best[k] && w < bid[k])) { best[k] = cost; bid[k] = w; blab[k] = L; }
        if (L == A && cost < cown[k]) cown[k] = cost;
      }
    }
  }
  unsigned long long n_exam = 0, n_changed = 0, n_filled = 0;
#pragma unroll
  for (int k = 0; k < RF_PPT; ++k) {
    const uint32_t j = p0 + k * RF_TB + lane;
    bool in = j < p1;
    const uint32_t dst = in ? perm[j] : 0u;   // the point's input index
    if (TILE) in = in && (int64_t)dst >= own_first && (int64_t)dst < own_first + n_own;
    int32_t out = A;
    if (A >= 0) { if (cown[k] < inf && best[k] < switch_ratio * cown[k]) out = blab[k]; }
    else out = blab[k];   // (an unlabelled node is listed with fill only)
    if (in) label[dst] = out;
    if (TILE) n_exam += (unsigned long long)__popcll(__ballot(in));
    n_changed += (unsigned long long)__popcll(__ballot(in && A >= 0 && out != A));
    n_filled += (unsigned long long)__popcll(__ballot(in && A < 0 && out >= 0));
  }
  if (lane == 0) {
    if (n_exam) atomicAdd(&counts[1], n_exam);   // (a tile only: k_rf_mark has counted a single context's)
    if (n_changed) atomicAdd(&counts[2], n_changed);
    if (n_filled) atomicAdd(&counts[3], n_filled);
  }
}

__global__ __launch_bounds__(RF_TB) void k_rf_refine(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                                     uint32_t n, int stride, const uint32_t* __restrict__ start, const NodeRec* __restrict__ node,
                                                     const int32_t* __restrict__ vox_label, const uint32_t* __restrict__ vox_start,
                                                     const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                     const uint32_t* __restrict__ perm, float patch_radius, float switch_ratio,
                                                     int32_t* __restrict__ label, unsigned long long* __restrict__ counts) {
  rf_refine_body<false>(ids, rows, cnt, n, stride, start, node, vox_label, vox_start, xs, ys, zs, perm, 0, 0, patch_radius, switch_ratio, label, counts);
}

__global__ __launch_bounds__(RF_TB) void k_rf_tile_refine(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                                          uint32_t n, int stride, const uint32_t* __restrict__ start, const NodeRec* __restrict__ node,
                                                          const int32_t* __restrict__ eff, const uint32_t* __restrict__ vox_start,
                                                          const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                          const uint32_t* __restrict__ perm, int64_t own_first, int64_t n_own, float patch_radius,
                                                          float switch_ratio, int32_t* __restrict__ label, unsigned long long* __restrict__ counts) {
  rf_refine_body<true>(ids, rows, cnt, n, stride, start, node, eff, vox_start, xs, ys, zs, perm, own_first, n_own, patch_radius, switch_ratio, label, counts);
}

// exclusive scan of n counts (flags, batches: in rf_batches, n + 1 entries allocated) into rf_start; the total is read back unless the
// caller knows it (total == nullptr)
static vgs_status rf_scan_flags(vgs_ctx* c, size_t n, uint32_t* total) {
  VGS_HIP_TRY(c, hipMemsetAsync(c->rf_batches.p + n, 0, 4, c->stream));
  size_t bytes = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, c->rf_batches.p, c->rf_start.p, 0u, n + 1, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, c->sort_tmp.ensure(bytes));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sort_tmp.p, bytes, c->rf_batches.p, c->rf_start.p, 0u, n + 1, rocprim::plus<uint32_t>(), c->stream));
  if (total) VGS_READBACK(c, total, c->rf_start.p + n, 4);
  return VGS_OK;
}

// mark, scan and refine one list of nodes with their rows; tile: over the effective labels and the mask, for the rank's own points
static vgs_status rf_pass(vgs_ctx* c, bool tile, const uint32_t* ids, const uint64_t* rows, const uint32_t* cnt, int64_t n, const vgs_refine_params& rp) {
  if (n <= 0) return VGS_OK;
  VGS_HIP_TRY(c, c->rf_batches.ensure((size_t)n + 1)); VGS_HIP_TRY(c, c->rf_start.ensure((size_t)n + 1));
  unsigned long long* counts = (unsigned long long*)c->rf_counts.p;
  const int32_t* lab = tile ? c->rf_eff.p : c->vox_label.p;
  const dim3 nb_mark((unsigned)((n + 3) / 4));
  if (tile)
    hipLaunchKernelGGL(k_rf_tile_mark, nb_mark, dim3(256), 0, c->stream, ids, rows, cnt, (uint32_t)n, c->adj_stride, c->node.p, lab, c->rf_mask.p,
                       c->vox_start.p, rp.fill ? 1 : 0, c->rf_batches.p, counts);
  else
    hipLaunchKernelGGL(k_rf_mark, nb_mark, dim3(256), 0, c->stream, ids, rows, cnt, (uint32_t)n, c->adj_stride, c->node.p, lab, c->vox_start.p,
                       rp.fill ? 1 : 0, c->rf_batches.p, counts);
  uint32_t n_items = 0;
  vgs_status s = rf_scan_flags(c, (size_t)n, &n_items);
  if (s != VGS_OK) return s;
  if (n_items > 0 && tile)
    hipLaunchKernelGGL(k_rf_tile_refine, dim3(n_items), dim3(RF_TB), 0, c->stream, ids, rows, cnt, (uint32_t)n, c->adj_stride, c->rf_start.p, c->node.p,
                       lab, c->vox_start.p, c->xs.p, c->ys.p, c->zs.p, c->perm_b.p, c->own_first, c->n_own, rp.patch_radius, rp.switch_ratio,
                       c->rf_label.p, counts);
  else if (n_items > 0)
    hipLaunchKernelGGL(k_rf_refine, dim3(n_items), dim3(RF_TB), 0, c->stream, ids, rows, cnt, (uint32_t)n, c->adj_stride, c->rf_start.p, c->node.p,
                       lab, c->vox_start.p, c->xs.p, c->ys.p, c->zs.p, c->perm_b.p, rp.patch_radius, rp.switch_ratio, c->rf_label.p, counts);
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}

// fill: list the unused voxels -- all V - U of them, or in a tile the refinable or owned ones, whose number is read back -- build their
// rows, used neighbours only, a chunk of at most 256 MB of keys at a time, and pass over each chunk
static vgs_status rf_fill(vgs_ctx* c, bool tile, const vgs_refine_params& rp) {
  const int64_t V = c->V;
  const int TB = 256;
  const unsigned nbV = (unsigned)((V + TB - 1) / TB);
  VGS_HIP_TRY(c, c->rf_batches.ensure((size_t)V + 1)); VGS_HIP_TRY(c, c->rf_start.ensure((size_t)V + 1));
  hipLaunchKernelGGL(k_rf_unused_flags, dim3(nbV), dim3(TB), 0, c->stream, c->used_rank.p, tile ? c->rf_mask.p : nullptr, V, c->rf_batches.p);
  uint32_t n_list = (uint32_t)(V - c->U);
  vgs_status s = rf_scan_flags(c, (size_t)V, tile ? &n_list : nullptr);
  if (s != VGS_OK) return s;
  if (n_list == 0) return VGS_OK;
  VGS_HIP_TRY(c, c->rf_ids.ensure((size_t)n_list));
  hipLaunchKernelGGL(k_rf_unused_list, dim3(nbV), dim3(TB), 0, c->stream, c->rf_batches.p, c->rf_start.p, V, n_list, c->rf_ids.p);
  VGS_HIP_TRY(c, hipGetLastError());
  const int64_t n_un = (int64_t)n_list;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_un, ((int64_t)32 << 20) / std::max(1, c->adj_stride)));
  VGS_HIP_TRY(c, c->rf_rows.ensure((size_t)chunk * c->adj_stride)); VGS_HIP_TRY(c, c->rf_cnt.ensure((size_t)chunk)); VGS_HIP_TRY(c, c->rf_nall.ensure((size_t)chunk));
  for (int64_t o = 0; o < n_un; o += chunk) {
    const int64_t m = std::min(chunk, n_un - o);
    s = vgs_run_adjacency(c, false, c->rf_rows.p, c->rf_cnt.p, c->rf_nall.p, c->adj_r2, c->rf_ids.p + o, m);
    if (s != VGS_OK) return s;
    if ((s = rf_pass(c, tile, c->rf_ids.p + o, c->rf_rows.p, c->rf_cnt.p, m, rp)) != VGS_OK) return s;
  }
  return VGS_OK;
}

vgs_status vgs_refine_on_device(vgs_ctx* c, const vgs_refine_params& rp, int64_t* counts4) {
  c->rf_valid = false;
  const int64_t N = c->N, V = c->V, U = c->U, nf = c->Nf;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  VGS_HIP_TRY(c, c->rf_label.ensure(N > 0 ? (size_t)N : 1)); VGS_HIP_TRY(c, c->rf_counts.ensure(4));
  VGS_HIP_TRY(c, hipMemsetAsync(c->rf_counts.p, 0, 4 * sizeof(uint64_t), c->stream));
  const int TB = 256;
  if (N > 0 && (V == 0 || nf == 0)) {   // no node: every point keeps -1 (the voxelize stage wrote neither the order nor the map)
    VGS_HIP_TRY(c, hipMemsetAsync(c->rf_label.p, 0xff, (size_t)N * sizeof(int32_t), c->stream));
  } else if (N > 0) {
    hipLaunchKernelGGL(k_rf_init, dim3((unsigned)((N + TB - 1) / TB)), dim3(TB), 0, c->stream, c->perm_b.p, c->pt_vox.p, c->node.p, c->vox_label.p, N,
                       c->rf_label.p);
    vgs_status s = rf_pass(c, false, c->used_ids.p, c->adj_key.p, c->adj_cnt.p, U, rp);
    if (s != VGS_OK) return s;
    if (c->P.method == 2 && rp.fill && V - U > 0 && U > 0)   // (without a used voxel there is no candidate anywhere)
      if ((s = rf_fill(c, false, rp)) != VGS_OK) return s;
  }
  uint64_t h[4] = {0, 0, 0, 0};
  VGS_READBACK(c, h, c->rf_counts.p, sizeof(h));
  if (counts4) for (int k = 0; k < 4; ++k) counts4[k] = (int64_t)h[k];
  c->rf_valid = true;
  return VGS_OK;
}

// ---- tile contexts ---------------------------------------------------------------------------------------------------------------
// the region of a tile and its grid, as k_owned (multigpu.hip) takes them: the centre of a voxel is a function of its global code and the
// shared grid only, so every rank computes the same one
// (RfRegion, rf_center, rf_region: tile_region.hpp, shared with labelcc_tiles.hip)

// the band: owned used voxels whose centre lies within `near` of a border line of the region -- what a neighbour can reach from a node it
// refines -- as a flag per voxel and (behind the scan) as records in ascending voxel id
__global__ void k_rf_band_flags(const uint64_t* __restrict__ vox_code, const uint8_t* __restrict__ owned, const uint32_t* __restrict__ used_rank, int64_t V,
                                RfRegion g, double near, uint32_t* __restrict__ flag) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  double cx, cy;
  rf_center(g, vox_code[v], cx, cy);
  const bool nr = fabs(cx - g.lo_x) < near || fabs(cx - g.hi_x) < near || fabs(cy - g.lo_y) < near || fabs(cy - g.hi_y) < near;
  flag[v] = (nr && owned[v] && used_rank[v] != 0xffffffffu) ? 1u : 0u;
}
__global__ void k_rf_band_compact(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, int64_t V, const uint64_t* __restrict__ vox_code,
                                  const int32_t* __restrict__ vox_label, uint64_t* __restrict__ code, int32_t* __restrict__ label) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V && flag[v]) { code[excl[v]] = vox_code[v]; label[excl[v]] = vox_label[v]; }   // (excl[v] < excl[V], the size of both arrays)
}

// one pass over V: the effective label and the mask of every voxel.  reach = 0.5001 voxel_size would be the geometric part of k_owned's
// straddle bit 0 (multigpu.hip): the cube crosses the border.
__global__ void k_rf_tile_labels(const uint64_t* __restrict__ vox_code, const NodeRec* __restrict__ node, const int32_t* __restrict__ vox_label,
                                 const uint8_t* __restrict__ owned, const uint8_t* __restrict__ mix, const int32_t* __restrict__ halo, int64_t V,
                                 RfRegion g, double reach, int32_t* __restrict__ eff, uint8_t* __restrict__ mask) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const bool own = owned[v] != 0;
  eff[v] = (node[v].flags & VGS_F_EIG) ? (own ? vox_label[v] : halo[v]) : -1;
  double cx, cy;
  rf_center(g, vox_code[v], cx, cy);
  const double dx = fmax(fmax(g.lo_x - cx, cx - g.hi_x), 0.0), dy = fmax(fmax(g.lo_y - cy, cy - g.hi_y), 0.0);   // outside the region by, per axis
  const bool within = own || (dx <= reach && dy <= reach);
  const bool mine = mix && mix[v] != 0;
  mask[v] = (uint8_t)((mine && within ? RF_M_REFINE : 0u) | (own ? RF_M_OWNED : 0u));
}

// own points only: A of a refinable node, the point label elsewhere (counts[4]); -1 outside every node
__global__ __launch_bounds__(256) void k_rf_tile_init(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pt_vox,
                                                      const int32_t* __restrict__ eff, const uint8_t* __restrict__ mask,
                                                      const int32_t* __restrict__ pt_label, int64_t N, int64_t own_first, int64_t n_own,
                                                      int32_t* __restrict__ label, unsigned long long* __restrict__ counts) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool beyond = false;
  if (j < N) {
    const int64_t i = (int64_t)perm[j];
    if (i >= own_first && i < own_first + n_own) {
      const uint32_t v = pt_vox[j];
      int32_t out = -1;
      if (v != 0xffffffffu) {
        if (mask[v] & RF_M_REFINE) out = max(eff[v], -1);
        else { out = pt_label[i]; beyond = true; }
      }
      label[i] = out;
    }
  }
  const unsigned long long nb = (unsigned long long)__popcll(__ballot(beyond));
  if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&counts[4], nb);
}

// how far outside its region a rank still refines a node, per axis; the band of the other ranks reaches graph_size further (a candidate
// lies within graph_size of the node) and half a voxel more, so that no rounding of a centre decides
static double rf_reach(const vgs_ctx* c) { return std::max((double)c->P.graph_size, 0.5001 * (double)c->P.voxel_size); }
static double rf_band_near(const vgs_ctx* c) { return rf_reach(c) + (double)c->P.graph_size + 0.5 * (double)c->P.voxel_size; }

vgs_status vgs_refine_own_on_device(vgs_ctx* c, const vgs_refine_params& rp, int64_t* counts5) {
  c->rf_valid = false;
  const int64_t N = c->N, V = c->V, U = c->U, nf = c->Nf;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  VGS_HIP_TRY(c, c->rf_label.ensure(N > 0 ? (size_t)N : 1)); VGS_HIP_TRY(c, c->rf_counts.ensure(8));
  VGS_HIP_TRY(c, hipMemsetAsync(c->rf_counts.p, 0, 8 * sizeof(uint64_t), c->stream));
  // -1 everywhere first: the points of other ranks' strips are never written by a kernel, and a cloud without a node keeps -1
  if (N > 0) VGS_HIP_TRY(c, hipMemsetAsync(c->rf_label.p, 0xff, (size_t)N * sizeof(int32_t), c->stream));
  const int TB = 256;
  if (N > 0 && V > 0 && nf > 0) {
    VGS_HIP_TRY(c, c->rf_eff.ensure((size_t)V)); VGS_HIP_TRY(c, c->rf_mask.ensure((size_t)V));
    hipLaunchKernelGGL(k_rf_tile_labels, dim3((unsigned)((V + TB - 1) / TB)), dim3(TB), 0, c->stream, c->vox_code.p, c->node.p, c->vox_label.p, c->owned.p,
                       c->mixsrc.p, c->rf_halo.p, V, rf_region(c), rf_reach(c), c->rf_eff.p, c->rf_mask.p);
    hipLaunchKernelGGL(k_rf_tile_init, dim3((unsigned)((N + TB - 1) / TB)), dim3(TB), 0, c->stream, c->perm_b.p, c->pt_vox.p, c->rf_eff.p, c->rf_mask.p,
                       c->pt_label.p, N, c->own_first, c->n_own, c->rf_label.p, (unsigned long long*)c->rf_counts.p);
    vgs_status s = rf_pass(c, true, c->used_ids.p, c->adj_key.p, c->adj_cnt.p, U, rp);
    if (s != VGS_OK) return s;
    if (rp.fill && V - U > 0 && U > 0)   // (without a used voxel there is no candidate anywhere)
      if ((s = rf_fill(c, true, rp)) != VGS_OK) return s;
  }
  uint64_t h[6] = {0, 0, 0, 0, 0, 0};
  VGS_READBACK(c, h, c->rf_counts.p, sizeof(h));
  if (h[5]) {
    c->err = "vgs_refine_own_point_labels: " + std::to_string(h[5]) + " candidates of this rank's nodes are used voxels of another rank whose label no record brought (vgs_set_refine_halo_labels)";
    return VGS_E_UNSUPPORTED;
  }
  if (counts5) for (int k = 0; k < 5; ++k) counts5[k] = (int64_t)h[k];
  c->rf_valid = true;
  return VGS_OK;
}

// which side a call serves: vgs_refine_point_labels refuses a tile context, the tile calls refuse a plain one, and the getters serve a
// tile context after vgs_refine_own_point_labels as well
enum RfSide { RF_PLAIN, RF_TILE, RF_EITHER };
static vgs_status rf_check(vgs_ctx* c, const char* fn, RfSide side) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (side == RF_TILE && (!c->have_region || c->n_own < 0)) {
    c->err = std::string(fn) + ": a tile context (vgs_set_owned_region and vgs_set_own_point_range) only";
    return VGS_E_STATE;
  }
  if (side == RF_PLAIN && vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of its segments; the tiled driver refines over all ranks (vgs_tiles_refine_point_labels, vgs_refine_own_point_labels)";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

static vgs_status rf_check_params(vgs_ctx* c, const vgs_refine_params* rp, const char* fn) {
  if (!(rp->patch_radius >= 0.f) || !std::isfinite(rp->patch_radius)) {
    c->err = std::string(fn) + ": patch_radius must be finite and not negative";
    return VGS_E_ARG;
  }
  if (!(rp->switch_ratio >= 0.f && rp->switch_ratio <= 1.f)) { c->err = std::string(fn) + ": switch_ratio must lie in [0, 1]"; return VGS_E_ARG; }
  return VGS_OK;
}

extern "C" vgs_status vgs_set_refine_halo_labels(vgs_ctx* c, const uint64_t* code, const int32_t* label, int64_t n) {
  if (!c || n < 0 || (n > 0 && (!code || !label))) return VGS_E_ARG;
  vgs_status s = rf_check(c, "vgs_set_refine_halo_labels", RF_TILE);
  if (s != VGS_OK) return s;
  for (int64_t k = 0; k < n; ++k)
    if (label[k] < -1) { c->err = "vgs_set_refine_halo_labels: a label below -1"; return VGS_E_ARG; }
  c->rf_halo_valid = false; c->rf_valid = false;
  const int64_t V = c->V;
  if (V == 0) { c->rf_halo_valid = true; return VGS_OK; }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  VGS_HIP_TRY(c, c->rf_halo.ensure((size_t)V));
  VGS_HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)c->rf_halo.p, RF_UNKNOWN, (size_t)V, c->stream));
  if (n > 0) {
    VGS_HIP_TRY(c, c->rf_hcode.ensure((size_t)n)); VGS_HIP_TRY(c, c->rf_hlab.ensure((size_t)n));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->rf_hcode.p, code, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->rf_hlab.p, label, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((s = vgs_halo_find(c, c->rf_hcode.p, c->rf_hlab.p, n, c->rf_halo.p)) != VGS_OK) return s;   // (one record per code: the caller's)
  }
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the upload reads the caller's arrays)
  c->rf_halo_valid = true;
  return VGS_OK;
}

extern "C" vgs_status vgs_get_own_band_labels(vgs_ctx* c, int64_t* n, uint64_t* code, int32_t* label) {
  if (!c || !n) return VGS_E_ARG;
  *n = 0;
  vgs_status s = rf_check(c, "vgs_get_own_band_labels", RF_TILE);
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const int64_t V = c->V;
  if ((!code && !label) || c->rf_band_n < 0) {   // two-call protocol: the size query computes, the call with arrays copies those records
    c->rf_band_n = -1;
    uint32_t total = 0;
    if (V > 0) {
      const int TB = 256;
      const unsigned nbV = (unsigned)((V + TB - 1) / TB);
      VGS_HIP_TRY(c, c->rf_batches.ensure((size_t)V + 1)); VGS_HIP_TRY(c, c->rf_start.ensure((size_t)V + 1));
      hipLaunchKernelGGL(k_rf_band_flags, dim3(nbV), dim3(TB), 0, c->stream, c->vox_code.p, c->owned.p, c->used_rank.p, V, rf_region(c), rf_band_near(c),
                         c->rf_batches.p);
      if ((s = rf_scan_flags(c, (size_t)V, &total)) != VGS_OK) return s;
      if (total > 0) {
        VGS_HIP_TRY(c, c->rf_bcode.ensure((size_t)total)); VGS_HIP_TRY(c, c->rf_blab.ensure((size_t)total));
        hipLaunchKernelGGL(k_rf_band_compact, dim3(nbV), dim3(TB), 0, c->stream, c->rf_batches.p, c->rf_start.p, V, c->vox_code.p, c->vox_label.p,
                           c->rf_bcode.p, c->rf_blab.p);
        VGS_HIP_TRY(c, hipGetLastError());
        VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // the copies below do not wait for the context's stream
      }
    }
    c->rf_band_n = (int64_t)total;
  }
  *n = c->rf_band_n;
  const size_t m = (size_t)c->rf_band_n;
  if (code && m) VGS_HIP_TRY(c, hipMemcpy(code, c->rf_bcode.p, m * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (label && m) VGS_HIP_TRY(c, hipMemcpy(label, c->rf_blab.p, m * sizeof(int32_t), hipMemcpyDeviceToHost));
  return VGS_OK;
}

extern "C" vgs_status vgs_refine_own_point_labels(vgs_ctx* c, const vgs_refine_params* rp, int64_t* counts) {
  if (!c || !rp) return VGS_E_ARG;
  vgs_status s = rf_check(c, "vgs_refine_own_point_labels", RF_TILE);
  if (s != VGS_OK) return s;
  if ((s = rf_check_params(c, rp, "vgs_refine_own_point_labels")) != VGS_OK) return s;
  if (!c->rf_halo_valid) { c->err = "vgs_refine_own_point_labels: no halo labels since the last labels of the tile (vgs_set_refine_halo_labels first)"; return VGS_E_STATE; }
  return vgs_refine_own_on_device(c, *rp, counts);
}

extern "C" vgs_status vgs_refine_params_default(vgs_ctx* c, vgs_refine_params* rp) {
  if (!c || !rp) return VGS_E_ARG;
  rp->patch_radius = c->P.method == 3 ? c->P.seed_size : c->P.voxel_size;
  rp->switch_ratio = 0.25f;
  rp->fill = 1;
  return VGS_OK;
}

extern "C" vgs_status vgs_refine_point_labels(vgs_ctx* c, const vgs_refine_params* rp, int64_t* counts) {
  if (!c || !rp) return VGS_E_ARG;
  vgs_status s = rf_check(c, "vgs_refine_point_labels", RF_PLAIN);
  if (s != VGS_OK) return s;
  if ((s = rf_check_params(c, rp, "vgs_refine_point_labels")) != VGS_OK) return s;
  return vgs_refine_on_device(c, *rp, counts);
}

extern "C" vgs_status vgs_get_refined_labels(vgs_ctx* c, int32_t* labels) {
  if (!c || !labels) return VGS_E_ARG;
  vgs_status s = rf_check(c, "vgs_get_refined_labels", RF_EITHER);
  if (s != VGS_OK) return s;
  if (!c->rf_valid) { c->err = "vgs_get_refined_labels: no refinement since the last run of the stages (vgs_refine_point_labels, or vgs_refine_own_point_labels on a tile context, first)"; return VGS_E_STATE; }
  if (c->N > 0) VGS_HIP_TRY(c, hipMemcpy(labels, c->rf_label.p, (size_t)c->N * 4, hipMemcpyDeviceToHost));
  return VGS_OK;
}

extern "C" vgs_status vgs_get_refined_labels_device(vgs_ctx* c, const int32_t** labels_dev) {
  if (!c || !labels_dev) return VGS_E_ARG;
  vgs_status s = rf_check(c, "vgs_get_refined_labels_device", RF_EITHER);
  if (s != VGS_OK) return s;
  if (!c->rf_valid) { c->err = "vgs_get_refined_labels_device: no refinement since the last run of the stages (vgs_refine_point_labels, or vgs_refine_own_point_labels on a tile context, first)"; return VGS_E_STATE; }
  *labels_dev = c->rf_label.p;
  return VGS_OK;
}
