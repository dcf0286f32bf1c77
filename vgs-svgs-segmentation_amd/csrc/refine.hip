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
#include <string.h>

#include <algorithm>
#include <cmath>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"

#define RF_TB 64                      // one wavefront per work item
#define RF_PPT 4                      // points per lane
#define RF_BATCH (RF_TB * RF_PPT)     // points per work item
#define RF_CH 256                     // candidates staged per chunk (two float4 each: 8 KB of LDS)

// A of the rule: the kept label of a used node, -1 otherwise
__device__ __forceinline__ int32_t rf_node_label(const NodeRec* __restrict__ node, const int32_t* __restrict__ vox_label, uint32_t v) {
  return (node[v].flags & VGS_F_EIG) ? vox_label[v] : -1;
}
// the label w brings as a candidate, -1 when it is none
__device__ __forceinline__ int32_t rf_cand_label(uint32_t flags, const int32_t* __restrict__ vox_label, uint32_t w) {
  const uint32_t need = VGS_F_EIG | VGS_F_POS | VGS_F_NRM;
  if ((flags & need) != need) return -1;
  const int32_t l = vox_label[w];
  return l >= 0 ? l : -1;
}

__global__ void k_rf_init(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pt_vox, const NodeRec* __restrict__ node,
                          const int32_t* __restrict__ vox_label, int64_t N, int32_t* __restrict__ label) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const uint32_t v = pt_vox[j];
  label[perm[j]] = (v == 0xffffffffu) ? -1 : rf_node_label(node, vox_label, v);
}

// the voxels without a stored row, as a flag per voxel and (behind the scan) as a list
__global__ void k_rf_unused_flags(const uint32_t* __restrict__ used_rank, int64_t V, uint32_t* __restrict__ flag) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V) flag[v] = (used_rank[v] == 0xffffffffu) ? 1u : 0u;
}
__global__ void k_rf_unused_list(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, int64_t V, uint32_t cap,
                                 uint32_t* __restrict__ ids) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V && flag[v] && excl[v] < cap) ids[excl[v]] = (uint32_t)v;   // (cap = V - U, the number of flags: the bound only guards the list)
}

// one wavefront per listed node i: node ids[i], row rows + i * stride of cnt[i] entries
__global__ __launch_bounds__(256) void k_rf_mark(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                                 uint32_t n, int stride, const NodeRec* __restrict__ node, const int32_t* __restrict__ vox_label,
                                                 const uint32_t* __restrict__ vox_start, int fill, uint32_t* __restrict__ batches,
                                                 unsigned long long* __restrict__ counts) {
  const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n) return;   // (whole wavefronts; no barrier follows)
  const uint32_t v = ids[i];
  const int32_t A = rf_node_label(node, vox_label, v);
  bool hit = false;
  if (A >= 0 || fill) {
    const uint32_t m = min(cnt[i], (uint32_t)stride);
    const uint64_t* row = rows + (size_t)i * stride;
    for (uint32_t k = lane; k <= m; k += 64) {   // entry m: the node itself
      const uint32_t w = k < m ? (uint32_t)row[k] : v;
      const int32_t L = rf_cand_label(node[w].flags, vox_label, w);
      hit = hit || (L >= 0 && L != A);
    }
  }
  const bool work = __ballot(hit) != 0ull;
  if (lane != 0) return;
  const uint32_t npts = vox_start[v + 1] - vox_start[v];
  batches[i] = work ? (npts + RF_BATCH - 1) / RF_BATCH : 0u;
  if (work) { atomicAdd(&counts[0], 1ull); atomicAdd(&counts[1], (unsigned long long)npts); }
}

__global__ __launch_bounds__(RF_TB) void k_rf_refine(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                                     uint32_t n, int stride, const uint32_t* __restrict__ start, const NodeRec* __restrict__ node,
                                                     const int32_t* __restrict__ vox_label, const uint32_t* __restrict__ vox_start,
                                                     const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                     const uint32_t* __restrict__ perm, float patch_radius, float switch_ratio,
                                                     int32_t* __restrict__ label, unsigned long long* __restrict__ counts) {
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
  const int32_t A = rf_node_label(node, vox_label, v);
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
      const int32_t L = rf_cand_label(r->flags, vox_label, w);
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
  unsigned long long n_changed = 0, n_filled = 0;
#pragma unroll
  for (int k = 0; k < RF_PPT; ++k) {
    const uint32_t j = p0 + k * RF_TB + lane;
    const bool in = j < p1;
    int32_t out = A;
    if (A >= 0) { if (cown[k] < inf && best[k] < switch_ratio * cown[k]) out = blab[k]; }
    else out = blab[k];   // (an unlabelled node is listed with fill only)
    if (in) label[perm[j]] = out;
    n_changed += (unsigned long long)__popcll(__ballot(in && A >= 0 && out != A));
    n_filled += (unsigned long long)__popcll(__ballot(in && A < 0 && out >= 0));
  }
  if (lane == 0) {
    if (n_changed) atomicAdd(&counts[2], n_changed);
    if (n_filled) atomicAdd(&counts[3], n_filled);
  }
}

// mark, scan and refine one list of nodes with their rows
static vgs_status rf_pass(vgs_ctx* c, const uint32_t* ids, const uint64_t* rows, const uint32_t* cnt, int64_t n, const vgs_refine_params& rp) {
  if (n <= 0) return VGS_OK;
  VGS_HIP_TRY(c, c->rf_batches.ensure((size_t)n + 1)); VGS_HIP_TRY(c, c->rf_start.ensure((size_t)n + 1));
  unsigned long long* counts = (unsigned long long*)c->rf_counts.p;
  VGS_HIP_TRY(c, hipMemsetAsync(c->rf_batches.p + n, 0, 4, c->stream));
  hipLaunchKernelGGL(k_rf_mark, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, ids, rows, cnt, (uint32_t)n, c->adj_stride, c->node.p,
                     c->vox_label.p, c->vox_start.p, rp.fill ? 1 : 0, c->rf_batches.p, counts);
  size_t bytes = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, c->rf_batches.p, c->rf_start.p, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, c->sort_tmp.ensure(bytes));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sort_tmp.p, bytes, c->rf_batches.p, c->rf_start.p, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), c->stream));
  uint32_t n_items = 0;
  VGS_READBACK(c, &n_items, c->rf_start.p + n, 4);
  if (n_items > 0)
    hipLaunchKernelGGL(k_rf_refine, dim3(n_items), dim3(RF_TB), 0, c->stream, ids, rows, cnt, (uint32_t)n, c->adj_stride, c->rf_start.p, c->node.p,
                       c->vox_label.p, c->vox_start.p, c->xs.p, c->ys.p, c->zs.p, c->perm_b.p, rp.patch_radius, rp.switch_ratio, c->rf_label.p,
                       counts);
  VGS_HIP_TRY(c, hipGetLastError());
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
    vgs_status s = rf_pass(c, c->used_ids.p, c->adj_key.p, c->adj_cnt.p, U, rp);
    if (s != VGS_OK) return s;
    const int64_t n_un = V - U;
    if (c->P.method == 2 && rp.fill && n_un > 0 && U > 0) {   // (without a used voxel there is no candidate anywhere)
      VGS_HIP_TRY(c, c->rf_batches.ensure((size_t)V + 1)); VGS_HIP_TRY(c, c->rf_start.ensure((size_t)V + 1)); VGS_HIP_TRY(c, c->rf_ids.ensure((size_t)n_un));
      const unsigned nbV = (unsigned)((V + TB - 1) / TB);
      hipLaunchKernelGGL(k_rf_unused_flags, dim3(nbV), dim3(TB), 0, c->stream, c->used_rank.p, V, c->rf_batches.p);
      size_t bytes = 0;
      VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, c->rf_batches.p, c->rf_start.p, 0u, (size_t)V, rocprim::plus<uint32_t>(), c->stream));
      VGS_HIP_TRY(c, c->sort_tmp.ensure(bytes));
      VGS_HIP_TRY(c, rocprim::exclusive_scan(c->sort_tmp.p, bytes, c->rf_batches.p, c->rf_start.p, 0u, (size_t)V, rocprim::plus<uint32_t>(), c->stream));
      hipLaunchKernelGGL(k_rf_unused_list, dim3(nbV), dim3(TB), 0, c->stream, c->rf_batches.p, c->rf_start.p, V, (uint32_t)n_un, c->rf_ids.p);
      VGS_HIP_TRY(c, hipGetLastError());
      // their rows, used neighbours only, a chunk of at most 256 MB of keys at a time
      const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_un, ((int64_t)32 << 20) / std::max(1, c->adj_stride)));
      VGS_HIP_TRY(c, c->rf_rows.ensure((size_t)chunk * c->adj_stride)); VGS_HIP_TRY(c, c->rf_cnt.ensure((size_t)chunk)); VGS_HIP_TRY(c, c->rf_nall.ensure((size_t)chunk));
      for (int64_t o = 0; o < n_un; o += chunk) {
        const int64_t m = std::min(chunk, n_un - o);
        s = vgs_run_adjacency(c, false, c->rf_rows.p, c->rf_cnt.p, c->rf_nall.p, c->adj_r2, c->rf_ids.p + o, m);
        if (s != VGS_OK) return s;
        if ((s = rf_pass(c, c->rf_ids.p + o, c->rf_rows.p, c->rf_cnt.p, m, rp)) != VGS_OK) return s;
      }
    }
  }
  uint64_t h[4] = {0, 0, 0, 0};
  VGS_READBACK(c, h, c->rf_counts.p, sizeof(h));
  if (counts4) for (int k = 0; k < 4; ++k) counts4[k] = (int64_t)h[k];
  c->rf_valid = true;
  return VGS_OK;
}

static vgs_status rf_check(vgs_ctx* c, const char* fn) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of its segments; refinement needs the whole cloud in one context";
    return VGS_E_STATE;
  }
  return VGS_OK;
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
  vgs_status s = rf_check(c, "vgs_refine_point_labels");
  if (s != VGS_OK) return s;
  if (!(rp->patch_radius >= 0.f) || !std::isfinite(rp->patch_radius)) {
    c->err = "vgs_refine_point_labels: patch_radius must be finite and not negative";
    return VGS_E_ARG;
  }
  if (!(rp->switch_ratio >= 0.f && rp->switch_ratio <= 1.f)) { c->err = "vgs_refine_point_labels: switch_ratio must lie in [0, 1]"; return VGS_E_ARG; }
  return vgs_refine_on_device(c, *rp, counts);
}

extern "C" vgs_status vgs_get_refined_labels(vgs_ctx* c, int32_t* labels) {
  if (!c || !labels) return VGS_E_ARG;
  vgs_status s = rf_check(c, "vgs_get_refined_labels");
  if (s != VGS_OK) return s;
  if (!c->rf_valid) { c->err = "vgs_get_refined_labels: no refinement since the last run of the stages (vgs_refine_point_labels first)"; return VGS_E_STATE; }
  if (c->N > 0) VGS_HIP_TRY(c, hipMemcpy(labels, c->rf_label.p, (size_t)c->N * 4, hipMemcpyDeviceToHost));
  return VGS_OK;
}

extern "C" vgs_status vgs_get_refined_labels_device(vgs_ctx* c, const int32_t** labels_dev) {
  if (!c || !labels_dev) return VGS_E_ARG;
  vgs_status s = rf_check(c, "vgs_get_refined_labels_device");
  if (s != VGS_OK) return s;
  if (!c->rf_valid) { c->err = "vgs_get_refined_labels_device: no refinement since the last run of the stages (vgs_refine_point_labels first)"; return VGS_E_STATE; }
  *labels_dev = c->rf_label.p;
  return VGS_OK;
}
