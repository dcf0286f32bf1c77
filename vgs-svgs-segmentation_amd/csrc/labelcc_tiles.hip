// labelcc_tiles.hip -- a tile context's share of the connected parts of a per-point labelling across the ranks of the tiled driver
// (include/vgs.h: vgs_own_point_label_parts, vgs_link_point_label_parts, vgs_apply_point_label_part_ids; include/vgs_tiles.h states the
// definition and the protocol, csrc/tiles.cpp runs it: vgs_tiles_point_label_components).  VGS only, as the tiled path.
//
// Step 1 (own parts).  labelcc.hip's pass over the rank's OWN points (vgs_label_parts_on_device with the own point range: k_ps_keys gives
// every other position the key K, so the vertices are the (label, node) pairs with an own point).  An own vertex's node holds an own point,
// so its cube meets the region and its row ends within graph_size + voxel_size of the border, inside the halo of 2 graph_size + voxel_size:
// the rows this pass reads are complete.  Behind it:
//   k_lt_band_flags / k_lt_band_records  the BAND: the own vertices whose node centre lies within near = graph_size + voxel_size of a
//                     border line of the region (tile_region.hpp; an infinite border never matches), compacted in ascending vertex order
//                     as (code, label, local part, vertex).  Why this band is enough: a vertex w of another rank adjacent to v holds a
//                     point of that rank's region, so w's centre is outside this region or at most half a voxel inside it, and v is within
//                     graph_size of it per axis.
//   k_lt_part_codes   the shared-grid code of every local part's first node
// Step 3 (cross links) over the OTHER ranks' band records (code, label, rank, part):
//   k_lt_find         code -> local node (vgs_find_voxel; a code this rank does not hold drops out), key = label << 32 | node; one stable
//                     radix sort of (key, record index): the hits are the front, a key's records one run in the order they came
//   k_lt_unused_flags / k_lt_unused_list  the band vertices whose node has no stored row; their rows are built in full a chunk at a time
//                     by vgs_run_adjacency in refine.hip's row scratch, as labelcc.hip does
//   k_lt_link_short / k_lt_link_long  for every own band vertex (l, v) the row of v -- stored, or built -- and for every neighbour w != v
//                     the run of records with key (l, w): one triple (own local part, rank, part) for EVERY record of the run (two or
//                     three ranks publish the same key at a corner).  Rows of at most LT_SHORT entries go eight to a wavefront, longer
//                     ones get a whole wavefront; both kernels run over the same list and each leaves the other's rows alone.  The triples
//                     go through one counter into a list; a list too short is grown to the count and the kernels run again.
//   merge sort and unique of the triples: the payload has the same bytes from call to call whatever the order of the atomics.
// Each rank walks only the rows of its own vertices.  r finds w in row(v), s finds v in row(w): the union over the ranks is the "either
// row" rule of vgs_point_label_components, and a stored row pruned to used neighbours is covered by the other side's full row.
// Step 6.  k_lt_apply: the global part of every own point through the map the driver's fold gives, in the order of the rank's load.
// Everything is integer; nothing here depends on the order of a reduction.
#include <string.h>

#include <algorithm>
#include <string>

#include <rocprim/rocprim.hpp>

#include "vgs_context.hpp"
#include "tile_region.hpp"

#define LT_TB 256
#define LT_SHORT 64   // rows of at most so many entries share a wavefront
#define LT_NONE 0xffffffffu

struct LtLink { uint32_t own, rank, part, pad; };
struct LtLess {
  __host__ __device__ bool operator()(const LtLink& a, const LtLink& b) const {
    if (a.own != b.own) return a.own < b.own;
    if (a.rank != b.rank) return a.rank < b.rank;
    return a.part < b.part;
  }
};
struct LtEqual {
  __host__ __device__ bool operator()(const LtLink& a, const LtLink& b) const { return a.own == b.own && a.rank == b.rank && a.part == b.part; }
};

// flag[nv] = 0 closes the scan
__global__ __launch_bounds__(LT_TB) void k_lt_band_flags(const uint32_t* __restrict__ vnode, const uint64_t* __restrict__ vox_code, uint32_t nv, RfRegion g,
                                                         double near, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * LT_TB + threadIdx.x;
  if (i > (uint64_t)nv) return;
  bool nr = false;
  if (i < (uint64_t)nv) {
    double cx, cy;
    rf_center(g, vox_code[vnode[i]], cx, cy);
    nr = fabs(cx - g.lo_x) < near || fabs(cx - g.hi_x) < near || fabs(cy - g.lo_y) < near || fabs(cy - g.hi_y) < near;
  }
  flag[i] = nr ? 1u : 0u;
}
__global__ __launch_bounds__(LT_TB) void k_lt_band_records(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ vnode,
                                                           const uint32_t* __restrict__ vlabel, const uint32_t* __restrict__ vpart,
                                                           const uint64_t* __restrict__ vox_code, uint32_t nv, uint32_t cap, uint64_t* __restrict__ code,
                                                           int32_t* __restrict__ label, int32_t* __restrict__ part, uint32_t* __restrict__ vtx) {
  const uint64_t i = (uint64_t)blockIdx.x * LT_TB + threadIdx.x;
  if (i >= (uint64_t)nv || !flag[i]) return;
  const uint32_t o = excl[i];
  if (o >= cap) return;   // (cap is the scan's own total: the bound only guards the arrays)
  code[o] = vox_code[vnode[i]]; label[o] = (int32_t)vlabel[i];
  if (vpart) { part[o] = (int32_t)vpart[i]; vtx[o] = (uint32_t)i; }   // (nullptr: the label graph's band, code and label only)
}
__global__ __launch_bounds__(LT_TB) void k_lt_part_codes(const int32_t* __restrict__ p_first, const uint64_t* __restrict__ vox_code, uint32_t C, int64_t V,
                                                         uint64_t* __restrict__ p_code) {
  const uint64_t p = (uint64_t)blockIdx.x * LT_TB + threadIdx.x;
  if (p >= (uint64_t)C) return;
  const int64_t v = (int64_t)p_first[p];
  p_code[p] = (v >= 0 && v < V) ? vox_code[v] : 0ull;
}

// the other ranks' records: key = label << 32 | local node, all ones for a code this rank does not hold; counts[0] += hits
__global__ __launch_bounds__(LT_TB) void k_lt_find(const uint64_t* __restrict__ code, const int32_t* __restrict__ label, int64_t n,
                                                   const uint64_t* __restrict__ vox_code, int64_t V, uint64_t* __restrict__ key, uint32_t* __restrict__ val,
                                                   unsigned long long* __restrict__ counts) {
  const int64_t k = (int64_t)blockIdx.x * LT_TB + threadIdx.x;
  bool hit = false;
  if (k < n) {
    const int64_t v = vgs_find_voxel(vox_code, V, code[k]);
    hit = v < V && label[k] >= 0;
    key[k] = hit ? ((uint64_t)(uint32_t)label[k] << 32) | (uint64_t)(uint32_t)v : ~0ull;
    val[k] = (uint32_t)k;
  }
  const unsigned long long nb = (unsigned long long)__popcll(__ballot(hit));
  if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&counts[0], nb);
}

// the band records whose node has no stored row, as a flag (flag[nb] = 0 closes the scan) and behind the scan as a list (band index, node id)
__global__ __launch_bounds__(LT_TB) void k_lt_unused_flags(const uint32_t* __restrict__ bvtx, const uint32_t* __restrict__ vnode,
                                                           const uint32_t* __restrict__ used_rank, uint32_t nb, uint32_t* __restrict__ flag) {
  const uint64_t j = (uint64_t)blockIdx.x * LT_TB + threadIdx.x;
  if (j > (uint64_t)nb) return;
  flag[j] = (j < (uint64_t)nb && used_rank[vnode[bvtx[j]]] == LT_NONE) ? 1u : 0u;
}
__global__ __launch_bounds__(LT_TB) void k_lt_unused_list(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ bvtx,
                                                          const uint32_t* __restrict__ vnode, uint32_t nb, uint32_t cap, uint32_t* __restrict__ u_band,
                                                          uint32_t* __restrict__ u_node) {
  const uint64_t j = (uint64_t)blockIdx.x * LT_TB + threadIdx.x;
  if (j >= (uint64_t)nb || !flag[j]) return;
  const uint32_t o = excl[j];
  if (o < cap) { u_band[o] = (uint32_t)j; u_node[o] = vnode[bvtx[j]]; }   // (cap = the number of flags: the bound only guards the list)
}

// W lanes per row, 64 / W rows per wavefront.  Item j: band record items[j] (items == nullptr: band record j).  used_rank != nullptr: the
// stored rows, row used_rank[node], a record of an unused node leaves; nullptr: the rows built for this list, row j.  W = 64 takes the
// rows above LT_SHORT entries, any other W those up to it.  counts[1] counts every triple; one past `cap` is counted and not written.
template <int W>
__device__ __forceinline__ void lt_link_body(const uint32_t* __restrict__ items, uint32_t n_items, const uint32_t* __restrict__ bvtx,
                                             const int32_t* __restrict__ blabel, const int32_t* __restrict__ bpart, const uint32_t* __restrict__ vnode,
                                             const uint32_t* __restrict__ used_rank, const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                             int stride, const uint64_t* __restrict__ fkey, const uint32_t* __restrict__ fval, uint32_t nh,
                                             const int32_t* __restrict__ frank, const int32_t* __restrict__ fpart, unsigned long long cap,
                                             LtLink* __restrict__ out, unsigned long long* __restrict__ counts) {
  const uint32_t j = blockIdx.x * (64 / W) + threadIdx.x / W;
  const uint32_t sub = threadIdx.x % W;
  if (j >= n_items) return;   // (whole row groups; no barrier follows)
  const uint32_t b = items ? items[j] : j;
  const uint32_t v = vnode[bvtx[b]];
  uint32_t r = j;
  if (used_rank) { r = used_rank[v]; if (r == LT_NONE) return; }
  const uint32_t m = min(cnt[r], (uint32_t)stride);
  if ((W == 64) != (m > LT_SHORT)) return;
  const uint64_t hi = (uint64_t)(uint32_t)blabel[b] << 32;
  const uint32_t own = (uint32_t)bpart[b];
  const uint64_t* row = rows + (size_t)r * stride;
  uint32_t last_rank = LT_NONE, last_part = LT_NONE;   // a lane's run of equal triples is written once; the unique pass takes the rest
  for (uint32_t k = sub; k < m; k += W) {
    const uint32_t w = (uint32_t)row[k];
    if (w == v) continue;   // (a stored row starts with its own node; the shared voxel itself is the fold's equal-key rule)
    const uint64_t key = hi | (uint64_t)w;
    uint32_t lo = 0, up = nh;
    while (lo < up) { const uint32_t mid = (lo + up) >> 1; if (fkey[mid] < key) lo = mid + 1; else up = mid; }
    for (; lo < nh && fkey[lo] == key; ++lo) {
      const uint32_t rec = fval[lo];
      const uint32_t rk = (uint32_t)frank[rec], pt = (uint32_t)fpart[rec];
      if (rk == last_rank && pt == last_part) continue;
      last_rank = rk; last_part = pt;
      const unsigned long long o = atomicAdd(&counts[1], 1ull);
      if (o < cap) out[o] = LtLink{own, rk, pt, 0u};
    }
  }
}

__global__ __launch_bounds__(64) void k_lt_link_short(const uint32_t* __restrict__ items, uint32_t n_items, const uint32_t* __restrict__ bvtx,
                                                      const int32_t* __restrict__ blabel, const int32_t* __restrict__ bpart,
                                                      const uint32_t* __restrict__ vnode, const uint32_t* __restrict__ used_rank,
                                                      const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt, int stride,
                                                      const uint64_t* __restrict__ fkey, const uint32_t* __restrict__ fval, uint32_t nh,
                                                      const int32_t* __restrict__ frank, const int32_t* __restrict__ fpart, unsigned long long cap,
                                                      LtLink* __restrict__ out, unsigned long long* __restrict__ counts) {
  lt_link_body<8>(items, n_items, bvtx, blabel, bpart, vnode, used_rank, rows, cnt, stride, fkey, fval, nh, frank, fpart, cap, out, counts);
}
__global__ __launch_bounds__(64) void k_lt_link_long(const uint32_t* __restrict__ items, uint32_t n_items, const uint32_t* __restrict__ bvtx,
                                                     const int32_t* __restrict__ blabel, const int32_t* __restrict__ bpart,
                                                     const uint32_t* __restrict__ vnode, const uint32_t* __restrict__ used_rank,
                                                     const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt, int stride,
                                                     const uint64_t* __restrict__ fkey, const uint32_t* __restrict__ fval, uint32_t nh,
                                                     const int32_t* __restrict__ frank, const int32_t* __restrict__ fpart, unsigned long long cap,
                                                     LtLink* __restrict__ out, unsigned long long* __restrict__ counts) {
  lt_link_body<64>(items, n_items, bvtx, blabel, bpart, vnode, used_rank, rows, cnt, stride, fkey, fval, nh, frank, fpart, cap, out, counts);
}

// own point i = cloud point own_first + i: its local part through the map, -1 without one
__global__ __launch_bounds__(LT_TB) void k_lt_apply(const int32_t* __restrict__ pop, const int32_t* __restrict__ map, int64_t own_first, int64_t n_own,
                                                    int64_t C, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * LT_TB + threadIdx.x;
  if (i >= n_own) return;
  const int64_t p = (int64_t)pop[own_first + i];
  out[i] = (p >= 0 && p < C) ? map[p] : -1;
}

// ---------------------------------------------------------------------------------------------------------------------- host
static unsigned lt_grid(uint64_t n) { return (unsigned)((n + LT_TB - 1) / LT_TB); }

// exclusive scan of n words on the context's stream, rocprim's storage in ps_tmp
static vgs_status lt_scan(vgs_ctx* c, uint32_t* in, uint32_t* out, size_t n) {
  size_t bytes = 0;
  VGS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
  VGS_HIP_TRY(c, c->ps_tmp.ensure(bytes));
  VGS_HIP_TRY(c, rocprim::exclusive_scan(c->ps_tmp.p, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
  return VGS_OK;
}

// the band's reach: a neighbour is within graph_size per axis, its centre at most half a voxel inside this region, and half a voxel more
// so that no rounding of a centre decides
static double lt_near(const vgs_ctx* c) { return (double)c->P.graph_size + (double)c->P.voxel_size; }

static vgs_status lt_check(vgs_ctx* c, const char* fn) {
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (!c->have_region || c->n_own < 0) {
    c->err = std::string(fn) + ": a tile context (vgs_set_owned_region and vgs_set_own_point_range) only";
    return VGS_E_STATE;
  }
  if (c->P.method != 2) { c->err = std::string(fn) + ": the tiled path is VGS only"; return VGS_E_UNSUPPORTED; }
  return VGS_OK;
}

// the band records of nv vertices, compacted in ascending vertex order (vpart == nullptr: code and label only, lct_bpart and lct_bvtx are
// left alone); the stream is waited for
vgs_status vgs_lt_band_on_device(vgs_ctx* c, const uint32_t* vnode, const uint32_t* vlabel, const uint32_t* vpart, uint32_t nv, uint32_t* n_band) {
  *n_band = 0;
  if (nv == 0) return VGS_OK;
  const size_t w = (size_t)nv + 1;
  uint32_t nb = 0;
  vgs_status s;
  VGS_HIP_TRY(c, c->lct_flag.ensure(w)); VGS_HIP_TRY(c, c->lct_scan.ensure(w));
  hipLaunchKernelGGL(k_lt_band_flags, dim3(lt_grid(w)), dim3(LT_TB), 0, c->stream, vnode, c->vox_code.p, nv, rf_region(c), lt_near(c), c->lct_flag.p);
  if ((s = lt_scan(c, c->lct_flag.p, c->lct_scan.p, w)) != VGS_OK) return s;
  VGS_READBACK(c, &nb, c->lct_scan.p + nv, 4);
  if (nb > 0) {
    VGS_HIP_TRY(c, c->lct_bcode.ensure(nb)); VGS_HIP_TRY(c, c->lct_blabel.ensure(nb));
    if (vpart) { VGS_HIP_TRY(c, c->lct_bpart.ensure(nb)); VGS_HIP_TRY(c, c->lct_bvtx.ensure(nb)); }
    hipLaunchKernelGGL(k_lt_band_records, dim3(lt_grid(nv)), dim3(LT_TB), 0, c->stream, c->lct_flag.p, c->lct_scan.p, vnode, vlabel, vpart, c->vox_code.p, nv, nb,
                       c->lct_bcode.p, c->lct_blabel.p, vpart ? c->lct_bpart.p : nullptr, vpart ? c->lct_bvtx.p : nullptr);
  }
  VGS_HIP_TRY(c, hipGetLastError());
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n_band = nb;
  return VGS_OK;
}

// the lookup of n records in the local grid (k_lt_find), left on the stream
vgs_status vgs_lt_find_on_device(vgs_ctx* c, const uint64_t* code_dev, const int32_t* label_dev, int64_t n, uint64_t* key, uint32_t* val,
                                 unsigned long long* counts) {
  if (n <= 0) return VGS_OK;
  hipLaunchKernelGGL(k_lt_find, dim3(lt_grid((uint64_t)n)), dim3(LT_TB), 0, c->stream, code_dev, label_dev, n, c->vox_code.p, c->V, key, val, counts);
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}

static vgs_status lt_own(vgs_ctx* c, const char* fn, const int32_t* labels, bool on_device, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_band,
                         int64_t* n_skipped) {
  if (!c) return VGS_E_ARG;
  if (n_parts) *n_parts = 0;
  if (n_band) *n_band = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status s = lt_check(c, fn);
  if (s != VGS_OK) return s;
  c->lcc_valid = false; c->lct_own = c->lct_linked = c->lct_applied = false; c->lgt_own = c->lgt_valid = false;
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
  int64_t C = 0;
  if ((s = vgs_label_parts_on_device(c, fn, labels, c->own_first, n, K, &C, n_skipped)) != VGS_OK) return s;
  const uint32_t nv = c->lcc_nv;
  uint32_t nb = 0;
  if (nv > 0 && C > 0) {
    const size_t w = (size_t)nv + 1;
    const uint32_t *vnode = c->lcc_vtx.p, *vlabel = vnode + w, *vpart = vnode + 5 * w;
    VGS_HIP_TRY(c, c->lct_pcode.ensure((size_t)C));
    hipLaunchKernelGGL(k_lt_part_codes, dim3(lt_grid((uint64_t)C)), dim3(LT_TB), 0, c->stream, c->lcc_pfirst.p, c->vox_code.p, (uint32_t)C, c->V, c->lct_pcode.p);
    if ((s = vgs_lt_band_on_device(c, vnode, vlabel, vpart, nv, &nb)) != VGS_OK) return s;
  }
  c->lct_band = (int64_t)nb; c->lct_links = 0; c->lct_K = K; c->lct_own = true;
  if (n_parts) *n_parts = C;
  if (n_band) *n_band = (int64_t)nb;
  return VGS_OK;
}

extern "C" vgs_status vgs_own_point_label_parts(vgs_ctx* c, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_band,
                                                int64_t* n_skipped) {
  return lt_own(c, "vgs_own_point_label_parts", labels_host, false, n, K, n_parts, n_band, n_skipped);
}
extern "C" vgs_status vgs_own_point_label_parts_device(vgs_ctx* c, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_band,
                                                       int64_t* n_skipped) {
  return lt_own(c, "vgs_own_point_label_parts_device", labels_dev, true, n, K, n_parts, n_band, n_skipped);
}

static vgs_status lt_have_own(vgs_ctx* c, const char* fn) {
  if (!c) return VGS_E_ARG;
  vgs_status s = lt_check(c, fn);
  if (s != VGS_OK) return s;
  if (!c->lcc_valid || !c->lct_own) {
    c->err = std::string(fn) + ": no own parts since the last run of the stages (vgs_own_point_label_parts first)";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

#define LT_COPY(dst, src, count) \
  if ((dst) && (count) > 0) VGS_HIP_TRY(c, hipMemcpy((dst), (src), (size_t)(count) * sizeof(*(dst)), hipMemcpyDeviceToHost))

extern "C" vgs_status vgs_get_own_point_label_parts(vgs_ctx* c, int32_t* part_label, int64_t* part_points, int32_t* part_nodes, uint64_t* part_first_code,
                                                    uint64_t* band_code, int32_t* band_label, int32_t* band_part) {
  vgs_status s = lt_have_own(c, "vgs_get_own_point_label_parts");
  if (s != VGS_OK) return s;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  LT_COPY(part_label, c->lcc_plabel.p, c->lcc_C); LT_COPY(part_points, c->lcc_ppoints.p, c->lcc_C); LT_COPY(part_nodes, c->lcc_pnodes.p, c->lcc_C);
  LT_COPY(part_first_code, c->lct_pcode.p, c->lcc_C);
  LT_COPY(band_code, c->lct_bcode.p, c->lct_band); LT_COPY(band_label, c->lct_blabel.p, c->lct_band); LT_COPY(band_part, c->lct_bpart.p, c->lct_band);
  return VGS_OK;
}

// both link kernels over one list of n items (items == nullptr: all band records against the stored rows)
static vgs_status lt_link(vgs_ctx* c, const uint32_t* items, uint32_t n, const uint32_t* used_rank, const uint64_t* rows, const uint32_t* cnt, uint32_t nh,
                          unsigned long long cap) {
  if (n == 0) return VGS_OK;
  unsigned long long* counts = (unsigned long long*)c->lct_count.p;
  hipLaunchKernelGGL(k_lt_link_short, dim3((n + 7) / 8), dim3(64), 0, c->stream, items, n, c->lct_bvtx.p, c->lct_blabel.p, c->lct_bpart.p, c->lcc_vtx.p, used_rank,
                     rows, cnt, c->adj_stride, c->lct_key2.p, c->lct_val2.p, nh, c->lct_frank.p, c->lct_fpart.p, cap, (LtLink*)c->lct_link.p, counts);
  hipLaunchKernelGGL(k_lt_link_long, dim3(n), dim3(64), 0, c->stream, items, n, c->lct_bvtx.p, c->lct_blabel.p, c->lct_bpart.p, c->lcc_vtx.p, used_rank, rows, cnt,
                     c->adj_stride, c->lct_key2.p, c->lct_val2.p, nh, c->lct_frank.p, c->lct_fpart.p, cap, (LtLink*)c->lct_link.p, counts);
  VGS_HIP_TRY(c, hipGetLastError());
  return VGS_OK;
}

extern "C" vgs_status vgs_link_point_label_parts(vgs_ctx* c, const uint64_t* code, const int32_t* label, const int32_t* rank, const int32_t* part, int64_t n,
                                                 int64_t* n_links) {
  if (n_links) *n_links = 0;
  vgs_status s = lt_have_own(c, "vgs_link_point_label_parts");
  if (s != VGS_OK) return s;
  c->lct_linked = false; c->lct_links = 0;
  if (n < 0 || n > (int64_t)0x7fffffff || (n > 0 && (!code || !label || !rank || !part))) {
    c->err = "vgs_link_point_label_parts: n records need four arrays, n at most 2^31 - 1";
    return VGS_E_ARG;
  }
  const uint32_t nb = (uint32_t)c->lct_band;
  const int64_t V = c->V;
  unsigned long long total = 0;
  if (n > 0 && nb > 0 && V > 0) {
    VGS_HIP_TRY(c, hipSetDevice(c->device));
    const size_t m = (size_t)n;
    VGS_HIP_TRY(c, c->lct_fcode.ensure(m)); VGS_HIP_TRY(c, c->lct_flabel.ensure(m)); VGS_HIP_TRY(c, c->lct_frank.ensure(m)); VGS_HIP_TRY(c, c->lct_fpart.ensure(m));
    VGS_HIP_TRY(c, c->lct_key.ensure(m)); VGS_HIP_TRY(c, c->lct_key2.ensure(m)); VGS_HIP_TRY(c, c->lct_val.ensure(m)); VGS_HIP_TRY(c, c->lct_val2.ensure(m));
    VGS_HIP_TRY(c, c->lct_count.ensure(4));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->lct_fcode.p, code, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->lct_flabel.p, label, m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->lct_frank.p, rank, m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    VGS_HIP_TRY(c, hipMemcpyAsync(c->lct_fpart.p, part, m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    unsigned long long* counts = (unsigned long long*)c->lct_count.p;
    VGS_HIP_TRY(c, hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), c->stream));
    if ((s = vgs_lt_find_on_device(c, c->lct_fcode.p, c->lct_flabel.p, n, c->lct_key.p, c->lct_val.p, counts)) != VGS_OK) return s;
    size_t t_sort = 0;
    VGS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, t_sort, c->lct_key.p, c->lct_key2.p, c->lct_val.p, c->lct_val2.p, m, 0, 64, c->stream));
    VGS_HIP_TRY(c, c->ps_tmp.ensure(t_sort));
    VGS_HIP_TRY(c, rocprim::radix_sort_pairs(c->ps_tmp.p, t_sort, c->lct_key.p, c->lct_key2.p, c->lct_val.p, c->lct_val2.p, m, 0, 64, c->stream));
    unsigned long long h = 0;
    VGS_READBACK(c, &h, counts, sizeof(h));   // (also: the upload has read the caller's arrays)
    const uint32_t nh = (uint32_t)std::min<unsigned long long>(h, (unsigned long long)m);
    if (nh > 0) {
      // the band records of unused voxels: their rows are built in full a chunk at a time
      const bool some_unused = V - c->U > 0;
      uint32_t n_un = 0;
      if (some_unused) {
        VGS_HIP_TRY(c, c->lct_flag.ensure((size_t)nb + 1)); VGS_HIP_TRY(c, c->lct_scan.ensure((size_t)nb + 1));
        hipLaunchKernelGGL(k_lt_unused_flags, dim3(lt_grid((uint64_t)nb + 1)), dim3(LT_TB), 0, c->stream, c->lct_bvtx.p, c->lcc_vtx.p, c->used_rank.p, nb, c->lct_flag.p);
        if ((s = lt_scan(c, c->lct_flag.p, c->lct_scan.p, (size_t)nb + 1)) != VGS_OK) return s;
        VGS_READBACK(c, &n_un, c->lct_scan.p + nb, 4);
        if (n_un > 0) {
          VGS_HIP_TRY(c, c->lct_list.ensure(2 * (size_t)n_un));
          hipLaunchKernelGGL(k_lt_unused_list, dim3(lt_grid(nb)), dim3(LT_TB), 0, c->stream, c->lct_flag.p, c->lct_scan.p, c->lct_bvtx.p, c->lcc_vtx.p, nb, n_un,
                             c->lct_list.p, c->lct_list.p + n_un);
          VGS_HIP_TRY(c, hipGetLastError());
        }
      }
      const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::max<uint32_t>(n_un, 1u), ((int64_t)32 << 20) / std::max(1, c->adj_stride)));   // at most 256 MB of keys
      if (n_un > 0) { VGS_HIP_TRY(c, c->rf_rows.ensure((size_t)chunk * c->adj_stride)); VGS_HIP_TRY(c, c->rf_cnt.ensure((size_t)chunk)); VGS_HIP_TRY(c, c->rf_nall.ensure((size_t)chunk)); }
      unsigned long long cap = std::max<unsigned long long>(4ull * nh, 1024ull);
      for (int pass = 0; pass < 2; ++pass) {   // a list too short: the count is exact, the second pass fits
        VGS_HIP_TRY(c, c->lct_link.ensure(4 * (size_t)cap));
        VGS_HIP_TRY(c, hipMemsetAsync(counts + 1, 0, sizeof(unsigned long long), c->stream));
        if (c->U > 0 && (s = lt_link(c, nullptr, nb, c->used_rank.p, c->adj_key.p, c->adj_cnt.p, nh, cap)) != VGS_OK) return s;
        const uint32_t *u_band = c->lct_list.p, *u_node = c->lct_list.p + n_un;
        for (int64_t o = 0; o < (int64_t)n_un; o += chunk) {
          const int64_t mm = std::min(chunk, (int64_t)n_un - o);
          if ((s = vgs_run_adjacency(c, true, c->rf_rows.p, c->rf_cnt.p, c->rf_nall.p, c->adj_r2, u_node + o, mm)) != VGS_OK) return s;
          if ((s = lt_link(c, u_band + o, (uint32_t)mm, nullptr, c->rf_rows.p, c->rf_cnt.p, nh, cap)) != VGS_OK) return s;
        }
        VGS_READBACK(c, &total, counts + 1, sizeof(total));
        if (total <= cap) break;
        if (pass == 1 || total > (unsigned long long)0x7fffffff) {
          c->err = "vgs_link_point_label_parts: " + std::to_string(total) + " link triples, above the limit of one list";
          return VGS_E_UNSUPPORTED;
        }
        cap = total;
      }
      if (total > 0) {
        const size_t nt = (size_t)total;
        VGS_HIP_TRY(c, c->lct_link2.ensure(4 * nt));
        LtLink *a = (LtLink*)c->lct_link.p, *b = (LtLink*)c->lct_link2.p;
        size_t t_ms = 0, t_un = 0;
        VGS_HIP_TRY(c, rocprim::merge_sort(nullptr, t_ms, a, b, nt, LtLess(), c->stream));
        VGS_HIP_TRY(c, rocprim::unique(nullptr, t_un, b, a, counts + 1, nt, LtEqual(), c->stream));
        VGS_HIP_TRY(c, c->ps_tmp.ensure(std::max(t_ms, t_un)));
        VGS_HIP_TRY(c, rocprim::merge_sort(c->ps_tmp.p, t_ms, a, b, nt, LtLess(), c->stream));
        VGS_HIP_TRY(c, rocprim::unique(c->ps_tmp.p, t_un, b, a, counts + 1, nt, LtEqual(), c->stream));
        VGS_READBACK(c, &total, counts + 1, sizeof(total));
        total = std::min<unsigned long long>(total, nt);
      }
    }
  }
  c->lct_links = (int64_t)total; c->lct_linked = true;
  if (n_links) *n_links = (int64_t)total;
  return VGS_OK;
}

extern "C" vgs_status vgs_get_point_label_part_links(vgs_ctx* c, int32_t* own_part, int32_t* rank, int32_t* part) {
  vgs_status s = lt_have_own(c, "vgs_get_point_label_part_links");
  if (s != VGS_OK) return s;
  if (!c->lct_linked) { c->err = "vgs_get_point_label_part_links: no links since the last own parts (vgs_link_point_label_parts first)"; return VGS_E_STATE; }
  const size_t n = (size_t)c->lct_links;
  if (n == 0) return VGS_OK;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  std::vector<LtLink> h(n);
  VGS_HIP_TRY(c, hipMemcpy(h.data(), c->lct_link.p, n * sizeof(LtLink), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    if (own_part) own_part[i] = (int32_t)h[i].own;
    if (rank) rank[i] = (int32_t)h[i].rank;
    if (part) part[i] = (int32_t)h[i].part;
  }
  return VGS_OK;
}

extern "C" vgs_status vgs_apply_point_label_part_ids(vgs_ctx* c, const int32_t* map, int64_t n) {
  vgs_status s = lt_have_own(c, "vgs_apply_point_label_part_ids");
  if (s != VGS_OK) return s;
  c->lct_applied = false;
  if (n != c->lcc_C || (n > 0 && !map)) {
    c->err = "vgs_apply_point_label_part_ids: n = " + std::to_string(n) + " must equal the number of own parts, " + std::to_string(c->lcc_C);
    return VGS_E_ARG;
  }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const int64_t n_own = c->n_own;
  VGS_HIP_TRY(c, c->lct_ids.ensure(n_own > 0 ? (size_t)n_own : 1)); VGS_HIP_TRY(c, c->lct_map.ensure(n > 0 ? (size_t)n : 1));
  if (n > 0) VGS_HIP_TRY(c, hipMemcpyAsync(c->lct_map.p, map, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (n_own > 0) {
    hipLaunchKernelGGL(k_lt_apply, dim3(lt_grid((uint64_t)n_own)), dim3(LT_TB), 0, c->stream, c->lcc_pop.p, c->lct_map.p, c->own_first, n_own, n, c->lct_ids.p);
    VGS_HIP_TRY(c, hipGetLastError());
  }
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the upload reads the caller's array)
  c->lct_applied = true;
  return VGS_OK;
}

static vgs_status lt_have_ids(vgs_ctx* c, const char* fn) {
  vgs_status s = lt_have_own(c, fn);
  if (s != VGS_OK) return s;
  if (!c->lct_applied) { c->err = std::string(fn) + ": no part ids since the last own parts (vgs_apply_point_label_part_ids first)"; return VGS_E_STATE; }
  return VGS_OK;
}

extern "C" vgs_status vgs_get_point_label_part_ids(vgs_ctx* c, int32_t* part_of_point, int64_t n) {
  vgs_status s = lt_have_ids(c, "vgs_get_point_label_part_ids");
  if (s != VGS_OK) return s;
  if (n != c->n_own || (n > 0 && !part_of_point)) { c->err = "vgs_get_point_label_part_ids: n must equal the number of own points of the context"; return VGS_E_ARG; }
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  LT_COPY(part_of_point, c->lct_ids.p, n);
  return VGS_OK;
}

extern "C" vgs_status vgs_get_point_label_part_ids_device(vgs_ctx* c, const int32_t** part_of_point) {
  vgs_status s = lt_have_ids(c, "vgs_get_point_label_part_ids_device");
  if (s != VGS_OK) return s;
  if (part_of_point) *part_of_point = c->n_own > 0 ? c->lct_ids.p : nullptr;
  return VGS_OK;
}
