// segbox.hip -- oriented bounding boxes of the kept segments (no reference counterpart: the size of a segment along its own axes, what
// pcl::MomentOfInertiaEstimation::getOBB gives for one cluster).  Row k covers exactly the points whose label is k.  Two frames:
//   VGS_BOX_PRINCIPAL  the segment's PCA axes, the evecs9 row of the descriptor table byte for byte
//   VGS_BOX_UPRIGHT    axis 2 = (0, 0, 1); axes 0 and 1 the eigenvectors of the xy block of the descriptor's cov6 (one Jacobi rotation in fp64,
//                      sd_jacobi_rotate's formulae), ascending eigenvalue, evecs9's sign rule
// The extents are min / max of projections onto axes that the descriptor pass produces, so they are a second pass over the points.
// Data flow: the descriptor table first (vgs_segdesc_on_device: centroid3, evecs9, cov6), k_sb_frames writes the frame of every segment
// into the box table's own buffer, sd_prepare gives the decomposition of segdesc.hip (nodes sorted by label, virtual positions, chunks of
// SD_CHUNK virtual points that never cross a segment and may split a node), then
//   k_sb_chunks  one workgroup per chunk: t_j = (W[0][j] dx + W[1][j] dy) + W[2][j] dz for d = p - c in fp64, per-lane min / max, wavefront
//                butterfly, the waves through LDS, one partial of SB_REC doubles
//   k_sb_final   one wavefront per segment folds its partials and writes lo3, hi3, half3 = (hi - lo) / 2 and
//                center3[r] = c[r] + ((W[r][0] mid[0] + W[r][1] mid[1]) + W[r][2] mid[2]), mid = (lo + hi) / 2
// Exact arithmetic: every product and sum above is one IEEE fp64 operation in the stated association (the build passes
// -ffp-contract=off: no FMA), and min / max do not depend on the order, so the table is a function of the points, c and W alone -- a
// float64 restatement reproduces it to the bit (tests/segment_boxes_ref.py).  A zero bound may carry either sign, as in bbox6.
// No atomics.  The chunk kernel takes c and W as arrays per label, so a rank of the tiled driver runs it over its own points about a
// centroid and frame handed in (k_sb_chunks_own, below).  Scratch: sb_part and the sd_* scratch of sd_prepare, nothing a getter reads.  Cached per frame until the
// next run (sb_valid[frame]); vgs_segment_descriptors_from_moments may overwrite the descriptor buffers afterwards, the box table keeps
// the frame its extents were taken in.
// Tile contexts (the tiled driver, include/vgs_tiles.h): the global descriptor rows come in from the host, k_sb_frames makes the frames,
// k_sb_chunks_own takes the extents of the rank's own points over the global labels and k_sb_final folds them per segment
// (vgs_get_own_segment_extents); the driver folds all ranks' records on the host (min / max) and k_sb_final, over one partial per segment,
// finishes the table (vgs_segment_boxes_from_extents).  Their buffers are sbt_* and sb_part: a cached table is not touched.
#include <string.h>
#include <vector>

#include "segpass.hpp"   // SB_REC doubles per partial record, and the bodies shared with pointseg.hip

// The frame of segment k.  Principal: the evecs9 row.  Upright: see the header.  One thread per segment.
__global__ __launch_bounds__(256) void k_sb_frames(const double* __restrict__ evec, const double* __restrict__ cov, uint32_t K, int upright,
                                                   double* __restrict__ frame) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  double* o = frame + (size_t)k * 9;
  if (!upright) {
#pragma unroll
    for (int f = 0; f < 9; ++f) o[f] = evec[(size_t)k * 9 + f];
    return;
  }
  // one Jacobi rotation that zeroes A[0][1] of the xy block (sd_jacobi_rotate<0, 1> without the third index): A' = J^T A J, W' = W J
  double a00 = cov[(size_t)k * 6 + 0], a11 = cov[(size_t)k * 6 + 3];
  const double apq = cov[(size_t)k * 6 + 1];
  double W[2][2] = {{1, 0}, {0, 1}};
  if (apq != 0.0) {
    const double theta = (a11 - a00) / (2.0 * apq);
    const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
    a00 -= t * apq;
    a11 += t * apq;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double wp = W[i][0], wq = W[i][1];
      W[i][0] = cs * wp - sn * wq;
      W[i][1] = sn * wp + cs * wq;
    }
  }
  if (a00 > a11) {   // ascending eigenvalue: axis 0 minor, axis 1 major (strictly greater only: xy = 0 with xx <= yy stays the identity)
#pragma unroll
    for (int i = 0; i < 2; ++i) { const double u = W[i][0]; W[i][0] = W[i][1]; W[i][1] = u; }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    // sign: the component of largest magnitude is positive (lowest index on a tie); the z component is 0 and stays +0
    double best = W[0][j];
    if (fabs(W[1][j]) > fabs(best)) best = W[1][j];
    if (best < 0.0) { W[0][j] = -W[0][j]; W[1][j] = -W[1][j]; }
  }
  o[0] = W[0][0]; o[1] = W[0][1]; o[2] = 0.0;
  o[3] = W[1][0]; o[4] = W[1][1]; o[5] = 0.0;
  o[6] = 0.0;     o[7] = 0.0;     o[8] = 1.0;
}

// One workgroup per chunk of SD_CHUNK virtual points of one segment: the chunk -> segment -> nodes walk of segdesc.hip's sd_chunk_body
// (same staging arrays, same point of every lane and step), the projections of the header, one partial record.  Grid: the bound of
// sd_prepare; workgroups past the real number of chunks leave at once.  cen / frame: 3 and 9 doubles per label.  OWN (tile contexts,
// k_sb_chunks_own): only the points whose input index perm[pos] lies in [own_first, own_end) count -- the selection of segdesc.hip's
// k_sd_chunks_own, so the extents cover the points its n_points counts; a chunk without one writes the empty record.
template <bool OWN>
__device__ __forceinline__ void sb_chunk_body(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                              const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                              const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                              const uint32_t* __restrict__ seg_chunk, uint32_t K, const double* __restrict__ cen,
                                              const double* __restrict__ frame, double* __restrict__ part,
                                              const uint32_t* __restrict__ perm, int64_t own_first, int64_t own_end) {
  __shared__ uint32_t s_vp[SD_CHUNK];    // virtual start of the chunk's nodes
  __shared__ uint32_t s_dl[SD_CHUNK];    // sorted position - virtual position of the same (mod 2^32)
  const uint32_t c = blockIdx.x;
  SdChunk wk;
  if (!sd_walk(vox_start, ids, vp, seg_node, seg_chunk, K, s_vp, s_dl, wk)) {
    if (wk.k != 0xffffffffu) sb_empty_record(part + (size_t)c * SB_REC);   // (an empty record keeps the fold well defined)
    return;
  }
  const uint32_t k = wk.k, a = wk.a, b = wk.b, m = wk.m;
  // the projections, the butterflies and the waves in index order: segpass.hpp (its first barrier closes the staging above)
  sb_chunk_extents<OWN>(xs, ys, zs, a, b, cen + (size_t)k * 3, frame + (size_t)k * 9, [&](uint32_t q) { return sd_pos(s_vp, s_dl, m, q); },
                        part + (size_t)c * SB_REC, perm, own_first, own_end);
}

__global__ __launch_bounds__(SD_TB) void k_sb_chunks(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                     const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                     const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                                     const uint32_t* __restrict__ seg_chunk, uint32_t K, const double* __restrict__ cen,
                                                     const double* __restrict__ frame, double* __restrict__ part) {
  sb_chunk_body<false>(xs, ys, zs, vox_start, ids, vp, seg_node, seg_chunk, K, cen, frame, part, nullptr, 0, 0);
}

__global__ __launch_bounds__(SD_TB) void k_sb_chunks_own(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                         const uint32_t* __restrict__ vox_start, const uint32_t* __restrict__ ids,
                                                         const uint32_t* __restrict__ vp, const uint32_t* __restrict__ seg_node,
                                                         const uint32_t* __restrict__ seg_chunk, uint32_t K, const double* __restrict__ cen,
                                                         const double* __restrict__ frame, double* __restrict__ part,
                                                         const uint32_t* __restrict__ perm, int64_t own_first, int64_t own_end) {
  sb_chunk_body<true>(xs, ys, zs, vox_start, ids, vp, seg_node, seg_chunk, K, cen, frame, part, perm, own_first, own_end);
}

// one wavefront per segment: fold its partials (lane stride, then butterfly), then the row on lane 0
__global__ __launch_bounds__(256) void k_sb_final(const uint32_t* __restrict__ seg_chunk, const double* __restrict__ part, uint32_t n_part, uint32_t K,
                                                  const double* __restrict__ cen, const double* __restrict__ frame, double* __restrict__ o_lo,
                                                  double* __restrict__ o_hi, double* __restrict__ o_half, double* __restrict__ o_center) {
  const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= K) return;   // (whole wavefronts; no barrier follows)
  const uint32_t c0 = seg_chunk[k], c1 = min(seg_chunk[k + 1], n_part);   // (the bound only guards the records: the chunks fit, see the launch)
  double mn[3], mx[3];
  sb_fold_partials(part, c0, c1, lane, mn, mx);
  if (lane != 0) return;
  sb_box_row(k, mn, mx, cen, frame, o_lo, o_hi, o_half, o_center);
}

// k_sb_frames over K rows of evecs9 / cov6 in HBM, left on the stream: the one launch site of the frame rule (pointseg.hip calls it too)
void sb_launch_frames(vgs_ctx* c, const double* evec, const double* cov, int64_t K, int frame, double* out) {
  hipLaunchKernelGGL(k_sb_frames, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, evec, cov, (uint32_t)K, frame == VGS_BOX_UPRIGHT ? 1 : 0, out);
}

// The table of one frame in HBM, K = counts[VGS_N_KEPT] rows; valid until the next run of the stages.
vgs_status vgs_segbox_on_device(vgs_ctx* c, int frame) {
  if (c->sb_valid[frame]) return VGS_OK;
  vgs_status s = vgs_segdesc_on_device(c);   // centroid3, evecs9, cov6
  if (s != VGS_OK) return s;
  const int64_t K = c->counts[VGS_N_KEPT], V = c->V, nf = c->Nf;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const size_t k1 = (size_t)(K > 0 ? K : 1);
  VGS_HIP_TRY(c, c->sb_frame[frame].ensure(9 * k1));
  VGS_HIP_TRY(c, c->sb_lo[frame].ensure(3 * k1)); VGS_HIP_TRY(c, c->sb_hi[frame].ensure(3 * k1));
  VGS_HIP_TRY(c, c->sb_half[frame].ensure(3 * k1)); VGS_HIP_TRY(c, c->sb_center[frame].ensure(3 * k1));
  if (K == 0 || V == 0 || nf == 0) { c->sb_valid[frame] = true; return VGS_OK; }
  SdPrep P;
  if ((s = sd_prepare(c, K, P)) != VGS_OK) return s;
  VGS_HIP_TRY(c, c->sb_part.ensure((size_t)P.n_chunks_max * SB_REC));
  sb_launch_frames(c, c->sd_evec.p, c->sd_cov.p, K, frame, c->sb_frame[frame].p);
  hipLaunchKernelGGL(k_sb_chunks, dim3((unsigned)P.n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, c->vox_start.p, P.ids, P.vp,
                     P.seg_node, P.seg_chunk, (uint32_t)K, c->sd_cen.p, c->sb_frame[frame].p, c->sb_part.p);
  hipLaunchKernelGGL(k_sb_final, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, c->stream, P.seg_chunk, c->sb_part.p, (uint32_t)P.n_chunks_max,
                     (uint32_t)K, c->sd_cen.p, c->sb_frame[frame].p, c->sb_lo[frame].p, c->sb_hi[frame].p, c->sb_half[frame].p,
                     c->sb_center[frame].p);
  VGS_HIP_TRY(c, hipGetLastError());
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->sb_valid[frame] = true;
  return VGS_OK;
}

static vgs_status sb_check(vgs_ctx* c, int32_t frame, const char* fn) {
  if (frame != VGS_BOX_PRINCIPAL && frame != VGS_BOX_UPRIGHT) {
    c->err = std::string(fn) + ": frame must be VGS_BOX_PRINCIPAL (0) or VGS_BOX_UPRIGHT (1)";
    return VGS_E_ARG;
  }
  if (c->stage < ST_SEGMENTED) { c->err = std::string(fn) + ": segment first"; return VGS_E_STATE; }
  if (vgs_is_tile(c)) {
    c->err = std::string(fn) + ": a tile context (owned region / own point range) holds only part of its segments; boxes need the whole cloud in one context";
    return VGS_E_STATE;
  }
  return VGS_OK;
}

extern "C" vgs_status vgs_get_segment_boxes(vgs_ctx* c, int32_t frame, double* center3, double* half3, double* frame9, double* lo3, double* hi3) {
  if (!c) return VGS_E_ARG;
  vgs_status s = sb_check(c, frame, "vgs_get_segment_boxes");
  if (s != VGS_OK) return s;
  const size_t K = (size_t)c->counts[VGS_N_KEPT];
  if (K == 0) return VGS_OK;
  if ((s = vgs_segbox_on_device(c, frame)) != VGS_OK) return s;
  if (center3) VGS_HIP_TRY(c, hipMemcpy(center3, c->sb_center[frame].p, 3 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (half3) VGS_HIP_TRY(c, hipMemcpy(half3, c->sb_half[frame].p, 3 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (frame9) VGS_HIP_TRY(c, hipMemcpy(frame9, c->sb_frame[frame].p, 9 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (lo3) VGS_HIP_TRY(c, hipMemcpy(lo3, c->sb_lo[frame].p, 3 * K * sizeof(double), hipMemcpyDeviceToHost));
  if (hi3) VGS_HIP_TRY(c, hipMemcpy(hi3, c->sb_hi[frame].p, 3 * K * sizeof(double), hipMemcpyDeviceToHost));
  return VGS_OK;
}

extern "C" vgs_status vgs_get_segment_boxes_device(vgs_ctx* c, int32_t frame, const double** center3, const double** half3, const double** frame9,
                                                   const double** lo3, const double** hi3) {
  if (!c) return VGS_E_ARG;
  vgs_status s = sb_check(c, frame, "vgs_get_segment_boxes_device");
  if (s != VGS_OK) return s;
  if ((s = vgs_segbox_on_device(c, frame)) != VGS_OK) return s;
  if (center3) *center3 = c->sb_center[frame].p;
  if (half3) *half3 = c->sb_half[frame].p;
  if (frame9) *frame9 = c->sb_frame[frame].p;
  if (lo3) *lo3 = c->sb_lo[frame].p;
  if (hi3) *hi3 = c->sb_hi[frame].p;
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ tile contexts (include/vgs_tiles.h)
static vgs_status sbt_check_frame(vgs_ctx* c, int32_t frame, const char* fn) {
  if (frame == VGS_BOX_PRINCIPAL || frame == VGS_BOX_UPRIGHT) return VGS_OK;
  c->err = std::string(fn) + ": frame must be VGS_BOX_PRINCIPAL (0) or VGS_BOX_UPRIGHT (1)";
  return VGS_E_ARG;
}

// K rows of the descriptor table from the host into sbt_in (centroid3 | cov6 | evecs9) and their frames into sbt_frame: k_sb_frames, the
// one copy of the frame rule.  The copies are staged before they return; the launches are left on the stream.
vgs_status sbt_upload_frames(vgs_ctx* c, int64_t K, int32_t frame, const double* centroid3, const double* cov6, const double* evecs9) {
  const size_t k = (size_t)K;
  VGS_HIP_TRY(c, c->sbt_in.ensure(18 * k)); VGS_HIP_TRY(c, c->sbt_frame.ensure(9 * k)); VGS_HIP_TRY(c, c->sbt_out.ensure(12 * k));
  double *cen = c->sbt_in.p, *cov = cen + 3 * k, *evec = cov + 6 * k;
  VGS_HIP_TRY(c, hipMemcpyAsync(cen, centroid3, 3 * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipMemcpyAsync(cov, cov6, 6 * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipMemcpyAsync(evec, evecs9, 9 * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
  sb_launch_frames(c, evec, cov, K, frame, c->sbt_frame.p);
  return VGS_OK;
}

// k_sb_final over `part` into sbt_out (lo3 | hi3 | half3 | center3, K rows each), about the rows of sbt_upload_frames
void sbt_launch_final(vgs_ctx* c, int64_t K, const uint32_t* seg_chunk, const double* part, uint32_t n_part) {
  const size_t k = (size_t)K;
  double* o = c->sbt_out.p;
  hipLaunchKernelGGL(k_sb_final, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, c->stream, seg_chunk, part, n_part, (uint32_t)K, c->sbt_in.p,
                     c->sbt_frame.p, o, o + 3 * k, o + 6 * k, o + 9 * k);
}

// This rank's extents of the global labels 0 .. K-1: sd_prepare over vox_label (global after vgs_apply_tile_labels), the own-point chunks
// about the centroids and frames handed in, the per-segment fold of k_sb_final.  Dense on the device (K rows), compact on the host: a
// label without an own point keeps the empty record and is left out.
extern "C" vgs_status vgs_get_own_segment_extents(vgs_ctx* c, int64_t K, int32_t frame, const double* centroid3, const double* cov6,
                                                  const double* evecs9, int64_t* n_records, int32_t* label, double* lo3, double* hi3) {
  if (!c || !n_records || K < 0 || K >= (int64_t)0xffffffffLL || (K > 0 && (!centroid3 || !cov6 || !evecs9))) return VGS_E_ARG;
  vgs_status s = sbt_check_frame(c, frame, "vgs_get_own_segment_extents");
  if (s != VGS_OK) return s;
  if (c->stage < ST_SEGMENTED) { c->err = "vgs_get_own_segment_extents: segment first"; return VGS_E_STATE; }
  if (!c->have_region || c->n_own < 0) {
    c->err = "vgs_get_own_segment_extents: a tile context (vgs_set_owned_region and vgs_set_own_point_range) only";
    return VGS_E_STATE;
  }
  *n_records = 0;
  const int64_t V = c->V, nf = c->Nf;
  if (K == 0 || V == 0 || nf == 0) return VGS_OK;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  SdPrep P;
  if ((s = sd_prepare(c, K, P)) != VGS_OK) return s;
  VGS_HIP_TRY(c, c->sb_part.ensure((size_t)P.n_chunks_max * SB_REC));
  if ((s = sbt_upload_frames(c, K, frame, centroid3, cov6, evecs9)) != VGS_OK) return s;
  hipLaunchKernelGGL(k_sb_chunks_own, dim3((unsigned)P.n_chunks_max), dim3(SD_TB), 0, c->stream, c->xs.p, c->ys.p, c->zs.p, c->vox_start.p, P.ids,
                     P.vp, P.seg_node, P.seg_chunk, (uint32_t)K, c->sbt_in.p, c->sbt_frame.p, c->sb_part.p, c->perm_b.p, c->own_first,
                     c->own_first + c->n_own);
  sbt_launch_final(c, K, P.seg_chunk, c->sb_part.p, (uint32_t)P.n_chunks_max);
  VGS_HIP_TRY(c, hipGetLastError());
  std::vector<double> e(6 * (size_t)K);   // lo3 | hi3
  VGS_HIP_TRY(c, hipMemcpyAsync(e.data(), c->sbt_out.p, e.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  VGS_HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double* lo = e.data();
  const double* hi = lo + 3 * (size_t)K;
  int64_t n = 0;
  for (int64_t k = 0; k < K; ++k) {
    if (lo[3 * k] > hi[3 * k]) continue;   // the empty record: no own point of this label here
    if (label) label[n] = (int32_t)k;
    if (lo3) for (int f = 0; f < 3; ++f) lo3[3 * n + f] = lo[3 * k + f];
    if (hi3) for (int f = 0; f < 3; ++f) hi3[3 * n + f] = hi[3 * k + f];
    ++n;
  }
  *n_records = n;
  return VGS_OK;
}

// The table from extents folded over the ranks: one partial per segment (seg_chunk[k] = k), so k_sb_final runs unchanged.
extern "C" vgs_status vgs_segment_boxes_from_extents(vgs_ctx* c, int64_t K, int32_t frame, const double* centroid3, const double* cov6,
                                                     const double* evecs9, const double* lo3, const double* hi3, double* center3, double* half3,
                                                     double* frame9) {
  if (!c || K < 0 || K >= (int64_t)0xffffffffLL || (K > 0 && (!centroid3 || !cov6 || !evecs9 || !lo3 || !hi3))) return VGS_E_ARG;
  vgs_status s = sbt_check_frame(c, frame, "vgs_segment_boxes_from_extents");
  if (s != VGS_OK) return s;
  if (K == 0) return VGS_OK;
  VGS_HIP_TRY(c, hipSetDevice(c->device));
  const size_t k = (size_t)K;
  std::vector<double> part(SB_REC * k);
  std::vector<uint32_t> idx(k + 1);
  for (size_t i = 0; i < k; ++i) {
    for (int f = 0; f < 3; ++f) { part[SB_REC * i + f] = lo3[3 * i + f]; part[SB_REC * i + 3 + f] = hi3[3 * i + f]; }
    idx[i] = (uint32_t)i;
  }
  idx[k] = (uint32_t)k;
  VGS_HIP_TRY(c, c->sb_part.ensure(part.size())); VGS_HIP_TRY(c, c->sbt_idx.ensure(idx.size()));
  if ((s = sbt_upload_frames(c, K, frame, centroid3, cov6, evecs9)) != VGS_OK) return s;
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sb_part.p, part.data(), part.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  VGS_HIP_TRY(c, hipMemcpyAsync(c->sbt_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  sbt_launch_final(c, K, c->sbt_idx.p, c->sb_part.p, (uint32_t)K);
  VGS_HIP_TRY(c, hipGetLastError());
  const double* o = c->sbt_out.p;
  const RowCol col[3] = {{half3, o + 6 * k, 3 * sizeof(double)}, {center3, o + 9 * k, 3 * sizeof(double)}, {frame9, c->sbt_frame.p, 9 * sizeof(double)}};
  return vgs_copy_rows(c, k, col, 3);
}
