// segpass.hpp -- the device bodies that the per-segment passes share, one copy each, so that equal points in an equal order give equal
// bytes whichever pass read them: segdesc.hip / segbox.hip walk the points of a labelling that is constant on a node (nodes sorted by
// label, each node's run of xs/ys/zs), pointseg.hip the points of any per-point labelling (sorted positions sorted by label).  What
// differs between them is where a lane's point comes from, and that is a parameter here (pos_of: virtual point q -> sorted position).
//   sd_lower_bound      the start of a label's run in sorted keys
//   sd_chunk_sums       the partial record of one chunk: sums of d = p - anchor and d d^T in fp64, min and max; the wave butterflies, the
//                       waves in index order
//   sd_fold_partials    the partials of one segment folded by one wavefront: lane stride, then butterfly
//   sd_segment_algebra  a row of the descriptor table from folded moments (centroid, covariance, Jacobi, sign rule, features)
//   sb_chunk_extents    the partial record of one chunk of the box pass: min / max of the projections onto a frame
//   sb_fold_partials, sb_box_row   the same fold for the extents, and a row of the box table from them
//   sf_chunk_sums       the partial records of one chunk of the attribute pass (segfield.hip, pointfield.hip): per channel S1, S2, count,
//                       min, max over the finite values
//   sf_hist_chunk       the class counts of one chunk: LDS counters, ballot fold, integer adds to the table; the chunk comes from a walk
//                       object (segfield.hip: sd_walk / sd_pos over staged nodes; pointfield.hip: ps_walk over pos_sorted)
#ifndef VGS_SEGPASS_HPP_
#define VGS_SEGPASS_HPP_

#include "vgs_context.hpp"

#ifdef __HIPCC__
#define SD_REC 16                   // doubles per partial record: sum d[3], sum dd^T[6] (xx xy xz yy yz zz), min[3], max[3], (pad)
#define SD_MREC 20                  // doubles per moment record of a tile context: points, nodes, min[3], max[3], anchor[3], sum d[3], sum dd^T[6]
#define SB_REC 6                    // doubles per partial record of the box pass: min t[3], max t[3]

// first position of the sorted keys (n of them) that is not below k: the start of label k's run
__device__ __forceinline__ uint32_t sd_lower_bound(const uint32_t* __restrict__ key, uint32_t n, uint32_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (key[mid] < k) lo = mid + 1; else hi = mid; }
  return lo;
}

__device__ __forceinline__ double sd_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}
__device__ __forceinline__ float sd_wave_min(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fminf(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ float sd_wave_max(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m, 64));
  return x;
}

// Empty partial record: zero sums and count, +inf min, -inf max
__device__ __forceinline__ void sd_empty_record(double* __restrict__ rec) {
  if (threadIdx.x < SD_REC) {
    const int f = threadIdx.x;
    rec[f] = f < 9 ? 0.0 : (f < 12 ? __builtin_huge_val() : (f < 15 ? -__builtin_huge_val() : 0.0));
  }
}

// The partial record of the chunk [a, b) of virtual points (b - a <= SD_CHUNK) about the anchor (ax, ay, az), by a workgroup of SD_TB
// threads: the point of a lane at step `it` is pos_of(a + it * SD_TB + tid), the lanes fold by a fixed butterfly, the waves in index
// order.  OWN (tile contexts): only the points whose input index perm[pos] lies in [own_first, own_end) count -- in the sums, the min /
// max and the point count (field 15).  Every thread of the workgroup calls it (two barriers inside).
template <bool OWN, typename PosOf>
__device__ __forceinline__ void sd_chunk_sums(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                              uint32_t a, uint32_t b, double ax, double ay, double az, PosOf pos_of,
                                              double* __restrict__ rec, const uint32_t* __restrict__ perm, int64_t own_first, int64_t own_end) {
  __shared__ double s_red[SD_TB / 64][SD_REC];
  __syncthreads();
  double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0, cnt = 0;
  float mnx = __builtin_huge_valf(), mny = __builtin_huge_valf(), mnz = __builtin_huge_valf();
  float mxx = -__builtin_huge_valf(), mxy = -__builtin_huge_valf(), mxz = -__builtin_huge_valf();
#pragma unroll 2
  for (int it = 0; it < SD_PPT; ++it) {
    const uint32_t q = a + (uint32_t)it * SD_TB + threadIdx.x;
    if (q < b) {
      const uint32_t pos = pos_of(q);
      if (OWN) {
        const int64_t o = (int64_t)perm[pos];
        if (o < own_first || o >= own_end) continue;
        cnt += 1.0;
      }
      const float x = xs[pos], y = ys[pos], z = zs[pos];
      mnx = fminf(mnx, x); mny = fminf(mny, y); mnz = fminf(mnz, z);
      mxx = fmaxf(mxx, x); mxy = fmaxf(mxy, y); mxz = fmaxf(mxz, z);
      // exact differences (two floats, one double); products and sums in fp64
      const double dx = (double)x - ax, dy = (double)y - ay, dz = (double)z - az;
      sx += dx; sy += dy; sz += dz;
      sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
    }
  }
  sx = sd_wave_sum(sx); sy = sd_wave_sum(sy); sz = sd_wave_sum(sz);
  sxx = sd_wave_sum(sxx); sxy = sd_wave_sum(sxy); sxz = sd_wave_sum(sxz); syy = sd_wave_sum(syy); syz = sd_wave_sum(syz); szz = sd_wave_sum(szz);
  if (OWN) cnt = sd_wave_sum(cnt);
  mnx = sd_wave_min(mnx); mny = sd_wave_min(mny); mnz = sd_wave_min(mnz);
  mxx = sd_wave_max(mxx); mxy = sd_wave_max(mxy); mxz = sd_wave_max(mxz);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    double* r = s_red[w];
    r[0] = sx; r[1] = sy; r[2] = sz; r[3] = sxx; r[4] = sxy; r[5] = sxz; r[6] = syy; r[7] = syz; r[8] = szz;
    r[9] = mnx; r[10] = mny; r[11] = mnz; r[12] = mxx; r[13] = mxy; r[14] = mxz; r[15] = OWN ? cnt : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < SD_REC) {   // the waves in index order
    const int f = threadIdx.x;
    double v = s_red[0][f];
    if (f < 9 || (OWN && f == 15)) { for (int u = 1; u < SD_TB / 64; ++u) v += s_red[u][f]; }
    else if (f < 12) { for (int u = 1; u < SD_TB / 64; ++u) v = fmin(v, s_red[u][f]); }
    else if (f < 15) { for (int u = 1; u < SD_TB / 64; ++u) v = fmax(v, s_red[u][f]); }
    rec[f] = v;
  }
}

// One Jacobi rotation that zeroes A[p][q] (Numerical Recipes' jacobi: A' = J^T A J, W' = W J; r = the third index)
template <int p, int q>
__device__ __forceinline__ void sd_jacobi_rotate(double (&A)[3][3], double (&W)[3][3]) {
  constexpr int r = 3 - p - q;
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
  const double arp = A[r][p], arq = A[r][q];
  A[p][p] -= t * apq;
  A[q][q] += t * apq;
  A[p][q] = 0.0; A[q][p] = 0.0;
  const double nrp = cs * arp - sn * arq, nrq = sn * arp + cs * arq;
  A[r][p] = nrp; A[p][r] = nrp; A[r][q] = nrq; A[q][r] = nrq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double wp = W[i][p], wq = W[i][q];
    W[i][p] = cs * wp - sn * wq;
    W[i][q] = sn * wp + cs * wq;
  }
}

template <int a, int b>
__device__ __forceinline__ void sd_order_pair(double (&d)[3], double (&W)[3][3]) {
  if (d[a] > d[b]) {
    const double t = d[a]; d[a] = d[b]; d[b] = t;
#pragma unroll
    for (int i = 0; i < 3; ++i) { const double u = W[i][a]; W[i][a] = W[i][b]; W[i][b] = u; }
  }
}

// The partials c0 .. c1 of one segment folded by one wavefront: lane stride, then butterfly; min / max come back as float values.
// CNT: field 15 (the own-point count of k_sd_chunks_own) too.
template <bool CNT>
__device__ __forceinline__ void sd_fold_partials(const double* __restrict__ part, uint32_t c0, uint32_t c1, uint32_t lane, double (&s)[9],
                                                 double (&mn)[3], double (&mx)[3], double& cnt) {
#pragma unroll
  for (int f = 0; f < 9; ++f) s[f] = 0.0;
#pragma unroll
  for (int f = 0; f < 3; ++f) { mn[f] = __builtin_huge_val(); mx[f] = -__builtin_huge_val(); }
  if (CNT) cnt = 0.0;
  for (uint32_t c = c0 + lane; c < c1; c += 64) {
    const double* r = part + (size_t)c * SD_REC;
#pragma unroll
    for (int f = 0; f < 9; ++f) s[f] += r[f];
#pragma unroll
    for (int f = 0; f < 3; ++f) { mn[f] = fmin(mn[f], r[9 + f]); mx[f] = fmax(mx[f], r[12 + f]); }
    if (CNT) cnt += r[15];
  }
#pragma unroll
  for (int f = 0; f < 9; ++f) s[f] = sd_wave_sum(s[f]);
  if (CNT) cnt = sd_wave_sum(cnt);
#pragma unroll
  for (int f = 0; f < 3; ++f) { mn[f] = (double)sd_wave_min((float)mn[f]); mx[f] = (double)sd_wave_max((float)mx[f]); }
}

// Row k of the table from a segment's folded moments: n points, n_nodes nodes, min / max, the anchor (a point of the segment, as
// doubles) and s = sum d, sum d d^T (xx xy xz yy yz zz) with d = p - anchor.  Centroid, population covariance, cyclic Jacobi in fp64,
// the sign rule and the features.  The one copy of this algebra: k_sd_final (one context), k_sd_algebra (moments folded over tiles) and
// k_ps_final (a caller's point labelling, pointseg.hip) all call it, so equal moments give equal bytes.
__device__ __forceinline__ void sd_segment_algebra(size_t k, int64_t n, int32_t n_nodes, const double (&mn)[3], const double (&mx)[3],
                                                   const double (&anc)[3], const double (&s)[9], int svgs, int64_t* __restrict__ o_npts,
                                                   int32_t* __restrict__ o_nnodes, float* __restrict__ o_bbox, double* __restrict__ o_cen,
                                                   double* __restrict__ o_cov, double* __restrict__ o_eval, double* __restrict__ o_evec,
                                                   float* __restrict__ o_eig8) {
  o_npts[k] = n;
  o_nnodes[k] = n_nodes;
#pragma unroll
  for (int f = 0; f < 3; ++f) { o_bbox[6 * k + f] = (float)mn[f]; o_bbox[6 * k + 3 + f] = (float)mx[f]; }
  const double inv = n > 0 ? 1.0 / (double)n : 0.0;   // (n = 0: no point anywhere -- zero moments about the anchor)
  const double md[3] = {s[0] * inv, s[1] * inv, s[2] * inv};
#pragma unroll
  for (int f = 0; f < 3; ++f) o_cen[3 * k + f] = anc[f] + md[f];
  // population covariance about the mean: E[d d^T] - E[d] E[d]^T, d relative to a point of the segment
  double cv[6];
  cv[0] = s[3] * inv - md[0] * md[0]; cv[1] = s[4] * inv - md[0] * md[1]; cv[2] = s[5] * inv - md[0] * md[2];
  cv[3] = s[6] * inv - md[1] * md[1]; cv[4] = s[7] * inv - md[1] * md[2]; cv[5] = s[8] * inv - md[2] * md[2];
  if (n <= 1) { for (int f = 0; f < 6; ++f) cv[f] = 0.0; }
#pragma unroll
  for (int f = 0; f < 6; ++f) o_cov[6 * k + f] = cv[f];
  // cyclic Jacobi in fp64 until the off-diagonal part is negligible against the diagonal
  double A[3][3] = {{cv[0], cv[1], cv[2]}, {cv[1], cv[3], cv[4]}, {cv[2], cv[4], cv[5]}};
  double W[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off == 0.0 || off <= 1e-36 * dia) break;
    sd_jacobi_rotate<0, 1>(A, W);
    sd_jacobi_rotate<0, 2>(A, W);
    sd_jacobi_rotate<1, 2>(A, W);
  }
  double d[3] = {A[0][0], A[1][1], A[2][2]};
  sd_order_pair<0, 1>(d, W);
  sd_order_pair<1, 2>(d, W);
  sd_order_pair<0, 1>(d, W);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // sign: the component of largest magnitude is positive (lowest index on a tie)
    double best = W[0][j];
    if (fabs(W[1][j]) > fabs(best)) best = W[1][j];
    if (fabs(W[2][j]) > fabs(best)) best = W[2][j];
    if (best < 0.0) { W[0][j] = -W[0][j]; W[1][j] = -W[1][j]; W[2][j] = -W[2][j]; }
    d[j] = d[j] > 0.0 ? d[j] : 0.0;
    o_eval[3 * k + j] = d[j];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) o_evec[9 * k + 3 * r + j] = W[r][j];
  const float ef[3] = {(float)d[0], (float)d[1], (float)d[2]};
  float F[8];
  vm_eigen_features(ef, svgs, F);
#pragma unroll
  for (int f = 0; f < 8; ++f) o_eig8[8 * k + f] = F[f];
}

// ---------------------------------------------------------------------------------------------------------------- the box pass
__device__ __forceinline__ double sb_wave_min(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmin(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ double sb_wave_max(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m, 64));
  return x;
}

// Empty partial record: +inf min, -inf max
__device__ __forceinline__ void sb_empty_record(double* __restrict__ rec) {
  if (threadIdx.x < SB_REC) rec[threadIdx.x] = threadIdx.x < 3 ? __builtin_huge_val() : -__builtin_huge_val();
}

// The partial record of the chunk [a, b) of virtual points of one segment, about its centroid cc[3] in its frame ww[9]: t_j = (W[0][j] dx +
// W[1][j] dy) + W[2][j] dz for d = p - c in fp64, per-lane min / max, wavefront butterfly, the waves through LDS.  The point of every lane
// and step, OWN and the barriers as in sd_chunk_sums.
template <bool OWN, typename PosOf>
__device__ __forceinline__ void sb_chunk_extents(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                 uint32_t a, uint32_t b, const double* __restrict__ cc, const double* __restrict__ ww,
                                                 PosOf pos_of, double* __restrict__ rec, const uint32_t* __restrict__ perm, int64_t own_first,
                                                 int64_t own_end) {
  __shared__ double s_red[SD_TB / 64][SB_REC];
  const double cx = cc[0], cy = cc[1], cz = cc[2];
  const double w00 = ww[0], w01 = ww[1], w02 = ww[2], w10 = ww[3], w11 = ww[4], w12 = ww[5], w20 = ww[6], w21 = ww[7], w22 = ww[8];
  __syncthreads();
  double mn0 = __builtin_huge_val(), mn1 = __builtin_huge_val(), mn2 = __builtin_huge_val();
  double mx0 = -__builtin_huge_val(), mx1 = -__builtin_huge_val(), mx2 = -__builtin_huge_val();
#pragma unroll 2
  for (int it = 0; it < SD_PPT; ++it) {
    const uint32_t q = a + (uint32_t)it * SD_TB + threadIdx.x;
    if (q < b) {
      const uint32_t pos = pos_of(q);
      if (OWN) {
        const int64_t o = (int64_t)perm[pos];
        if (o < own_first || o >= own_end) continue;
      }
      // exact differences (a float against a double), then one fp64 operation per product and sum, in this association
      const double dx = (double)xs[pos] - cx, dy = (double)ys[pos] - cy, dz = (double)zs[pos] - cz;
      const double t0 = (w00 * dx + w10 * dy) + w20 * dz;
      const double t1 = (w01 * dx + w11 * dy) + w21 * dz;
      const double t2 = (w02 * dx + w12 * dy) + w22 * dz;
      mn0 = fmin(mn0, t0); mn1 = fmin(mn1, t1); mn2 = fmin(mn2, t2);
      mx0 = fmax(mx0, t0); mx1 = fmax(mx1, t1); mx2 = fmax(mx2, t2);
    }
  }
  mn0 = sb_wave_min(mn0); mn1 = sb_wave_min(mn1); mn2 = sb_wave_min(mn2);
  mx0 = sb_wave_max(mx0); mx1 = sb_wave_max(mx1); mx2 = sb_wave_max(mx2);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    double* r = s_red[w];
    r[0] = mn0; r[1] = mn1; r[2] = mn2; r[3] = mx0; r[4] = mx1; r[5] = mx2;
  }
  __syncthreads();
  if (threadIdx.x < SB_REC) {   // the waves in index order
    const int f = threadIdx.x;
    double v = s_red[0][f];
    if (f < 3) { for (int u = 1; u < SD_TB / 64; ++u) v = fmin(v, s_red[u][f]); }
    else { for (int u = 1; u < SD_TB / 64; ++u) v = fmax(v, s_red[u][f]); }
    rec[f] = v;
  }
}

// the extent partials c0 .. c1 of one segment folded by one wavefront: lane stride, then butterfly
__device__ __forceinline__ void sb_fold_partials(const double* __restrict__ part, uint32_t c0, uint32_t c1, uint32_t lane, double (&mn)[3],
                                                 double (&mx)[3]) {
#pragma unroll
  for (int f = 0; f < 3; ++f) { mn[f] = __builtin_huge_val(); mx[f] = -__builtin_huge_val(); }
  for (uint32_t c = c0 + lane; c < c1; c += 64) {
    const double* r = part + (size_t)c * SB_REC;
#pragma unroll
    for (int f = 0; f < 3; ++f) { mn[f] = fmin(mn[f], r[f]); mx[f] = fmax(mx[f], r[3 + f]); }
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) { mn[f] = sb_wave_min(mn[f]); mx[f] = sb_wave_max(mx[f]); }
}

// row k of the box table from its folded extents, about the centroid and in the frame of row k
__device__ __forceinline__ void sb_box_row(size_t k, const double (&mn)[3], const double (&mx)[3], const double* __restrict__ cen,
                                           const double* __restrict__ frame, double* __restrict__ o_lo, double* __restrict__ o_hi,
                                           double* __restrict__ o_half, double* __restrict__ o_center) {
  const double* W = frame + k * 9;
  double mid[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    o_lo[3 * k + f] = mn[f];
    o_hi[3 * k + f] = mx[f];
    o_half[3 * k + f] = (mx[f] - mn[f]) * 0.5;
    mid[f] = (mn[f] + mx[f]) * 0.5;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o_center[3 * k + r] = cen[3 * k + r] + ((W[3 * r + 0] * mid[0] + W[3 * r + 1] * mid[1]) + W[3 * r + 2] * mid[2]);
}

// ------------------------------------------------------------------------------------- chunks of a per-point labelling (ps_sort_points)
// The walk of a chunk workgroup (blockIdx.x) from chunk to label: the label k of the chunk, the start s0 of the label's run and the
// chunk's range [a, b) in pos_sorted.  False for a workgroup past the real number of chunks.
struct PsChunk { uint32_t k, s0, a, b; };
__device__ __forceinline__ bool ps_walk(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_chunk, uint32_t K, PsChunk& o) {
  const uint32_t c = blockIdx.x;
  if (c >= seg_chunk[K]) return false;
  // label of chunk c: the last k with seg_chunk[k] <= c -- a label without a chunk shares its value with the next one and is passed over
  uint32_t lo = 0, hi = K - 1;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if (seg_chunk[mid] <= c) lo = mid; else hi = mid - 1; }
  o.k = lo;
  o.s0 = seg_start[lo];
  o.a = o.s0 + (c - seg_chunk[lo]) * SD_CHUNK;
  o.b = min(o.a + (uint32_t)SD_CHUNK, seg_start[lo + 1]);
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- the attribute passes
// segfield.hip walks the points of the node labelling (pos_of = sd_pos over the staged nodes), pointfield.hip those of a caller's per-point
// labelling (pos_of = pos_sorted[q]); the row of a point is field + perm[pos] * stride.
#define SF_G 4     // channels per pass over the points: 4 x (S1, S2, count, min, max) stay in registers
#define SF_REC 5   // doubles per partial record of one (chunk, channel): S1, S2, count, min, max

__device__ __forceinline__ double sf_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}
__device__ __forceinline__ double sf_wave_min(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmin(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ double sf_wave_max(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ bool sf_valid(float x) { return fabsf(x) < __builtin_huge_valf(); }   // finite: false for NaN and +-inf

// The partial records of the chunk [a, b) of virtual points (b - a <= SD_CHUNK) for the channels c0 .. c0 + ng - 1 (ng <= SF_G) of the
// field, about the anchors an[]: per channel, over the finite values, S1 = sum d, S2 = sum d d with d = (double)x - anchor, the count,
// min and max.  The point of a lane at step `it` is pos_of(a + it * SD_TB + tid); wavefront butterfly, the waves through LDS in index
// order.  OWN (tile contexts): only the points whose input index o = perm[pos] lies in [own_first, own_end) count, and their row is
// field + (o - own_first) * stride.  Every thread of the workgroup calls it (two barriers inside; the first also covers what the caller
// staged in LDS for pos_of).
template <bool OWN, typename PosOf>
__device__ __forceinline__ void sf_chunk_sums(const float* __restrict__ field, int64_t stride_f, uint32_t c0, uint32_t ng, uint32_t a, uint32_t b,
                                              const double (&an)[SF_G], PosOf pos_of, const uint32_t* __restrict__ perm, int64_t own_first,
                                              int64_t own_end, double* __restrict__ rec) {
  __shared__ double s_red[SD_TB / 64][SF_G][SF_REC];
  __syncthreads();
  double s1[SF_G], s2[SF_G], cn[SF_G];
  float mn[SF_G], mx[SF_G];
#pragma unroll
  for (int g = 0; g < SF_G; ++g) { s1[g] = 0.0; s2[g] = 0.0; cn[g] = 0.0; mn[g] = __builtin_huge_valf(); mx[g] = -__builtin_huge_valf(); }
#pragma unroll 2
  for (int it = 0; it < SD_PPT; ++it) {
    const uint32_t q = a + (uint32_t)it * SD_TB + threadIdx.x;
    if (q < b) {
      const uint32_t pos = pos_of(q);
      size_t ri = (size_t)perm[pos];
      if (OWN) {
        const int64_t o = (int64_t)ri;
        if (o < own_first || o >= own_end) continue;
        ri = (size_t)(o - own_first);
      }
      const float* row = field + ri * (size_t)stride_f + c0;
#pragma unroll
      for (int g = 0; g < SF_G; ++g) {
        if ((uint32_t)g < ng) {
          const float x = row[g];
          if (sf_valid(x)) {
            const double d = (double)x - an[g];   // exact conversion, then one fp64 operation per difference, product and sum
            s1[g] += d;
            s2[g] += d * d;
            cn[g] += 1.0;
            mn[g] = fminf(mn[g], x);
            mx[g] = fmaxf(mx[g], x);
          }
        }
      }
    }
  }
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int g = 0; g < SF_G; ++g) {
    const double a1 = sf_wave_sum(s1[g]), a2 = sf_wave_sum(s2[g]), a3 = sf_wave_sum(cn[g]);
    const double a4 = sf_wave_min((double)mn[g]), a5 = sf_wave_max((double)mx[g]);
    if ((threadIdx.x & 63) == 0) {
      double* r = s_red[wv][g];
      r[0] = a1; r[1] = a2; r[2] = a3; r[3] = a4; r[4] = a5;
    }
  }
  __syncthreads();
  if (threadIdx.x < SF_G * SF_REC) {   // the waves in index order
    const int g = threadIdx.x / SF_REC, f = threadIdx.x % SF_REC;
    double v = s_red[0][g][f];
    if (f < 3) { for (int u = 1; u < SD_TB / 64; ++u) v += s_red[u][g][f]; }
    else if (f == 3) { for (int u = 1; u < SD_TB / 64; ++u) v = fmin(v, s_red[u][g][f]); }
    else { for (int u = 1; u < SD_TB / 64; ++u) v = fmax(v, s_red[u][g][f]); }
    rec[threadIdx.x] = v;
  }
}

// One workgroup per chunk: the classes of its points counted in LDS (slot n_classes: out of range; a wavefront first folds the lanes that
// share its first active lane's class into one add), the non-zero counters added to the zeroed tables hist (K x n_classes) and n_outside
// (K).  Integer atomics: the sums do not depend on the order.  walk.begin(k, a, b) gives the chunk's label and its range [a, b) of virtual
// points (false: the workgroup has no chunk) and may stage what walk.pos(q), the sorted position of the virtual point q, reads from LDS --
// the barrier behind the zeroing covers it.  OWN as in sf_chunk_sums, the class of an own point being cls[o - own_first].
template <bool OWN, typename Walk>
__device__ __forceinline__ void sf_hist_chunk(const int32_t* __restrict__ cls, uint32_t n_classes, const uint32_t* __restrict__ perm, Walk walk,
                                              unsigned long long* __restrict__ hist, unsigned long long* __restrict__ n_outside, int64_t own_first,
                                              int64_t own_end) {
  __shared__ uint32_t s_cnt[1024 + 1];
  uint32_t k, a, b;
  if (!walk.begin(k, a, b)) return;
  for (uint32_t j = threadIdx.x; j <= n_classes; j += SD_TB) s_cnt[j] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  for (int it = 0; it < SD_PPT; ++it) {
    const uint32_t q = a + (uint32_t)it * SD_TB + threadIdx.x;
    bool act = q < b;
    uint32_t slot = 0;
    if (act) {
      size_t ri = (size_t)perm[walk.pos(q)];
      if (OWN) {
        const int64_t o = (int64_t)ri;
        act = o >= own_first && o < own_end;
        ri = act ? (size_t)(o - own_first) : 0;
      }
      if (act) {
        const int32_t v = cls[ri];
        slot = (v < 0 || (uint32_t)v >= n_classes) ? n_classes : (uint32_t)v;
      }
    }
    // the lanes that share the first active lane's class fold into one add; the others add one each
    const uint64_t am = __ballot(act);
    if (am == 0) continue;
    const uint32_t first = (uint32_t)__ffsll((unsigned long long)am) - 1u;
    const uint32_t lead = __shfl(slot, (int)first, 64);
    const uint64_t peers = __ballot(act && slot == lead);
    if (lane == first) atomicAdd(&s_cnt[lead], (uint32_t)__popcll(peers));
    else if (act && slot != lead) atomicAdd(&s_cnt[slot], 1u);
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j <= n_classes; j += SD_TB) {
    const uint32_t v = s_cnt[j];
    if (v == 0) continue;
    if (j < n_classes) atomicAdd(hist + (size_t)k * n_classes + j, (unsigned long long)v);
    else atomicAdd(n_outside + k, (unsigned long long)v);
  }
}

#endif   // __HIPCC__

#endif
