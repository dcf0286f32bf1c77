// cutorder_arith.h -- the two pieces of integer arithmetic of csrc/cutorder.hip that need no GPU to be checked: the pair index of
// k_co_eval and the partition of the used voxels into chunks of one segmented sort.  Plain C++ for the host check
// (tests/cpp/cutorder_check.cpp, built with g++), VGS_HD where the kernel calls it.
#pragma once
#include <stdint.h>
#include <math.h>

#include <vector>

#include "vgs_math.h"

// The largest connect set S0 whose order is replayed: the largest ball the pair-list kernel of the local cut cuts whole (localcut.hip:
// PG_XL).  Rows themselves hold up to 8192 stored entries (XL_M); positions inside a row stay below 65536 (uint16_t).
#define CO_MAXK 4224

// first pair index of row i (pairs (i, j), i < j < k, in row-major order)
VGS_HD int64_t co_row_start(int i, int k) { return (int64_t)i * (2 * k - i - 1) / 2; }

// pair p (0 <= p < k (k - 1) / 2) in row-major order over i < j < k: the sqrt gives i to within rounding, the two loops settle it
VGS_HD void co_pair_index(int64_t p, int k, int* pi, int* pj) {
  int i = (int)(((double)(2 * k - 1) - sqrt((double)(2 * k - 1) * (double)(2 * k - 1) - 8.0 * (double)p)) * 0.5);
  while (i > 0 && co_row_start(i, k) > p) --i;
  while (co_row_start(i + 1, k) <= p) ++i;
  *pi = i;
  *pj = i + 1 + (int)(p - co_row_start(i, k));
}

// pairs inside a set of k vertices (0 for k = 0 and k = 1)
inline uint64_t co_pairs(uint64_t k) { return k * (k - (k > 0 ? 1 : 0)) / 2; }

// One chunk of consecutive voxels from u0: voxels are added while the chunk's pair total stays within `budget`; the first voxel always
// goes in, so a single voxel above the budget gets a chunk of its own.  offs (cleared first) gets the running sums of the pair counts:
// offs[0] = 0, offs[i + 1] - offs[i] = pairs of voxel u0 + i.  Returns the end u1 of the chunk (u1 > u0 whenever u0 < U).
inline int64_t co_chunk(const uint32_t* k, int64_t U, int64_t u0, uint64_t budget, std::vector<uint64_t>& offs) {
  offs.assign(1, 0ull);
  int64_t u1 = u0;
  while (u1 < U) {
    const uint64_t np = co_pairs(k[u1]);
    if (u1 > u0 && offs.back() + np > budget) break;
    offs.push_back(offs.back() + np);
    ++u1;
  }
  return u1;
}
