// Host check of the integer arithmetic of csrc/cutorder.hip (csrc/cutorder_arith.h): the pair index p -> (i, j) of k_co_eval and the
// partition of the used voxels into the chunks of one segmented sort.  Built and run by tests/test_cutorder_arith.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cutorder_arith.h"

static long check_pair(int64_t p, int k, int wi, int wj) {
  int i = -1, j = -1;
  co_pair_index(p, k, &i, &j);
  return (i == wi && j == wj) ? 0 : 1;
}

// every p of a small k against the enumeration itself
static long pairs_all(int k) {
  long bad = 0;
  int64_t p = 0;
  for (int i = 0; i < k; ++i)
    for (int j = i + 1; j < k; ++j, ++p) bad += check_pair(p, k, i, j);
  if (p != (int64_t)co_pairs((uint64_t)k)) ++bad;
  return bad;
}

// first and last p of every row of a large k; the row starts are summed here, not taken from co_row_start
static long pairs_row_ends(int k) {
  long bad = 0;
  int64_t start = 0;
  for (int i = 0; i + 1 < k; ++i) {
    const int64_t len = k - 1 - i;
    bad += check_pair(start, k, i, i + 1);
    bad += check_pair(start + len - 1, k, i, k - 1);
    if (co_row_start(i, k) != start) ++bad;
    start += len;
  }
  if (start != (int64_t)co_pairs((uint64_t)k)) ++bad;
  return bad;
}

// the six properties of the partition for one k[] and budget
static long chunks(const std::vector<uint32_t>& k, uint64_t budget) {
  long bad = 0;
  const int64_t U = (int64_t)k.size();
  std::vector<uint64_t> offs;
  int64_t u0 = 0, covered = 0;
  while (u0 < U) {
    const int64_t u1 = co_chunk(k.data(), U, u0, budget, offs);
    if (u1 <= u0 || u1 > U) return bad + 1;                      // consecutive, not empty (or the loop would not end)
    const int64_t m = u1 - u0;
    if ((int64_t)offs.size() != m + 1 || offs[0] != 0) return bad + 1;
    uint64_t run = 0;
    for (int64_t i = 0; i < m; ++i) {                            // offsets: running sums of k (k - 1) / 2, 0 for k = 0 and k = 1
      const uint64_t kk = k[(size_t)(u0 + i)];
      const uint64_t np = kk < 2 ? 0 : kk * (kk - 1) / 2;
      if (kk < 2 && offs[(size_t)i + 1] != offs[(size_t)i]) ++bad;
      run += np;
      if (offs[(size_t)i + 1] != run) ++bad;
    }
    if (m > 1 && offs.back() > budget) ++bad;                    // more than one voxel: within the budget
    if (m == 1 && offs.back() > budget) {                        // a single voxel above the budget: a chunk of its own
      const uint64_t kk = k[(size_t)u0];
      if (kk * (kk - 1) / 2 <= budget) ++bad;
    }
    if (u1 < U) {                                                // the chunk is full: the next voxel would not have fitted
      const uint64_t kk = k[(size_t)u1];
      if (offs.back() + (kk < 2 ? 0 : kk * (kk - 1) / 2) <= budget) ++bad;
    }
    covered += m;
    u0 = u1;                                                     // the next chunk starts where this one ends: every voxel once
  }
  if (covered != U) ++bad;
  return bad;
}

int main() {
  long bad = 0, runs = 0;
  for (int k = 2; k <= 300; ++k) { bad += pairs_all(k); ++runs; }
  const int big[] = {2047, 2048, 2049, 4224, 8191, 8192};
  for (int k : big) { bad += pairs_row_ends(k); ++runs; }
  bad += pairs_all(CO_MAXK); ++runs;                             // every pair of the largest set the kernels take
  srand(11);
  const uint64_t budgets[] = {1ull, 10ull, 1ull << 29};
  for (uint64_t budget : budgets)
    for (int it = 0; it < 3000; ++it) {
      const int U = 1 + rand() % 200;
      const int mode = it % 5;   // 0: small k, 1: mostly 0 and 1, 2: wide, 3: up to the cap, 4: rows at the budget's scale
      std::vector<uint32_t> k((size_t)U);
      for (int u = 0; u < U; ++u) {
        if (mode == 0) k[(size_t)u] = (uint32_t)(rand() % 8);
        else if (mode == 1) k[(size_t)u] = (uint32_t)(rand() % 10 < 8 ? rand() % 2 : rand() % 6);
        else if (mode == 2) k[(size_t)u] = (uint32_t)(rand() % 400);
        else if (mode == 3) k[(size_t)u] = (uint32_t)(rand() % (CO_MAXK + 1));
        else k[(size_t)u] = (uint32_t)(budget >= (1ull << 29) ? 30000 + rand() % 4000 : rand() % 7);
      }
      bad += chunks(k, budget); ++runs;
    }
  bad += chunks(std::vector<uint32_t>(), 10); ++runs;            // no used voxel: no chunk
  bad += chunks(std::vector<uint32_t>(50, 0u), 1); ++runs;
  bad += chunks(std::vector<uint32_t>(3, 40000u), 1ull << 29); ++runs;   // each above 2^29 pairs: three chunks of one
  printf("runs=%ld bad=%ld\n", runs, bad);
  return bad != 0;
}
