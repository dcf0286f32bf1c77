// wavefold.hpp -- the wavefront-wide folds of the graph passes (seggraph.hip, labelgraph.hip): fixed xor butterflies over the 64 lanes,
// so that every lane ends with the same value and a sum's shape depends on the lane count alone; and the test whether a stored adjacency
// row holds a node.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

__device__ __forceinline__ double sg_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}
__device__ __forceinline__ long long sg_wave_sum(long long x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}
__device__ __forceinline__ int sg_wave_sum(int x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}
__device__ __forceinline__ int sg_wave_min(int x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = min(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ float sg_wave_min(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fminf(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ float sg_wave_max(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m, 64));
  return x;
}

// is u in the row of v?  The pair's key there is the same d2 bits with id u (the predicate is symmetric); a linear scan for the id backs
// the binary search up, so only a real absence counts
__device__ __forceinline__ bool sg_in_row(const uint64_t* __restrict__ row, uint32_t n, uint64_t key, uint32_t u) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (row[mid] < key) lo = mid + 1; else hi = mid; }
  if (lo < n && row[lo] == key) return true;
  for (uint32_t k = 0; k < n; ++k) if ((uint32_t)row[k] == u) return true;
  return false;
}
