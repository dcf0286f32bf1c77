// unionfind.hpp -- the lock-free union-find of the connected-component passes: merge.hip (the nodes of the segmentation) and labelcc.hip
// (the (label, node) vertices of a caller's labelling).  min-hooking: a root only ever gets a parent with a smaller index, so the root
// of a finished component is its smallest member.
#ifndef VGS_UNIONFIND_HPP_
#define VGS_UNIONFIND_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {
  // path halving: parents only ever move towards the root (smaller ids), so a stale write is still an ancestor
  while (true) {
    const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    const uint32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g != p) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}
__device__ __forceinline__ void uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(&parent[hi], hi, lo) == hi) return;
  }
}

// The unions are complete: every voxel gets its ROOT as parent.  The walk must not write on the way (no path halving
// here): a halving store of another thread that lands after this voxel's final store would leave it pointing at an
// ancestor below the root, and the labels read parent[v] as the root (seen once in ~20 runs of a 90 k-point scene as a
// voxel dropped from its segment).  With read-only walks the only writes are the final ones, each a root.
__device__ __forceinline__ uint32_t uf_root(const uint32_t* parent, uint32_t x) {
  while (true) {
    const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}

#endif
