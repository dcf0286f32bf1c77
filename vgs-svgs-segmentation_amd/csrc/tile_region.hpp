// tile_region.hpp -- the region of a tile context and its grid, as k_owned (multigpu.hip) takes them: the centre of a voxel is a function of
// its global code and the shared grid only, so every rank computes the same one.  Shared by refine.hip (the band of used voxels, the reach
// of a rank's refinement) and labelcc_tiles.hip (the band of a labelling's vertices).
#ifndef VGS_TILE_REGION_HPP_
#define VGS_TILE_REGION_HPP_
#include "vgs_context.hpp"

struct RfRegion { float res_f, min_x, min_y; double lo_x, lo_y, hi_x, hi_y; };
#ifdef __HIPCC__
__device__ __forceinline__ void rf_center(const RfRegion& g, uint64_t code, double& cx, double& cy) {
  cx = (double)vm_voxel_center(vm_compact21(code >> 2), g.res_f, g.min_x);
  cy = (double)vm_voxel_center(vm_compact21(code >> 1), g.res_f, g.min_y);
}
#endif
static inline RfRegion rf_region(const vgs_ctx* c) {
  return RfRegion{c->P.voxel_size, (float)c->box.min[0], (float)c->box.min[1], c->own_lo[0], c->own_lo[1], c->own_hi[0], c->own_hi[1]};
}
#endif
