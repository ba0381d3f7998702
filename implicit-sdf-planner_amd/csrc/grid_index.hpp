// The voxel a world point falls in: GridMap3D::getGridIndex (Gridmap3D.cpp:135-175).  One statement of the arithmetic for every
// kernel that bins points (map_build.hip: the point cloud's counts; points_merge.hip: the obstacle-point set's voxels).
#pragma once
#include "isdf_internal.hpp"

namespace isdf {
// false: the point lies outside the map, where the reference answers voxel (0, 0, 0) (:137-140) - (ix, iy, iz) are that voxel then
__device__ __forceinline__ bool grid_index(const DevGrid &G, double x, double y, double z, int &ix, int &iy, int &iz) {
    ix = 0; iy = 0; iz = 0;
    const bool in = !(x < G.bmin[0] || y < G.bmin[1] || z < G.bmin[2] || x > G.bmax[0] || y > G.bmax[1] || z > G.bmax[2]);
    if (in) {
        ix = (int)floor((x - G.bmin[0]) / G.res); iy = (int)floor((y - G.bmin[1]) / G.res); iz = (int)floor((z - G.bmin[2]) / G.res);
        if (ix >= G.X) ix = G.X - 1;       // the lower clamps of :149-168 cannot trigger inside the map
        if (iy >= G.Y) iy = G.Y - 1;
        if (iz >= G.Z) iz = G.Z - 1;
    }
    return in;
}
}  // namespace isdf
