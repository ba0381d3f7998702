// The cell of a point as the cost-to-go field takes it (frontend_field.hip, view_select.hip): the map's box and the rounding of
// GridMap3D::isInMap / getGridIndex.  Both users are built with -ffp-contract=off: one subtraction, one division, one floor per axis.
#pragma once
#include "isdf_ctx.hpp"
#include <cmath>

namespace isdf {

// GridMap3D::isInMap / getGridIndex as isdf_frontend_astar_search restates them (Gridmap3D.cpp:41-69,135-175)
struct FfMap { int X, Y, Z; double res, bmin[3], bmax[3]; };
__host__ __device__ inline bool ff_cell(const FfMap &M, const double p[3], int idx[3]) {
    for (int a = 0; a < 3; a++) if (p[a] < M.bmin[a]) return false;
    for (int a = 0; a < 3; a++) if (p[a] > M.bmax[a]) return false;
    const int dims[3] = {M.X, M.Y, M.Z};
    for (int a = 0; a < 3; a++) {
        const double dd = p[a] - M.bmin[a];
        int i = (int)floor(dd / M.res);
        if (i < 0) i = 0;
        if (i >= dims[a]) i = dims[a] - 1;
        idx[a] = i;
    }
    return true;
}

inline FfMap ff_map(const isdf_ctx *c) {
    FfMap M{};
    M.X = c->grid.X; M.Y = c->grid.Y; M.Z = c->grid.Z; M.res = c->grid.res;
    for (int a = 0; a < 3; a++) { M.bmin[a] = c->grid.bmin[a]; M.bmax[a] = c->grid.bmax[a]; }
    return M;
}

}  // namespace isdf
