// Cost-to-go field of one goal over the front end's free graph, host form (no device, no HIP): Dijkstra with a binary heap.
// Graph = that of AstarPathSearcher::AstarGetSucc (front_end_Astar.hpp:197-236): voxel v is FREE when any attitude bit of its word of
// the configuration-space table is set (occupied voxels hold 0); a step goes to any of the 26 neighbours that is free and inside the
// map; its cost is edge[i*i + j*j + k*k] = sqrt(i*i + j*j + k*k), in cells (:230).
//   d[goal] = 0;  d[v] = min over free neighbours u of fl(d[u] + w(u, v)) for free v, the least fixed point from +inf;
//   +inf on voxels that are not free or cannot reach the goal; everything +inf when the goal cell is not free.
// One plain fp64 addition per candidate (build without FMA contraction - there is no product to contract, the rule is for the record).
// Addition is monotone and every value is a real path's length summed from the goal outward, so EVERY relaxation order that reaches a
// fixed point reaches these bytes: the device form (frontend_field.hip) is held to this one byte for byte.
// "Any bit set" equals the reference's checkKernelValue (sw_manager.hpp:911-942) when the parent's attitude lies on the attitude grid
// and the grid has at most 801 attitudes: visit_kernels_by_distance (:850-909) pops at most maxdeepth + 1 = 801 attitudes, and only
// then does its breadth-first order reach every attitude of the grid.
#pragma once
#include "map_shift_host.hpp"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace isdf_host {

inline bool field_voxel_free(const uint32_t *mask, size_t nw, size_t v) {
    uint32_t any = 0;
    for (size_t w = 0; w < nw; w++) any |= mask[nw * v + w];
    return any != 0u;
}

// a binary min-heap of (key, voxel); stale entries are skipped by the consumer
struct FieldHeap {
    struct E { double key; size_t v; };
    std::vector<E> heap;
    bool empty() const { return heap.empty(); }
    void push(double key, size_t v) {
        heap.push_back(E{key, v});
        size_t i = heap.size() - 1;
        while (i > 0) { const size_t p = (i - 1) >> 1; if (!(heap[i].key < heap[p].key)) break; std::swap(heap[i], heap[p]); i = p; }
    }
    E pop() {
        const E top = heap[0];
        heap[0] = heap.back(); heap.pop_back();
        const size_t m = heap.size();
        for (size_t i = 0;;) {
            const size_t l = 2 * i + 1, r = l + 1; size_t s = i;
            if (l < m && heap[l].key < heap[s].key) s = l;
            if (r < m && heap[r].key < heap[s].key) s = r;
            if (s == i) break;
            std::swap(heap[i], heap[s]); i = s;
        }
        return top;
    }
};

// Dijkstra's loop from whatever the heap holds: every popped voxel offers fl(key + w) to its free neighbours
inline void field_relax_heap(const uint32_t *mask, int X, int Y, int Z, size_t nw, FieldHeap &heap, double *d) {
    const size_t YZ = (size_t)Y * Z;
    double edge[4];
    for (int q = 0; q < 4; q++) edge[q] = std::sqrt((double)q);
    while (!heap.empty()) {
        const FieldHeap::E e = heap.pop();
        if (e.key > d[e.v]) continue;                     // a stale entry: the voxel was lowered after this one was pushed
        const int x = (int)(e.v / YZ), y = (int)((e.v / Z) % Y), z = (int)(e.v % Z);
        for (int i = -1; i < 2; i++)
            for (int j = -1; j < 2; j++)
                for (int k = -1; k < 2; k++) {
                    if (!(i | j | k)) continue;
                    const int vx = x + i, vy = y + j, vz = z + k;
                    if (vx < 0 || vx >= X || vy < 0 || vy >= Y || vz < 0 || vz >= Z) continue;
                    const size_t u = (size_t)vx * YZ + (size_t)vy * Z + (size_t)vz;
                    if (!field_voxel_free(mask, nw, u)) continue;
                    const double cand = e.key + edge[i * i + j * j + k * k];
                    if (cand < d[u]) { d[u] = cand; heap.push(cand, u); }
                }
    }
}

// the goal's voxel in grid order (z fastest); false: a component lies outside the map = no goal
inline bool field_goal_voxel(int X, int Y, int Z, const int goal[3], size_t *g) {
    if (goal[0] < 0 || goal[0] >= X || goal[1] < 0 || goal[1] >= Y || goal[2] < 0 || goal[2] >= Z) return false;
    *g = ((size_t)goal[0] * Y + (size_t)goal[1]) * Z + (size_t)goal[2];
    return true;
}

// what the two in-place changes start from: one byte per voxel, free in the mask or not, and their count
inline std::vector<unsigned char> field_free_bytes(const uint32_t *mask, size_t nw, size_t n, long long *n_free) {
    std::vector<unsigned char> fr(n);
    for (size_t v = 0; v < n; v++) {
        fr[v] = field_voxel_free(mask, nw, v) ? 1 : 0;
        *n_free += fr[v];
    }
    return fr;
}

// mask: nw = 4 * ceil(n_att / 128) dwords per voxel, grid order (z fastest).  goal: voxel index, any component outside the map = no goal.
// d_out: X * Y * Z doubles.  Returns true when the goal cell is inside the map and free.
inline bool field_dijkstra(const uint32_t *mask, int X, int Y, int Z, int n_att, const int goal[3], double *d_out) {
    const size_t nw = 4 * (size_t)((n_att + 127) / 128);
    const size_t n = (size_t)X * Y * Z;
    const double inf = std::numeric_limits<double>::infinity();
    for (size_t v = 0; v < n; v++) d_out[v] = inf;
    size_t g;
    if (!field_goal_voxel(X, Y, Z, goal, &g) || !field_voxel_free(mask, nw, g)) return false;
    FieldHeap heap;
    d_out[g] = 0.0;
    heap.push(0.0, g);
    field_relax_heap(mask, X, Y, Z, nw, heap, d_out);
    return true;
}

// The field REPAIRED after voxels closed (occupancy only grows).  d: the field of the same goal on a mask of which
// mask_new is a subset (every voxel free in mask_new was free before) - the premise; nothing here can check it.
//   tau = the smallest d over the voxels with a finite d whose new word is 0 (the closed voxels that had been reached), +inf if none;
//   every d < tau is kept: the chain of minimising neighbours from such a voxel to the goal only passes voxels with d < tau, none of
//   them closed, so the old value is still reached, and the new graph being a subgraph it cannot be beaten;
//   every finite d >= tau becomes +inf, and Dijkstra runs on from the kept voxels as its sources.
// The result has the bytes of field_dijkstra on mask_new.  Returns true when the goal cell is inside the map and free in mask_new.
struct FieldRepairCounts { long long closed_reached = 0, reset_voxels = 0, free_voxels = 0, reached_voxels = 0; double tau = 0.0; };
// tau_left: the smallest d of reached voxels that are no longer part of d at all (field_shift's leaving voxels); they closed as well.
inline bool field_repair(const uint32_t *mask_new, int X, int Y, int Z, int n_att, const int goal[3], double *d, FieldRepairCounts *counts,
                         double tau_left = std::numeric_limits<double>::infinity()) {
    const size_t nw = 4 * (size_t)((n_att + 127) / 128);
    const size_t n = (size_t)X * Y * Z;
    const double inf = std::numeric_limits<double>::infinity();
    FieldRepairCounts C;
    C.tau = tau_left;
    const std::vector<unsigned char> fr = field_free_bytes(mask_new, nw, n, &C.free_voxels);
    for (size_t v = 0; v < n; v++)
        if (!fr[v] && d[v] < inf) { C.closed_reached++; if (d[v] < C.tau) C.tau = d[v]; }
    FieldHeap heap;
    for (size_t v = 0; v < n; v++) {
        if (!(d[v] < inf)) continue;
        if (d[v] >= C.tau) { d[v] = inf; C.reset_voxels++; }
        else heap.push(d[v], v);
    }
    field_relax_heap(mask_new, X, Y, Z, nw, heap, d);
    for (size_t v = 0; v < n; v++) C.reached_voxels += d[v] < inf;
    if (counts) *counts = C;
    size_t g;
    return field_goal_voxel(X, Y, Z, goal, &g) && fr[g] != 0;
}

// The field LOWERED after voxels opened (occupancy only shrinks).  d: the field of the same goal on a mask of which
// mask_new is a superset (every voxel free before is free in mask_new) - the premise; nothing here can check it.
//   every old value is kept: it is the length of a path that still exists, an upper bound of the new least fixed point;
//   the goal cell, free in mask_new and +inf, takes 0 (it had not been free: the field was all +inf);
//   the heap is seeded from the finite neighbours of the voxels that are free and +inf - the opened voxels are among them -, and
//   Dijkstra runs on.  A voxel that is never pushed has no lowered neighbour and satisfies its old equation.
// A fixed point that is >= the least one and has d[goal] = 0 is the least one: the bytes of field_dijkstra on mask_new.
// No old mask is given, so the counts speak of the voxels that were +inf and are finite now.  Returns true when the goal cell is
// inside the map and free in mask_new.
struct FieldReopenCounts { long long newly_reached = 0, reached_before = 0, free_voxels = 0, reached_voxels = 0; bool goal_opened = false; };
inline bool field_reopen(const uint32_t *mask_new, int X, int Y, int Z, int n_att, const int goal[3], double *d, FieldReopenCounts *counts) {
    const size_t nw = 4 * (size_t)((n_att + 127) / 128);
    const size_t n = (size_t)X * Y * Z, YZ = (size_t)Y * Z;
    const double inf = std::numeric_limits<double>::infinity();
    FieldReopenCounts C;
    const std::vector<unsigned char> fr = field_free_bytes(mask_new, nw, n, &C.free_voxels);
    for (size_t v = 0; v < n; v++) C.reached_before += d[v] < inf;
    size_t g = 0;
    const bool goal_in = field_goal_voxel(X, Y, Z, goal, &g);
    FieldHeap heap;
    if (goal_in && fr[g] && !(d[g] < inf)) { C.goal_opened = true; d[g] = 0.0; heap.push(0.0, g); }
    for (size_t v = 0; v < n; v++) {
        if (!fr[v] || d[v] < inf) continue;
        const int x = (int)(v / YZ), y = (int)((v / Z) % Y), z = (int)(v % Z);
        for (int i = -1; i < 2; i++)
            for (int j = -1; j < 2; j++)
                for (int k = -1; k < 2; k++) {
                    if (!(i | j | k)) continue;
                    const int ux = x + i, uy = y + j, uz = z + k;
                    if (ux < 0 || ux >= X || uy < 0 || uy >= Y || uz < 0 || uz >= Z) continue;
                    const size_t u = (size_t)ux * YZ + (size_t)uy * Z + (size_t)uz;
                    if (fr[u] && d[u] < inf) heap.push(d[u], u);
                }
    }
    field_relax_heap(mask_new, X, Y, Z, nw, heap, d);
    for (size_t v = 0; v < n; v++) C.reached_voxels += d[v] < inf;
    C.newly_reached = C.reached_voxels - C.reached_before;
    if (counts) *counts = C;
    return goal_in && fr[g] != 0;
}

// The field CARRIED through a shift of the map window by s (bits move both ways).  d: on entry the field of goal_old on
// the old table; mask_new: the table after the shift (new voxel v holds old voxel v + s, entering voxels free, the bands at the faces
// changed either way).  On return d is the field of goal' = goal_old - s on mask_new, the bytes of field_dijkstra.
//   d1 = d translated by msh_shift_grid's index rule, +inf where there is no source;
//   tau_left = the smallest finite old d of a voxel without a destination;
//   phase 1: field_repair with tau_left on mask_new restricted to the voxels with a finite d1 - an overlap voxel that was free and
//   unreached stays unreached on a subgraph of the old graph, so no old table is needed; its own tau covers the finite d1 whose new
//   word is 0;
//   phase 2: field_reopen on mask_new.
// A goal' outside the map: goal_left, everything +inf, false.  Returns true when the goal cell is inside the map and free in mask_new.
struct FieldShiftCounts { long long left_reached = 0; bool goal_left = false; FieldRepairCounts close; FieldReopenCounts open; };
inline bool field_shift(const uint32_t *mask_new, int X, int Y, int Z, int n_att, const int s[3], const int goal_old[3], double *d, FieldShiftCounts *counts) {
    const size_t nw = 4 * (size_t)((n_att + 127) / 128);
    const size_t n = (size_t)X * Y * Z;
    const double inf = std::numeric_limits<double>::infinity();
    const int32_t dims[3] = {X, Y, Z}, s32[3] = {s[0], s[1], s[2]};
    const int goal[3] = {goal_old[0] - s[0], goal_old[1] - s[1], goal_old[2] - s[2]};
    FieldShiftCounts C;
    size_t g;
    if (!field_goal_voxel(X, Y, Z, goal_old, &g) || !field_goal_voxel(X, Y, Z, goal, &g)) {
        for (size_t v = 0; v < n; v++) d[v] = inf;
        C.goal_left = true;
        C.close.tau = inf;
        if (counts) *counts = C;
        return false;
    }
    auto inside = [&](long long x, long long y, long long z) { return x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z; };
    double tau_left = inf;
    {
        size_t v = 0;
        for (int x = 0; x < X; x++)
            for (int y = 0; y < Y; y++)
                for (int z = 0; z < Z; z++, v++)
                    if (!inside((long long)x - s[0], (long long)y - s[1], (long long)z - s[2]) && d[v] < inf) { C.left_reached++; if (d[v] < tau_left) tau_left = d[v]; }
    }
    isdf::msh_shift_grid(d, sizeof(double), dims, s32, d);
    std::vector<uint32_t> mask1(mask_new, mask_new + n * nw);
    {
        size_t v = 0;
        for (int x = 0; x < X; x++)
            for (int y = 0; y < Y; y++)
                for (int z = 0; z < Z; z++, v++) {
                    if (!inside((long long)x + s[0], (long long)y + s[1], (long long)z + s[2])) d[v] = inf;       // (the grid's zero fill)
                    if (!(d[v] < inf)) for (size_t w = 0; w < nw; w++) mask1[nw * v + w] = 0u;
                }
    }
    (void)field_repair(mask1.data(), X, Y, Z, n_att, goal, d, &C.close, tau_left);
    const bool goal_free = field_reopen(mask_new, X, Y, Z, n_att, goal, d, &C.open);
    if (counts) *counts = C;
    return goal_free;
}

}  // namespace isdf_host
