// Host arithmetic of the eroded known grid (known_erode.hip), free of HIP so that a plain C++ program can run it under a
// sanitizer.  K is map_known_host.hpp's bit stream.  For r >= 0 and border in {0, 1}
//   E[v] = 1  iff  for every u with max(|ux - vx|, |uy - vy|, |uz - vz|) <= r:  (u inside the grid and K[u] = 1) or (u outside and border = 1)
// in K's layout, tail bits 0: the voxels round which the whole cube of 2 r + 1 voxels a side has been observed.
// The cube is a product of three intervals, so E is three one-axis passes, z then y then x: a voxel survives a pass when its 2 r + 1
// neighbours along the axis do, a neighbour outside the grid counting as `border`.  (A position outside the grid in x or y has all its
// z-neighbours outside, so the z pass leaves `border` there - the constant the y pass assumes; likewise for x.)  On the stream a
// neighbour along z, y, x is the constant offset 1, nz, ny nz: one pass over one dword is 2 r + 1 reads of mk_bits_at, each under the
// mask of the dword's voxels whose neighbour at that offset lies inside the grid.  Offsets of nz or more dims along the axis have an
// empty mask, so a radius larger than the grid costs reads, not correctness.
// ke_pass_word is the one the device kernel calls: one statement of the arithmetic for both sides.
#pragma once
#include "map_known_host.hpp"

namespace isdf {

constexpr int KE_MAX_RADIUS = 64;

// the voxel of a dword's bit 0, found with the pass's only divisions
struct KeFirst { int x, y, z; };
MU_HD KeFirst ke_first(long long w, int ny, int nz) {
    const long long a = 32 * w, col = a / nz;
    KeFirst F;
    F.z = (int)(a - col * nz); F.x = (int)(col / ny); F.y = (int)(col - (long long)F.x * ny);
    return F;
}

// The bits of dword w (bit 0 = voxel F, `count` voxels of it exist) whose coordinate along `axis` (0 x, 1 y, 2 z) lies in [lo, hi]:
// mk_box_mask for a slab, walked per column segment as mk_edge_masks walks - a column starts at any bit and nz need not divide 32.
MU_HD uint32_t ke_slab_mask(KeFirst F, int count, int ny, int nz, int axis, int lo, int hi) {
    if (lo > hi) return 0u;
    uint32_t m = 0u;
    int b = 0, x = F.x, y = F.y, z = F.z;
    while (b < count) {
        const int seg = nz - z < count - b ? nz - z : count - b;        // this column's bits of the dword: [b, b + seg)
        if (axis == 2) {
            const int zs = z > lo ? z : lo, ze = z + seg - 1 < hi ? z + seg - 1 : hi;
            if (zs <= ze) m |= mk_run(b + (zs - z), b + (ze - z));
        } else {
            const int q = axis == 0 ? x : y;
            if (q >= lo && q <= hi) m |= mk_run(b, b + seg - 1);
        }
        b += seg; z = 0;
        if (++y == ny) { y = 0; ++x; }
    }
    return m;
}

// dword w of one pass along `axis` over the stream `in` (tail bits clean or not: only voxels of the grid are read as such)
MU_HD uint32_t ke_pass_word(const uint32_t *in, long long n_words, long long w, int nx, int ny, int nz, long long n_vox, int axis, int r, int border) {
    const long long rest = n_vox - 32 * w;
    if (rest <= 0) return 0u;
    const int count = rest < 32 ? (int)rest : 32;
    const uint32_t valid = mk_run(0, count - 1);
    if (r == 0) return in[w] & valid;
    const KeFirst F = ke_first(w, ny, nz);
    const int n = axis == 0 ? nx : axis == 1 ? ny : nz;
    const long long stride = axis == 0 ? (long long)ny * nz : axis == 1 ? nz : 1;
    uint32_t out = valid;
    for (int k = -r; k <= r && out; k++) {
        // the voxels whose neighbour at +k along the axis lies inside: coordinate in [max(0, -k), min(n, n - k) - 1]
        const uint32_t inside = ke_slab_mask(F, count, ny, nz, axis, k < 0 ? -k : 0, (k > 0 ? n - k : n) - 1);
        const uint32_t v = inside ? mk_bits_at(in, n_words, 32 * w + k * stride) : 0u;
        out &= border ? (v | ~inside) : (v & inside);
    }
    return out;
}

// ---- the host form's loop: bits_out != bits, both ceil(nx ny nz / 32) words; two scratch grids of that size
inline void ke_erode_host(const uint32_t *bits, const int32_t dims[3], int r, int border, uint32_t *bits_out, uint32_t *scratch) {
    const long long n = mk_voxels(dims), nw = mk_words(n);
    const uint32_t *src = bits;
    for (int pass = 0; pass < 3; pass++) {          // z: bits -> out, y: out -> scratch, x: scratch -> out
        uint32_t *dst = pass == 1 ? scratch : bits_out;
        for (long long w = 0; w < nw; w++) dst[w] = ke_pass_word(src, nw, w, dims[0], dims[1], dims[2], n, 2 - pass, r, border);
        src = dst;
    }
}

}  // namespace isdf
