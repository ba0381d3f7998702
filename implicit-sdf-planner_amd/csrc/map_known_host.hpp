// Host arithmetic of the known grid (map_known.hip), free of HIP so that a plain C++ program can run it under a sanitizer.
// One bit per voxel: voxel a = (x * ny + y) * nz + z is bit a & 31 of word a >> 5, ceil(nx ny nz / 32) words, the bits beyond the last
// voxel always 0.  Columns are nz bits long and nz is anything in [1, 4096], so a column starts at any bit and a dword may cover
// several: everything here treats the grid as ONE stream of bits and a neighbour or a translation as a constant offset in it.
// The functions marked MU_HD are the ones the device kernels call: one statement of the arithmetic for both sides.
#pragma once
#include "map_update_host.hpp"

namespace isdf {

inline bool mk_dims_bad(const int32_t dims[3]) {
    if (!dims) return true;
    for (int a = 0; a < 3; a++) if (dims[a] < 1 || dims[a] > 4096) return true;
    return false;
}
inline long long mk_voxels(const int32_t dims[3]) { return (long long)dims[0] * dims[1] * dims[2]; }
inline long long mk_words(long long n_vox) { return (n_vox + 31) >> 5; }

MU_HD int mk_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// The 32 bits of the stream that start at bit offset b (signed): two dword loads and a funnel shift.  Where the stream does not exist
// - before bit 0, from word n_words on - it reads zeros.
MU_HD uint32_t mk_bits_at(const uint32_t *bits, long long n_words, long long b) {
    if (b <= -32 || b >= 32 * n_words) return 0u;
    const long long w = b >= 0 ? b >> 5 : -1;                 // floor(b / 32): b > -32 here
    const unsigned r = (unsigned)(b - 32 * w);                // 0 .. 31
    const uint64_t lo = w >= 0 ? bits[w] : 0u;
    const uint64_t hi = w + 1 < n_words ? bits[w + 1] : 0u;
    return (uint32_t)(((hi << 32) | lo) >> r);
}

// bits [first, last] of a dword, 0 <= first <= last <= 31
MU_HD uint32_t mk_run(int first, int last) { return (0xFFFFFFFFu << (unsigned)first) & (0xFFFFFFFFu >> (31u - (unsigned)last)); }

// The bits of dword w whose voxel lies in the inclusive index box [lo, hi] (and in the grid: n_vox = nx ny nz ends the stream).  Built
// per column segment the dword covers: one division for the first column, then y and x are carried.
MU_HD uint32_t mk_box_mask(long long w, int ny, int nz, long long n_vox, const int lo[3], const int hi[3]) {
    long long a = 32 * w;
    const long long end = a + 32 < n_vox ? a + 32 : n_vox;
    if (a >= end) return 0u;
    const long long col = a / nz;
    int z = (int)(a - col * nz), x = (int)(col / ny), y = (int)(col - (long long)x * ny);
    uint32_t m = 0u;
    while (a < end) {
        const long long seg_end = a + (nz - z) < end ? a + (nz - z) : end;      // this column's bits of the dword: [a, seg_end)
        if (x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1]) {
            const int z_last = z + (int)(seg_end - a) - 1;
            const int zs = z > lo[2] ? z : lo[2], ze = z_last < hi[2] ? z_last : hi[2];
            if (zs <= ze) m |= mk_run((int)(a - 32 * w) + (zs - z), (int)(a - 32 * w) + (ze - z));
        }
        a = seg_end; z = 0;
        if (++y == ny) { y = 0; ++x; }
    }
    return m;
}

// ---- the shift: K'[v] = K[v + s] where v + s lies in the old grid, else 0
struct MkShift { long long delta; int lo[3], hi[3]; int empty; };       // the stream offset; the destination voxels that have a source
inline MkShift mk_shift_plan(const int32_t dims[3], const int32_t s[3]) {
    MkShift P{};
    P.delta = ((long long)s[0] * dims[1] + s[1]) * dims[2] + s[2];
    for (int a = 0; a < 3; a++) {
        const long long l = s[a] < 0 ? -(long long)s[a] : 0, h = (long long)dims[a] - 1 - (s[a] > 0 ? (long long)s[a] : 0);
        if (l > h) P.empty = 1;
        P.lo[a] = (int)(l > 4096 ? 4096 : l); P.hi[a] = (int)(h < -1 ? -1 : h);
    }
    return P;
}
MU_HD uint32_t mk_shift_word(const uint32_t *bits, long long n_words, long long w, int ny, int nz, long long n_vox, const MkShift &P) {
    if (P.empty) return 0u;
    const uint32_t m = mk_box_mask(w, ny, nz, n_vox, P.lo, P.hi);
    return m ? mk_bits_at(bits, n_words, 32 * w + P.delta) & m : 0u;
}

// ---- the frontier: K = 1, occupancy byte 0, some 6-neighbour inside the grid with K = 0
// the voxels of four occupancy bytes that are free, as bits 0 .. 3
MU_HD uint32_t mk_free4(uint32_t v) {
    v |= v >> 4; v |= v >> 2; v |= v >> 1;                    // bit 0 of every byte: the OR of the byte
    v = ~v & 0x01010101u;
    return (v * 0x01020408u) >> 24;                           // bits 0, 8, 16, 24 -> 24, 25, 26, 27, no two partial products meet
}
// the six masks of dword w: bit set where the voxel's neighbour at -z, +z, -y, +y, -x, +x lies inside the grid - one walk over the
// column segments for all six
MU_HD void mk_edge_masks(long long w, int nx, int ny, int nz, long long n_vox, uint32_t m[6]) {
    for (int q = 0; q < 6; q++) m[q] = 0u;
    long long a = 32 * w;
    const long long end = a + 32 < n_vox ? a + 32 : n_vox;
    if (a >= end) return;
    const long long col = a / nz;
    int z = (int)(a - col * nz), x = (int)(col / ny), y = (int)(col - (long long)x * ny);
    while (a < end) {
        const long long seg_end = a + (nz - z) < end ? a + (nz - z) : end;
        const int b0 = (int)(a - 32 * w), b1 = b0 + (int)(seg_end - a) - 1, z_last = z + (b1 - b0);
        const uint32_t seg = mk_run(b0, b1);
        if (z > 0) m[0] |= seg; else if (b1 > b0) m[0] |= mk_run(b0 + 1, b1);
        if (z_last < nz - 1) m[1] |= seg; else if (b1 > b0) m[1] |= mk_run(b0, b1 - 1);
        if (y > 0) m[2] |= seg;
        if (y < ny - 1) m[3] |= seg;
        if (x > 0) m[4] |= seg;
        if (x < nx - 1) m[5] |= seg;
        a = seg_end; z = 0;
        if (++y == ny) { y = 0; ++x; }
    }
}
// free: bit set where the voxel's occupancy byte is 0 (bits beyond the grid: anything)
MU_HD uint32_t mk_frontier_word(const uint32_t *bits, long long n_words, long long w, int nx, int ny, int nz, long long n_vox, uint32_t free_mask) {
    const uint32_t k = bits[w] & free_mask;
    if (!k) return 0u;
    uint32_t m[6];
    mk_edge_masks(w, nx, ny, nz, n_vox, m);
    const long long b = 32 * w, sy = nz, sx = (long long)ny * nz;
    const uint32_t unknown = (~mk_bits_at(bits, n_words, b - 1) & m[0]) | (~mk_bits_at(bits, n_words, b + 1) & m[1]) |
                             (~mk_bits_at(bits, n_words, b - sy) & m[2]) | (~mk_bits_at(bits, n_words, b + sy) & m[3]) |
                             (~mk_bits_at(bits, n_words, b - sx) & m[4]) | (~mk_bits_at(bits, n_words, b + sx) & m[5]);
    return k & unknown;
}

MU_HD int mk_lowest(uint32_t v) {             // index of the lowest set bit, v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)v) - 1;
#else
    return __builtin_ctz(v);
#endif
}
MU_HD int mk_highest(uint32_t v) {            // index of the highest set bit, v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int)v);
#else
    return 31 - __builtin_clz(v);
#endif
}
// the index box [lo, hi] widened by the voxels whose bits are set in v, dword w of the grid: per column segment, not per bit
MU_HD void mk_word_box(long long w, uint32_t v, int ny, int nz, long long n_vox, int lo[3], int hi[3]) {
    long long a = 32 * w;
    const long long end = a + 32 < n_vox ? a + 32 : n_vox;
    if (!v || a >= end) return;
    const long long col = a / nz;
    int z = (int)(a - col * nz), x = (int)(col / ny), y = (int)(col - (long long)x * ny);
    while (a < end) {
        const long long seg_end = a + (nz - z) < end ? a + (nz - z) : end;
        const int b0 = (int)(a - 32 * w), b1 = b0 + (int)(seg_end - a) - 1;
        const uint32_t sb = v & mk_run(b0, b1);
        if (sb) {
            const int zf = z + mk_lowest(sb) - b0, zl = z + mk_highest(sb) - b0;
            if (x < lo[0]) lo[0] = x;
            if (x > hi[0]) hi[0] = x;
            if (y < lo[1]) lo[1] = y;
            if (y > hi[1]) hi[1] = y;
            if (zf < lo[2]) lo[2] = zf;
            if (zl > hi[2]) hi[2] = zl;
        }
        a = seg_end; z = 0;
        if (++y == ny) { y = 0; ++x; }
    }
}

// ---- the host forms' loops
inline bool mk_box_bad(const int32_t dims[3], const int32_t box[6]) {
    for (int a = 0; a < 3; a++) if (box[a] < 0 || box[3 + a] >= dims[a] || box[a] > box[3 + a]) return true;
    return false;
}

// K |= V, V = free byte != 0 or hit multiplicity > 0; returns the bits that went from 0 to 1
inline long long mk_merge_host(uint32_t *bits, const int32_t dims[3], const uint8_t *free_bytes, const uint32_t *hits) {
    const long long n = mk_voxels(dims);
    long long newly = 0;
    for (long long a = 0; a < n; a++) {
        if (!((free_bytes && free_bytes[a]) || (hits && hits[a]))) continue;
        const uint32_t b = 1u << (unsigned)(a & 31);
        if (!(bits[a >> 5] & b)) { bits[a >> 5] |= b; newly++; }
    }
    return newly;
}

inline void mk_shift_host(const uint32_t *in, const int32_t dims[3], const int32_t s[3], uint32_t *out) {
    const long long n = mk_voxels(dims), nw = mk_words(n);
    const MkShift P = mk_shift_plan(dims, s);
    for (long long w = 0; w < nw; w++) out[w] = mk_shift_word(in, nw, w, dims[1], dims[2], n, P);
}

// sets or clears the box; returns the bits that went from 0 to 1
inline long long mk_fill_host(uint32_t *bits, const int32_t dims[3], const int32_t box[6], int value) {
    const long long n = mk_voxels(dims);
    const long long w0 = (((long long)box[0] * dims[1] + box[1]) * dims[2] + box[2]) >> 5, w1 = (((long long)box[3] * dims[1] + box[4]) * dims[2] + box[5]) >> 5;
    long long newly = 0;
    for (long long w = w0; w <= w1; w++) {
        const uint32_t m = mk_box_mask(w, dims[1], dims[2], n, box, box + 3), old = bits[w], now = value ? old | m : old & ~m;
        bits[w] = now;
        newly += mk_popc(now & ~old);
    }
    return newly;
}

// the free mask of dword w from occupancy bytes, read one by one (n_vox bytes exist)
inline uint32_t mk_free_mask_host(const uint8_t *occ, long long w, long long n_vox) {
    uint32_t f = 0u;
    for (int b = 0; b < 32 && 32 * w + b < n_vox; b++) if (occ[32 * w + b] == 0) f |= 1u << b;
    return f;
}

// bits_out (nullable): the frontier's bit grid; vox_out (nullable): its voxels ascending, written only when capacity >= their number.
// Returns that number; lo / hi: their index box (lo > hi: none).
inline long long mk_frontier_host(const uint32_t *bits, const uint8_t *occ, const int32_t dims[3], uint32_t *bits_out, int64_t *vox_out, long long capacity,
                                  int lo[3], int hi[3]) {
    const long long n = mk_voxels(dims), nw = mk_words(n);
    for (int a = 0; a < 3; a++) { lo[a] = 0x7FFFFFFF; hi[a] = -1; }
    long long count = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && (!vox_out || capacity < count)) break;
        long long at = 0;
        for (long long w = 0; w < nw; w++) {
            uint32_t f = mk_frontier_word(bits, nw, w, dims[0], dims[1], dims[2], n, mk_free_mask_host(occ, w, n));
            if (pass == 0) {
                if (bits_out) bits_out[w] = f;
                count += mk_popc(f);
            }
            if (pass == 0) mk_word_box(w, f, dims[1], dims[2], n, lo, hi);
            else for (; f; f &= f - 1) vox_out[at++] = 32 * w + mk_lowest(f);
        }
    }
    if (count == 0) for (int a = 0; a < 3; a++) { lo[a] = 0; hi[a] = -1; }
    return count;
}

}  // namespace isdf
