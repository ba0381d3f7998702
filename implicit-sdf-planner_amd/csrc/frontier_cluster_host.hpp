// Host arithmetic of the frontier clusters (frontier_cluster.hip), free of HIP so that a plain C++ program can run it under
// a sanitizer.  The input set S is a bit grid in the known grid's layout (map_known_host.hpp); its voxels in ascending order are "the
// list", and pos(v) is a voxel's place in it.  The functions marked MU_HD are the ones the device kernels call: one statement of the
// voxel's coordinates, of the neighbours a connectivity has, of pos() and of the representative's key for both sides.  The host form's
// component search is a plain sequential union-find over list positions.
#pragma once
#include "map_known_host.hpp"
#include <vector>

namespace isdf {

constexpr int FC_ROW = 16;              // int64 words per cluster row: label, size, lo xyz, hi xyz, sum xyz, rep_voxel, rep_d2, first_pos, 0, 0
constexpr int FC_KEY_SHIFT = 36;        // the representative's key: (d2 << 36) | voxel
// a dimension is at most 4096: a voxel index is below 4096^3 = 2^36, d2 = |p - c|^2 at most 3 * 4095^2 < 2^26, so a key is below 2^62
static_assert(4096ll * 4096 * 4096 == (1ll << FC_KEY_SHIFT), "a voxel index fits the key's low 36 bits");
static_assert(3ll * 4095 * 4095 < (1ll << 26), "d2 fits 26 bits: the key fits 62");
constexpr unsigned long long FC_KEY_NONE = ~0ull;

struct FcGeom { int X, Y, Z; long long n_vox, n_words; };
inline FcGeom fc_geom(const int32_t dims[3]) {
    const long long n = mk_voxels(dims);
    return FcGeom{dims[0], dims[1], dims[2], n, mk_words(n)};
}

// connectivity 6 / 18 / 26 -> the largest number of non-zero entries an offset may have (1 / 2 / 3); anything else: 0
inline int fc_max_nonzero(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

MU_HD void fc_xyz(long long v, int ny, int nz, int &x, int &y, int &z) {
    const long long col = v / nz;
    z = (int)(v - col * nz);
    x = (int)(col / ny);
    y = (int)(col - (long long)x * ny);
}

// The LOWER neighbours: of the 26 offsets in {-1, 0, 1}^3 the 13 that come before (0, 0, 0) in the order of the voxel index - k = 0 .. 12
// is (k / 9 - 1, k / 3 % 3 - 1, k % 3 - 1) -, so every unordered pair of neighbours is met once, from its higher voxel.  False where the
// offset has more non-zero entries than the connectivity allows or the neighbour lies outside the grid; else *nv is its voxel index.
constexpr int FC_LOWER = 13;
MU_HD bool fc_lower_neighbour(int max_nonzero, int k, int x, int y, int z, const FcGeom &g, long long *nv) {
    const int dx = k / 9 - 1, dy = k / 3 % 3 - 1, dz = k % 3 - 1;
    if ((dx != 0) + (dy != 0) + (dz != 0) > max_nonzero) return false;
    const int px = x + dx, py = y + dy, pz = z + dz;
    if (px < 0 || py < 0 || py >= g.Y || pz < 0 || pz >= g.Z) return false;       // (dx <= 0: px < nx always)
    *nv = ((long long)px * g.Y + py) * g.Z + pz;
    return true;
}

MU_HD bool fc_in_set(const uint32_t *set_bits, long long v) { return (set_bits[v >> 5] >> (unsigned)(v & 31)) & 1u; }

// the place of voxel v of S in the ascending list: base[w] = the number of voxels of S in the words before w
template <typename Base> MU_HD long long fc_pos(const uint32_t *set_bits, const Base *base, long long v) {
    return (long long)base[v >> 5] + mk_popc(set_bits[v >> 5] & ((1u << (unsigned)(v & 31)) - 1u));
}

MU_HD long long fc_d2(int x, int y, int z, int cx, int cy, int cz) {
    const long long a = x - cx, b = y - cy, c = z - cz;
    return a * a + b * b + c * c;
}
MU_HD unsigned long long fc_key(long long d2, long long voxel) { return ((unsigned long long)d2 << FC_KEY_SHIFT) | (unsigned long long)voxel; }
MU_HD long long fc_key_voxel(unsigned long long key) { return (long long)(key & ((1ull << FC_KEY_SHIFT) - 1ull)); }
MU_HD long long fc_key_d2(unsigned long long key) { return (long long)(key >> FC_KEY_SHIFT); }

// the bits of the last word beyond the last voxel must be 0
inline bool fc_tail_dirty(const uint32_t *set_bits, const FcGeom &g) {
    const unsigned r = (unsigned)(g.n_vox & 31);
    return r != 0 && (set_bits[g.n_words - 1] >> r) != 0u;
}

struct FcCounts { long long n_voxels, n_clusters, n_rows, n_voxels_dropped, largest_size, largest_label; };

// The host form.  Returns 0, or 1 where a non-null output is too small - the counts are filled either way and the outputs are written
// only by a call that returns 0.  S's tail bits are clean (the caller has checked).
inline int fc_clusters_host(const uint32_t *set_bits, const FcGeom &g, int max_nonzero, long long min_size, int64_t *vox_out, int32_t *labels_out, long long vox_capacity,
                            int64_t *rows_out, long long row_capacity, FcCounts &N) {
    std::vector<long long> base((size_t)g.n_words);
    long long n = 0;
    for (long long w = 0; w < g.n_words; w++) { base[(size_t)w] = n; n += mk_popc(set_bits[w]); }
    std::vector<long long> vox((size_t)n), parent((size_t)n);
    {
        long long at = 0;
        for (long long w = 0; w < g.n_words; w++)
            for (uint32_t f = set_bits[w]; f; f &= f - 1) vox[(size_t)at++] = 32 * w + mk_lowest(f);
    }
    auto find = [&](long long i) {
        while (parent[(size_t)i] != i) {
            parent[(size_t)i] = parent[(size_t)parent[(size_t)i]];      // path halving
            i = parent[(size_t)i];
        }
        return i;
    };
    for (long long i = 0; i < n; i++) parent[(size_t)i] = i;
    for (long long i = 0; i < n; i++) {
        int x, y, z;
        fc_xyz(vox[(size_t)i], g.Y, g.Z, x, y, z);
        for (int k = 0; k < FC_LOWER; k++) {
            long long nv;
            if (!fc_lower_neighbour(max_nonzero, k, x, y, z, g, &nv) || !fc_in_set(set_bits, nv)) continue;
            const long long a = find(i), b = find(fc_pos(set_bits, base.data(), nv));
            if (a != b) parent[(size_t)(a > b ? a : b)] = a > b ? b : a;        // the lower position stays the root
        }
    }
    // number the roots in ascending position (= ascending label); cnum of a position: its cluster's number
    std::vector<long long> cnum((size_t)n), first;
    for (long long i = 0; i < n; i++)
        if (find(i) == i) { cnum[(size_t)i] = (long long)first.size(); first.push_back(i); }
    const long long nc = (long long)first.size();
    std::vector<long long> acc((size_t)nc * FC_ROW, 0);
    for (long long c = 0; c < nc; c++) {
        long long *r = &acc[(size_t)c * FC_ROW];
        r[0] = vox[(size_t)first[(size_t)c]]; r[13] = first[(size_t)c];
        r[2] = r[3] = r[4] = 0x7FFFFFFF; r[5] = r[6] = r[7] = -1;
    }
    for (long long i = 0; i < n; i++) {
        const long long c = cnum[(size_t)find(i)];
        cnum[(size_t)i] = c;                                   // (i's root has a lower position: its number is read before it is overwritten)
        long long *r = &acc[(size_t)c * FC_ROW];
        int p[3];
        fc_xyz(vox[(size_t)i], g.Y, g.Z, p[0], p[1], p[2]);
        r[1]++;
        for (int a = 0; a < 3; a++) {
            if (p[a] < r[2 + a]) r[2 + a] = p[a];
            if (p[a] > r[5 + a]) r[5 + a] = p[a];
            r[8 + a] += p[a];
        }
    }
    std::vector<unsigned long long> key((size_t)nc, FC_KEY_NONE);
    for (long long i = 0; i < n; i++) {
        const long long c = cnum[(size_t)i];
        const long long *r = &acc[(size_t)c * FC_ROW];
        int x, y, z;
        fc_xyz(vox[(size_t)i], g.Y, g.Z, x, y, z);
        const unsigned long long q = fc_key(fc_d2(x, y, z, (int)(r[8] / r[1]), (int)(r[9] / r[1]), (int)(r[10] / r[1])), vox[(size_t)i]);
        if (q < key[(size_t)c]) key[(size_t)c] = q;
    }
    std::vector<long long> row_of((size_t)nc);
    N = FcCounts{n, nc, 0, 0, 0, -1};
    for (long long c = 0; c < nc; c++) {
        long long *r = &acc[(size_t)c * FC_ROW];
        r[11] = fc_key_voxel(key[(size_t)c]); r[12] = fc_key_d2(key[(size_t)c]);
        if (r[1] > N.largest_size) { N.largest_size = r[1]; N.largest_label = r[0]; }
        if (r[1] >= min_size) row_of[(size_t)c] = N.n_rows++;
        else { row_of[(size_t)c] = -1; N.n_voxels_dropped += r[1]; }
    }
    if (((vox_out || labels_out) && vox_capacity < n) || (rows_out && row_capacity < N.n_rows)) return 1;
    for (long long i = 0; i < n; i++) {
        if (vox_out) vox_out[i] = vox[(size_t)i];
        if (labels_out) labels_out[i] = (int32_t)row_of[(size_t)cnum[(size_t)i]];
    }
    if (rows_out)
        for (long long c = 0; c < nc; c++)
            if (row_of[(size_t)c] >= 0) std::memcpy(rows_out + row_of[(size_t)c] * FC_ROW, &acc[(size_t)c * FC_ROW], FC_ROW * sizeof(int64_t));
    return 0;
}

}  // namespace isdf
