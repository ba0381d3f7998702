// Swept-volume SDF field and its surface mesh on the device (isdf_swept_sdf*, isdf_swept_mesh_*): the other half of the
// reference's SweptVolumeManager::calculateSwept (sw_manager.hpp:225-237 -> sw_calculate::calculation / getmesh).
//
// Field: the V1 step's own launches (swept_sweep.hip: prepare, scan, descent) on scratch of their own, in chunks of FIELD_CHUNK
// points, followed by swept_field_reduce_kernel, which folds a point's interval slots into (value, t*) - getSDFofSweptVolume
// (sw_manager.hpp:710-747) per point.  PLANNER is the query exactly as the collision term binds it; CLOSED adds the coarse sample
// t = duration and keeps a run still in range there (the scan's CLOSED instantiation).
//
// Mesh: the field on a lattice of spacing eps, then marching tetrahedra on the Kuhn (Freudenthal) split - six tetrahedra per cell
// around its main diagonal, the same in every cell, so neighbouring cells agree on every face (crack-free, no ambiguity tables).
//   narrow band  the field on every B-th node first; a coarse cell is refined when its corners change sign about iso, or when none
//                of them lies farther than L * sqrt(3) * B * eps from it (a corner that does proves the whole cell's side for an
//                L-Lipschitz field; a corner that reads 10, no interval, counts as 2 safety_hor + 0.1); the fine nodes of the refined cells are flagged (a gather per node: each once), compacted and
//                evaluated in one batch.
//   extraction   cells whose eight corners are known: triangles per cell (count, exclusive scan, emit); a vertex per sign-changing
//                lattice edge (7 per node: +x +y +z +xy +xz +yz +xyz) that lies in such a cell, numbered by ascending global edge
//                id (node * 7 + dir) through a per-node count and scan.  No atomics decide any order: the output is the same bytes
//                on every run, and the narrow-band mesh is the dense one.
// The reference continues its field along a flood fill (descents of +-0.1 s seeded by a neighbour's t*, sw_manager.hpp:1173-1193):
// its values depend on the flood order and are deliberately not reproduced - every node here is an independent query.
#include "swept_field.hpp"
#include "dev_reduce.hpp"
#include "dev_scan.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

constexpr long long MESH_MAX_NODES = 1ll << 27;           // fine lattice nodes of one mesh build (~20 B of scratch per node)

void free_mesh_result(SweptMeshState *s) {
    s->d_V.release(); s->d_F.release();
    s->nV = s->nF = 0; s->have_mesh = false;
}

int fail(isdf_ctx *c, int code, const char *msg) { return isdf_fail(c, code, msg); }

}  // namespace

int swept_field_scratch(isdf_ctx *c, SweptMeshState **out) {
    ISDF_TRY(c->swm.make(c, out));
    SweptMeshState *s = *out;
    if (!s->d_stats) HIPCHK(c, s->d_stats.alloc(8));
    ISDF_TRY(s->h_overflow.reserve(c, 1));
    return s->field.reserve(c, (size_t)FIELD_CHUNK, false);
}

// host-side checks shared by both field entry points and the mesh build
int swept_check_traj(isdf_ctx *c, int N, const double *T) {
    double td = 0.0;
    for (int i = 0; i < N; i++) {
        if (!(T[i] > 0.0) || !std::isfinite(T[i])) return fail(c, ISDF_ERR_INVALID_ARG, "piece durations must be finite and > 0");
        td += T[i];
    }
    if (!(td < MAX_DURATION)) return fail(c, ISDF_ERR_INVALID_ARG, "swept-volume field: trajectory of 300 s or longer (the reference's duration rule)");
    return ISDF_OK;
}
int swept_check_ctx(isdf_ctx *c) {
    if (!c->peers.empty() || c->is_peer || c->rccl_comm) return fail(c, ISDF_ERR_UNSUPPORTED, "swept-volume field on a multi-device ctx");
    if (!c->have_shape) return fail(c, ISDF_ERR_STATE, "shape not set");
    return ISDF_OK;
}

// the field launches' parameters on the query's own scratch
static SweptParams field_params(isdf_ctx *c, SweptMeshState *s, int N, const double *d_T, const double *d_coeffs) {
    SweptParams P{};
    P.shape = c->shape;
    isdf_fill_flat(c->cfg, P.flat);
    P.N = N;
    P.safety_hor = c->cfg.safety_hor; P.weight_p = c->cfg.weight_p;
    P.T = d_T; P.coeffs = d_coeffs;
    s->field.bind(P);
    P.stats = s->d_stats;
    return P;
}

// the coarse table of a trajectory alone (prepare kernel; asynchronous on `st`): n_coarse and the component-major poses in the
// query's scratch, the doubles swept_field_run builds again for the same trajectory and mode
int swept_field_coarse_table(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, int mode, hipStream_t st) {
    SweptMeshState *s;
    ISDF_TRY(swept_field_scratch(c, &s));
    SweptParams P = field_params(c, s, N, d_T, d_coeffs);
    P.points = nullptr; P.point_begin = 0; P.point_end = 0; P.M = 0;
    launch_swept_prepare(P, st, mode == ISDF_SWEPT_FIELD_CLOSED);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

// the field's launches at n points (device arrays) on `st`; the overflow word stays on the device (d_stats[4])
int swept_field_launch(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const double *d_xyz, long long n, int mode,
                       double *d_value, double *d_tstar, hipStream_t st) {
    SweptMeshState *s;
    ISDF_TRY(swept_field_scratch(c, &s));
    if (n <= 0) return ISDF_OK;
    const bool closed = mode == ISDF_SWEPT_FIELD_CLOSED;
    SweptParams P = field_params(c, s, N, d_T, d_coeffs);
    HIPCHK(c, hipMemsetAsync(s->d_stats, 0, 8 * sizeof(unsigned long long), st));
    // the coarse table once (it depends on the trajectory alone): the prepare kernel reads no point
    P.points = d_xyz; P.point_begin = 0; P.point_end = 0; P.M = 0;
    launch_swept_prepare(P, st, closed);
    for (long long b = 0; b < n; b += FIELD_CHUNK) {
        const int m = (int)std::min<long long>(FIELD_CHUNK, n - b);
        P.points = d_xyz + 3 * b; P.M = m; P.point_begin = 0; P.point_end = m;
        if (b > 0) HIPCHK(c, hipMemsetAsync(s->field.words, 0, 2 * sizeof(unsigned), st));    // the descent's task counters (the prepare kernel zeroed the first chunk's)
        launch_swept_sweep(P, st, nullptr, nullptr, closed);
        launch_swept_field_reduce(P, d_value + b, d_tstar ? d_tstar + b : nullptr, st);
    }
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

// the field at n points (device arrays), synchronous on `st` at the end (the overflow word is read back)
int swept_field_run(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const double *d_xyz, long long n, int mode,
                    double *d_value, double *d_tstar, hipStream_t st) {
    ISDF_TRY(swept_field_launch(c, N, d_T, d_coeffs, d_xyz, n, mode, d_value, d_tstar, st));
    if (n <= 0) return ISDF_OK;
    SweptMeshState *s = c->swm.get();
    HIPCHK(c, hipMemcpyAsync(s->h_overflow, s->d_stats + 4, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*s->h_overflow.get()) return fail(c, ISDF_ERR_OVERFLOW, "swept-volume field: a point has more than 32 in-range intervals (results not valid)");
    return ISDF_OK;
}

namespace {

// ---- mesh kernels ---------------------------------------------------------------------------------------------------
struct Lattice {
    int nx, ny, nz;          // fine nodes per axis; node id = (i * ny + j) * nz + k (z fastest, GridMap3D::toAddr)
    double ox, oy, oz, eps;
};
__device__ __forceinline__ void node_ijk(const Lattice &L, long long id, int &i, int &j, int &k) {
    k = (int)(id % L.nz); id /= L.nz; j = (int)(id % L.ny); i = (int)(id / L.ny);
}
__device__ __forceinline__ long long node_id(const Lattice &L, int i, int j, int k) { return ((long long)i * L.ny + j) * L.nz + k; }

// xyz of the nodes [first, first + n) of a list (ids) or of the lattice itself (ids == null): origin + i * eps, the product and the
// sum each rounded on its own (no contraction into an fma)
__global__ void node_xyz_kernel(Lattice L, const int *ids, long long first, int n, double *xyz) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long long id = ids ? (long long)ids[first + t] : first + t;
    int i, j, k;
    node_ijk(L, id, i, j, k);
    xyz[3 * t] = L.ox + (double)i * L.eps; xyz[3 * t + 1] = L.oy + (double)j * L.eps; xyz[3 * t + 2] = L.oz + (double)k * L.eps;
}
__global__ void node_scatter_kernel(const int *ids, long long first, int n, const double *val, double *f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    f[ids ? (long long)ids[first + t] : first + t] = val[t];
}

// coarse lattice: every B-th fine node per axis, the last fine node always included (cell c of an axis spans [c B, min(c B + B, n - 1)])
struct Coarse { int B, cx, cy, cz; };
__device__ __forceinline__ int coarse_coord(int c, int B, int n) { return min(c * B, n - 1); }
__global__ void coarse_ids_kernel(Lattice L, Coarse Q, int *ids) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nc = (long long)Q.cx * Q.cy * Q.cz;
    if (t >= nc) return;
    const int ck = (int)(t % Q.cz), cj = (int)((t / Q.cz) % Q.cy), ci = (int)(t / ((long long)Q.cz * Q.cy));
    ids[t] = (int)node_id(L, coarse_coord(ci, Q.B, L.nx), coarse_coord(cj, Q.B, L.ny), coarse_coord(ck, Q.B, L.nz));
}
// refine[coarse cell] = its corners change sign about iso, or none of them lies farther than thr = L sqrt(3) B eps from it.  A corner
// c with |f(c) - iso| > thr proves the whole cell: every point of it is within the cell's diagonal of c, so an L-Lipschitz f keeps
// the side of iso that c is on.  A corner that found no qualifying interval reads the constant 10, which is no distance: all it
// proves is that the corner is not within the qualification radius unq = 2 safety_hor + 0.1, so it counts as the value unq.
__global__ void refine_kernel(Lattice L, Coarse Q, const double *f, double iso, double thr, double unq, unsigned char *refine) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ex = Q.cx - 1, ey = Q.cy - 1, ez = Q.cz - 1;
    if (t >= (long long)ex * ey * ez) return;
    const int ck = (int)(t % ez), cj = (int)((t / ez) % ey), ci = (int)(t / ((long long)ez * ey));
    bool any_in = false, any_out = false, far = false;
    for (int c = 0; c < 8; c++) {
        const double v = f[node_id(L, coarse_coord(ci + (c & 1), Q.B, L.nx), coarse_coord(cj + ((c >> 1) & 1), Q.B, L.ny),
                                   coarse_coord(ck + ((c >> 2) & 1), Q.B, L.nz))];
        if (v < iso) any_in = true; else any_out = true;
        if (!(fabs((v == 1e1 ? unq : v) - iso) <= thr)) far = true;
    }
    refine[t] = (any_in && any_out) || !far ? 1 : 0;
}
// per axis: the coarse cells whose span holds fine coordinate i ([lo, hi], one or two of them)
__device__ __forceinline__ void coarse_span(int i, int B, int n_cells, int &lo, int &hi) {
    hi = min(i / B, n_cells - 1);
    lo = (i % B == 0 && i > 0) ? min(i / B - 1, hi) : hi;
}
// flag[node] = a fine node (not on the coarse lattice) of a refined coarse cell
__global__ void flag_kernel(Lattice L, Coarse Q, const unsigned char *refine, unsigned char *flag) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)L.nx * L.ny * L.nz) return;
    int i, j, k;
    node_ijk(L, id, i, j, k);
    const bool coarse = (i % Q.B == 0 || i == L.nx - 1) && (j % Q.B == 0 || j == L.ny - 1) && (k % Q.B == 0 || k == L.nz - 1);
    unsigned char fl = 0;
    if (!coarse) {
        const int ex = Q.cx - 1, ey = Q.cy - 1, ez = Q.cz - 1;
        int i0, i1, j0, j1, k0, k1;
        coarse_span(i, Q.B, ex, i0, i1); coarse_span(j, Q.B, ey, j0, j1); coarse_span(k, Q.B, ez, k0, k1);
        for (int a = i0; a <= i1; a++)
            for (int b = j0; b <= j1; b++)
                for (int c = k0; c <= k1; c++) fl |= refine[((long long)a * ey + b) * ez + c];
    }
    flag[id] = fl;
}

// ---- marching tetrahedra on the Kuhn split --------------------------------------------------------------------------
// Cell corners are numbered by their offset bits (x | y << 1 | z << 2).  Tetrahedron p of a cell is the monotone path
// 0 -> e_a -> e_a + e_b -> 7 for the p-th permutation (a, b, c) of the axes; its orientation is the sign of the permutation.
// Every edge of it joins two corners one of which is a subset of the other: a lattice edge from the lower node in one of 7
// directions (offset bits 1..7 -> +x +y +xy +z +xz +yz +xyz, numbered 0 1 3 2 4 5 6 below).
__constant__ int c_perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__constant__ int c_perm_odd[6] = {0, 1, 1, 0, 0, 1};
__constant__ int c_dir_of_offset[8] = {-1, 0, 1, 3, 2, 4, 5, 6};    // offset bits -> direction 0..6 (x, y, z, xy, xz, yz, xyz)
__constant__ int c_offset_of_dir[7] = {1, 2, 4, 3, 5, 6, 7};

__device__ __forceinline__ int parity4(const int v[4]) {
    int inv = 0;
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++) inv += v[a] > v[b];
    return inv & 1;
}
// The triangles of one positively oriented tetrahedron (corners q[0..3], inside = value < iso): 0, 1 or 2 of them, each as three
// edges (pairs of cell corners).  One corner apart from the others (1 or 3 inside): the triangle on its three edges; two and two:
// the quad on the four edges between the pairs, split along (a, c) - (b, d).  The corner orderings are even permutations of the
// tetrahedron's, so the orientation rule is the same in every case: normals point from inside to outside, towards larger f.
__device__ __forceinline__ int tet_tris(const int q[4], const bool in[4], int e[2][3][2]) {
    const int n_in = (int)in[0] + (int)in[1] + (int)in[2] + (int)in[3];
    if (n_in == 0 || n_in == 4) return 0;
    if (n_in == 1 || n_in == 3) {
        const bool lone_in = n_in == 1;
        int k = 0;
        while (in[k] != lone_in) k++;
        int v[4] = {k, 0, 0, 0}, m = 1;
        for (int a = 0; a < 4; a++) if (a != k) v[m++] = a;
        if (parity4(v)) { const int t = v[2]; v[2] = v[3]; v[3] = t; }
        // lone inside: (ab, ac, ad) faces away from a; lone outside: (ab, ad, ac) faces towards it
        const int s1 = lone_in ? v[2] : v[3], s2 = lone_in ? v[3] : v[2];
        e[0][0][0] = q[v[0]]; e[0][0][1] = q[v[1]];
        e[0][1][0] = q[v[0]]; e[0][1][1] = q[s1];
        e[0][2][0] = q[v[0]]; e[0][2][1] = q[s2];
        return 1;
    }
    int v[4], m = 0;
    for (int a = 0; a < 4; a++) if (in[a]) v[m++] = a;
    for (int a = 0; a < 4; a++) if (!in[a]) v[m++] = a;
    if (parity4(v)) { const int t = v[2]; v[2] = v[3]; v[3] = t; }
    const int a = q[v[0]], b = q[v[1]], cc = q[v[2]], d = q[v[3]];
    e[0][0][0] = a; e[0][0][1] = cc; e[0][1][0] = a; e[0][1][1] = d;  e[0][2][0] = b; e[0][2][1] = d;
    e[1][0][0] = a; e[1][0][1] = cc; e[1][1][0] = b; e[1][1][1] = d;  e[1][2][0] = b; e[1][2][1] = cc;
    return 2;
}
// tetrahedron p of a cell: its corners in positive orientation
__device__ __forceinline__ void kuhn_tet(int p, int q[4]) {
    const int a = c_perm[p][0], b = c_perm[p][1];
    q[0] = 0; q[1] = 1 << a; q[2] = (1 << a) | (1 << b); q[3] = 7;
    if (c_perm_odd[p]) { const int t = q[1]; q[1] = q[2]; q[2] = t; }
}

__device__ __forceinline__ bool cell_values(const Lattice &L, const double *f, int i, int j, int k, double v[8]) {
    bool ok = true;
    for (int c = 0; c < 8; c++) {
        v[c] = f[node_id(L, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))];
        ok = ok && !(v[c] != v[c]);
    }
    return ok;
}

// per cell: known (all eight corners evaluated) and its number of triangles; stats[0] += known cells, stats[1] += triangles
__global__ void cell_count_kernel(Lattice L, const double *f, double iso, unsigned char *known, int *tcount, unsigned long long *stats) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ex = L.nx - 1, ey = L.ny - 1, ez = L.nz - 1;
    const long long n_cells = (long long)ex * ey * ez;
    unsigned long long k_sum = 0, t_sum = 0;
    if (t < n_cells) {
        const int k = (int)(t % ez), j = (int)((t / ez) % ey), i = (int)(t / ((long long)ez * ey));
        double v[8];
        const bool ok = cell_values(L, f, i, j, k, v);
        int n = 0;
        if (ok) {
            for (int p = 0; p < 6; p++) {
                int q[4], e[2][3][2];
                kuhn_tet(p, q);
                const bool in[4] = {v[q[0]] < iso, v[q[1]] < iso, v[q[2]] < iso, v[q[3]] < iso};
                n += tet_tris(q, in, e);
            }
        }
        known[t] = ok ? 1 : 0;
        tcount[t] = n;
        k_sum = ok; t_sum = (unsigned long long)n;
    }
    k_sum = wave_sum(k_sum); t_sum = wave_sum(t_sum);
    if ((threadIdx.x & 63) == 0) { if (k_sum) atomicAdd(&stats[0], k_sum); if (t_sum) atomicAdd(&stats[1], t_sum); }
}

// per node: bit d of mask = a vertex on edge (node, d): both ends evaluated, values on either side of iso, and the edge lies in a
// known cell (cells node - o with o = 0 wherever the direction's offset has a 1); stats[2] += vertices, stats[3] += those with an
// end that found no interval (value 10)
__global__ void vertex_count_kernel(Lattice L, const double *f, const unsigned char *known, double iso, unsigned char *mask,
                                    int *vcount, unsigned long long *stats) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n_nodes = (long long)L.nx * L.ny * L.nz;
    unsigned long long v_sum = 0, u_sum = 0;
    if (id < n_nodes) {
        int i, j, k;
        node_ijk(L, id, i, j, k);
        const double f0 = f[id];
        unsigned m = 0;
        int nu = 0;
        if (!(f0 != f0)) {
            const int ex = L.nx - 1, ey = L.ny - 1, ez = L.nz - 1;
            for (int d = 0; d < 7; d++) {
                const int o = c_offset_of_dir[d], dx = o & 1, dy = (o >> 1) & 1, dz = (o >> 2) & 1;
                if (i + dx >= L.nx || j + dy >= L.ny || k + dz >= L.nz) continue;
                const double f1 = f[node_id(L, i + dx, j + dy, k + dz)];
                if (f1 != f1 || ((f0 < iso) == (f1 < iso))) continue;
                bool in_cell = false;
                for (int c = 0; c < 8 && !in_cell; c++) {
                    if (c & o) continue;
                    const int ci = i - (c & 1), cj = j - ((c >> 1) & 1), ck = k - ((c >> 2) & 1);
                    if (ci < 0 || cj < 0 || ck < 0 || ci >= ex || cj >= ey || ck >= ez) continue;
                    in_cell = known[((long long)ci * ey + cj) * ez + ck] != 0;
                }
                if (!in_cell) continue;
                m |= 1u << d;
                nu += (f0 == 1e1 || f1 == 1e1) ? 1 : 0;
            }
        }
        mask[id] = (unsigned char)m;
        vcount[id] = __popc(m);
        v_sum = __popc(m); u_sum = nu;
    }
    v_sum = wave_sum(v_sum); u_sum = wave_sum(u_sum);
    if ((threadIdx.x & 63) == 0) { if (v_sum) atomicAdd(&stats[2], v_sum); if (u_sum) atomicAdd(&stats[3], u_sum); }
}

// vertex positions: linear interpolation of the two node values along the edge, from its lower node - node + t * (d * eps) with
// t = (iso - f0) / (f1 - f0), every operation rounded on its own (no contraction into an fma)
__global__ void vertex_emit_kernel(Lattice L, const double *f, double iso, const unsigned char *mask, const int *vbase, double *V) {
#pragma clang fp contract(off)
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)L.nx * L.ny * L.nz) return;
    const unsigned m = mask[id];
    if (!m) return;
    int i, j, k;
    node_ijk(L, id, i, j, k);
    const double f0 = f[id];
    const double px = L.ox + (double)i * L.eps, py = L.oy + (double)j * L.eps, pz = L.oz + (double)k * L.eps;
    int out = vbase[id];
    for (int d = 0; d < 7; d++) {
        if (!((m >> d) & 1u)) continue;
        const int o = c_offset_of_dir[d], dx = o & 1, dy = (o >> 1) & 1, dz = (o >> 2) & 1;
        const double f1 = f[node_id(L, i + dx, j + dy, k + dz)];
        const double t = (iso - f0) / (f1 - f0);
        V[3 * (long long)out] = px + t * ((double)dx * L.eps);
        V[3 * (long long)out + 1] = py + t * ((double)dy * L.eps);
        V[3 * (long long)out + 2] = pz + t * ((double)dz * L.eps);
        out++;
    }
}

// vertex index of the edge between cell corners u and w of cell (i, j, k)
__device__ __forceinline__ int edge_vertex(const Lattice &L, int i, int j, int k, int u, int w, const unsigned char *mask, const int *vbase) {
    const int lo = (__popc(u) < __popc(w)) ? u : w, hi = lo == u ? w : u;
    const long long n = node_id(L, i + (lo & 1), j + ((lo >> 1) & 1), k + ((lo >> 2) & 1));
    const int d = c_dir_of_offset[hi ^ lo];
    return vbase[n] + __popc((unsigned)mask[n] & ((1u << d) - 1u));
}
__global__ void tri_emit_kernel(Lattice L, const double *f, double iso, const unsigned char *known, const int *tbase,
                                const unsigned char *mask, const int *vbase, int32_t *F) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ex = L.nx - 1, ey = L.ny - 1, ez = L.nz - 1;
    if (t >= (long long)ex * ey * ez || !known[t]) return;
    const int k = (int)(t % ez), j = (int)((t / ez) % ey), i = (int)(t / ((long long)ez * ey));
    double v[8];
    (void)cell_values(L, f, i, j, k, v);
    long long out = tbase[t];
    for (int p = 0; p < 6; p++) {
        int q[4], e[2][3][2];
        kuhn_tet(p, q);
        const bool in[4] = {v[q[0]] < iso, v[q[1]] < iso, v[q[2]] < iso, v[q[3]] < iso};
        const int n = tet_tris(q, in, e);
        for (int r = 0; r < n; r++, out++)
            for (int s = 0; s < 3; s++) F[3 * out + s] = edge_vertex(L, i, j, k, e[r][s][0], e[r][s][1], mask, vbase);
    }
}

// ---- host helpers ---------------------------------------------------------------------------------------------------
// the field at the nodes [0, n) of a list (ids) or of the lattice (ids == null) into f[node]
int field_nodes(isdf_ctx *c, int N, const double *d_T, const double *d_C, const Lattice &L, const int *ids, long long n, int mode,
                double *f, hipStream_t st) {
    DevBuf<double> xyz, val;
    const long long chunk = std::min<long long>(n, 16 * (long long)FIELD_CHUNK);
    HIPCHK(c, xyz.alloc((size_t)chunk * 3));
    HIPCHK(c, val.alloc((size_t)chunk));
    for (long long b = 0; b < n; b += chunk) {
        const int m = (int)std::min(chunk, n - b);
        hipLaunchKernelGGL(node_xyz_kernel, dim3(blocks(m)), dim3(256), 0, st, L, ids, b, m, xyz.get());
        ISDF_TRY(swept_field_run(c, N, d_T, d_C, xyz.get(), m, mode, val.get(), nullptr, st));
        hipLaunchKernelGGL(node_scatter_kernel, dim3(blocks(m)), dim3(256), 0, st, ids, b, m, val.get(), f);
    }
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

int check_mesh_params(isdf_ctx *c, const isdf_swept_mesh_params *p) {
    if (!p) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: null parameters");
    if (!(p->eps > 0.0) || !std::isfinite(p->eps)) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: eps must be finite and > 0");
    if (!(p->iso >= 0.0) || !std::isfinite(p->iso)) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: iso must be finite and >= 0");
    if (p->mode != ISDF_SWEPT_FIELD_PLANNER && p->mode != ISDF_SWEPT_FIELD_CLOSED) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: unknown mode");
    if (p->band < 0) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: band must be >= 0");
    if (p->band > 0 && (!(p->lipschitz > 0.0) || !std::isfinite(p->lipschitz))) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: lipschitz must be finite and > 0");
    if (p->use_bbox)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(p->bmin[a]) || !std::isfinite(p->bmax[a]) || !(p->bmax[a] > p->bmin[a]))
                return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: bbox needs bmin < bmax");
    return ISDF_OK;
}

// AABB of the trajectory's positions: 64 samples per piece plus, per axis, the largest bulge of the polynomial between two samples
// (h^2 / 8 * max |p''|, with |p''| bounded by its coefficients' absolute values)
void traj_aabb(int N, const double *T, const double *C, double lo[3], double hi[3]) {
    const int S = 64;
    const size_t ld = (size_t)6 * N;
    for (int a = 0; a < 3; a++) { lo[a] = 1e300; hi[a] = -1e300; }
    for (int i = 0; i < N; i++) {
        const double h = T[i] / S;
        for (int a = 0; a < 3; a++) {
            const double *c = C + a * ld + 6 * (size_t)i;
            double acc_max = 0.0, tp = 1.0;
            for (int k = 2; k < 6; k++) { acc_max += k * (k - 1) * std::fabs(c[k]) * tp; tp *= T[i]; }
            const double bulge = h * h / 8.0 * acc_max;
            for (int s = 0; s <= S; s++) {
                const double t = s == S ? T[i] : s * h;
                const double x = ((((c[5] * t + c[4]) * t + c[3]) * t + c[2]) * t + c[1]) * t + c[0];
                lo[a] = std::min(lo[a], x - bulge); hi[a] = std::max(hi[a], x + bulge);
            }
        }
    }
}

// ---- extraction: count, scan, emit.  The mesh of the field f (device, NaN = node not evaluated) on lattice L into s->d_V / s->d_F,
// asynchronous on `st` after the counters' read-back; cnt = known cells, triangles, vertices, unqualified edges.  The caller
// synchronises and then takes the mesh as kept (nV, nF, have_mesh).
int extract_mesh(isdf_ctx *c, SweptMeshState *s, const Lattice &L, const double *f, double iso, hipStream_t st, unsigned long long cnt[4]) {
    const long long n_nodes = (long long)L.nx * L.ny * L.nz;
    const long long n_cells = (long long)(L.nx - 1) * (L.ny - 1) * (L.nz - 1);
    DevBuf<unsigned char> known, mask;
    DevBuf<int> tcount, tbase, vcount, vbase;
    DevBuf<unsigned long long> d_cnt;
    HIPCHK(c, known.alloc((size_t)n_cells)); HIPCHK(c, tcount.alloc((size_t)n_cells)); HIPCHK(c, tbase.alloc((size_t)n_cells));
    HIPCHK(c, mask.alloc((size_t)n_nodes)); HIPCHK(c, vcount.alloc((size_t)n_nodes)); HIPCHK(c, vbase.alloc((size_t)n_nodes));
    HIPCHK(c, d_cnt.alloc(4));
    HIPCHK(c, hipMemsetAsync(d_cnt.get(), 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(cell_count_kernel, dim3(blocks(n_cells)), dim3(256), 0, st, L, f, iso, known.get(), tcount.get(), d_cnt.get());
    hipLaunchKernelGGL(vertex_count_kernel, dim3(blocks(n_nodes)), dim3(256), 0, st, L, f, (const unsigned char *)known.get(),
                       iso, mask.get(), vcount.get(), d_cnt.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cnt, d_cnt.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (cnt[1] > (unsigned long long)INT32_MAX / 3 || cnt[2] > (unsigned long long)INT32_MAX / 3)
        return fail(c, ISDF_ERR_OVERFLOW, "swept mesh: more than 2^31 / 3 vertices or triangles");
    DevBuf<unsigned char> tmp;          // each scan's scratch is its own and is freed behind it
    ISDF_TRY(exclusive_sum(c, tmp, tcount.get(), tbase.get(), n_cells, st)); tmp.release();
    ISDF_TRY(exclusive_sum(c, tmp, vcount.get(), vbase.get(), n_nodes, st)); tmp.release();
    HIPCHK(c, s->d_V.alloc((size_t)(cnt[2] ? cnt[2] : 1) * 3));
    HIPCHK(c, s->d_F.alloc((size_t)(cnt[1] ? cnt[1] : 1) * 3));
    hipLaunchKernelGGL(vertex_emit_kernel, dim3(blocks(n_nodes)), dim3(256), 0, st, L, f, iso,
                       (const unsigned char *)mask.get(), (const int *)vbase.get(), s->d_V);
    hipLaunchKernelGGL(tri_emit_kernel, dim3(blocks(n_cells)), dim3(256), 0, st, L, f, iso,
                       (const unsigned char *)known.get(), (const int *)tbase.get(), (const unsigned char *)mask.get(), (const int *)vbase.get(), s->d_F);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_swept_sdf_device(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const double *d_xyz, long long n,
                                     int mode, double *d_value_out, double *d_tstar_out, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (N < 1 || !d_T || !d_coeffs || n < 0 || (n > 0 && (!d_xyz || !d_value_out))) return fail(c, ISDF_ERR_INVALID_ARG, "swept field: bad arguments");
    if (mode != ISDF_SWEPT_FIELD_PLANNER && mode != ISDF_SWEPT_FIELD_CLOSED) return fail(c, ISDF_ERR_INVALID_ARG, "swept field: unknown mode");
    ISDF_TRY(swept_check_ctx(c));
    HIPCHK(c, hipSetDevice(c->device));
    // the 300 s rule needs the durations on the host
    std::vector<double> hT(N);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(c, hipMemcpyAsync(hT.data(), d_T, N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ISDF_TRY(swept_check_traj(c, N, hT.data()));
    return swept_field_run(c, N, d_T, d_coeffs, d_xyz, n, mode, d_value_out, d_tstar_out, st);
}

extern "C" int isdf_swept_sdf(isdf_ctx *c, int N, const double *T, const double *coeffs, const double *xyz, long long n, int mode,
                              double *value_out, double *tstar_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (N < 1 || !T || !coeffs || n < 0 || (n > 0 && (!xyz || !value_out))) return fail(c, ISDF_ERR_INVALID_ARG, "swept field: bad arguments");
    if (mode != ISDF_SWEPT_FIELD_PLANNER && mode != ISDF_SWEPT_FIELD_CLOSED) return fail(c, ISDF_ERR_INVALID_ARG, "swept field: unknown mode");
    ISDF_TRY(swept_check_ctx(c));
    ISDF_TRY(swept_check_traj(c, N, T));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf<double> d_in, d_xyz, d_out;
    HIPCHK(c, d_in.alloc((size_t)19 * N));
    HIPCHK(c, d_xyz.alloc((size_t)3 * n));
    HIPCHK(c, d_out.alloc((size_t)2 * n));
    HIPCHK(c, hipMemcpyAsync(d_in.get(), T, N * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_in.get() + N, coeffs, (size_t)18 * N * sizeof(double), hipMemcpyHostToDevice, st));
    if (n > 0) HIPCHK(c, hipMemcpyAsync(d_xyz.get(), xyz, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, st));
    ISDF_TRY(swept_field_run(c, N, d_in.get(), d_in.get() + N, d_xyz.get(), n, mode, d_out.get(), d_out.get() + n, st));
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(value_out, d_out.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        if (tstar_out) HIPCHK(c, hipMemcpyAsync(tstar_out, d_out.get() + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return ISDF_OK;
}

extern "C" void isdf_swept_mesh_params_default(isdf_swept_mesh_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->eps = 0.1;
    p->iso = 0.0;
    p->mode = ISDF_SWEPT_FIELD_CLOSED;
    p->band = 4;
    p->lipschitz = 1.0;
    p->use_bbox = 0;
}

extern "C" int isdf_swept_mesh_build(isdf_ctx *c, int N, const double *T, const double *coeffs, const isdf_swept_mesh_params *p,
                                     isdf_swept_mesh_info *info_out) {
    // (arguments first: a NULL ctx with bad arguments reports what is wrong with them through isdf_last_error(NULL))
    if (N < 1 || !T || !coeffs) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: null trajectory");
    ISDF_TRY(check_mesh_params(c, p));
    if (!c) return fail(nullptr, ISDF_ERR_INVALID_ARG, "swept mesh: null ctx");
    ISDF_TRY(swept_check_ctx(c));
    ISDF_TRY(swept_check_traj(c, N, T));
    for (int k = 0; k < 18 * N; k++) if (!std::isfinite(coeffs[k])) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: non-finite coefficient");
    HIPCHK(c, hipSetDevice(c->device));
    SweptMeshState *s;
    ISDF_TRY(swept_field_scratch(c, &s));
    free_mesh_result(s);
    hipStream_t st = c->stream;

    // ---- the lattice
    const double eps = p->eps;
    double lo[3], hi[3];
    if (p->use_bbox) {
        for (int a = 0; a < 3; a++) { lo[a] = p->bmin[a]; hi[a] = p->bmax[a]; }
    } else {
        const double R = c->shape.kind == ISDF_SHAPE_MESH ? c->mesh_rmax : c->shape_host.bound_radius;
        if (!(R > 0.0) || !std::isfinite(R)) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: the shape has no bound radius - pass a box (use_bbox)");
        traj_aabb(N, T, coeffs, lo, hi);
        const double grow = R + p->iso + 2.0 * eps;
        for (int a = 0; a < 3; a++) { lo[a] -= grow; hi[a] += grow; }
    }
    Lattice L{};
    long long dims[3];
    double org[3];
    for (int a = 0; a < 3; a++) {
        org[a] = std::floor(lo[a] / eps) * eps;
        dims[a] = (long long)std::ceil((hi[a] - org[a]) / eps) + 1;
        if (dims[a] < 2) dims[a] = 2;
    }
    if (!(dims[0] <= MESH_MAX_NODES && dims[1] <= MESH_MAX_NODES && dims[2] <= MESH_MAX_NODES) || dims[0] * dims[1] * dims[2] > MESH_MAX_NODES) {
        char msg[200];
        std::snprintf(msg, sizeof(msg), "swept mesh: %lld x %lld x %lld lattice nodes exceed the cap of %lld - a larger eps or a smaller box",
                      dims[0], dims[1], dims[2], MESH_MAX_NODES);
        return fail(c, ISDF_ERR_INVALID_ARG, msg);
    }
    L.nx = (int)dims[0]; L.ny = (int)dims[1]; L.nz = (int)dims[2];
    L.ox = org[0]; L.oy = org[1]; L.oz = org[2]; L.eps = eps;
    const long long n_nodes = dims[0] * dims[1] * dims[2];

    // ---- the trajectory on the device
    ISDF_TRY(s->d_traj.reserve(c, (size_t)19 * N));
    HIPCHK(c, hipMemcpyAsync(s->d_traj, T, N * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->d_traj + N, coeffs, (size_t)18 * N * sizeof(double), hipMemcpyHostToDevice, st));
    const double *d_T = s->d_traj, *d_C = s->d_traj + N;

    DevEvents<3> ev;
    ISDF_TRY(ev.ready(c));
    DevBuf<double> f;
    HIPCHK(c, f.alloc((size_t)n_nodes));
    HIPCHK(c, hipMemsetAsync(f.get(), 0xFF, (size_t)n_nodes * sizeof(double), st));      // all-ones = NaN: not evaluated
    HIPCHK(c, hipEventRecord(ev[0], st));

    // ---- the field: dense, or coarse lattice + narrow band
    long long coarse_points = 0, fine_points = 0;
    if (p->band == 0) {
        ISDF_TRY(field_nodes(c, N, d_T, d_C, L, nullptr, n_nodes, p->mode, f.get(), st));
        fine_points = n_nodes;
    } else {
        const int B = p->band;
        Coarse Q{B, (int)((dims[0] - 1 + B - 1) / B + 1), (int)((dims[1] - 1 + B - 1) / B + 1), (int)((dims[2] - 1 + B - 1) / B + 1)};
        const long long n_coarse = (long long)Q.cx * Q.cy * Q.cz, n_ccells = (long long)(Q.cx - 1) * (Q.cy - 1) * (Q.cz - 1);
        DevBuf<int> cids;
        HIPCHK(c, cids.alloc((size_t)n_coarse));
        hipLaunchKernelGGL(coarse_ids_kernel, dim3(blocks(n_coarse)), dim3(256), 0, st, L, Q, cids.get());
        ISDF_TRY(field_nodes(c, N, d_T, d_C, L, cids.get(), n_coarse, p->mode, f.get(), st));
        coarse_points = n_coarse;
        DevBuf<unsigned char> refine, flag;
        HIPCHK(c, refine.alloc((size_t)n_ccells));
        HIPCHK(c, flag.alloc((size_t)n_nodes));
        const double thr = p->lipschitz * std::sqrt(3.0) * B * eps;
        const double unq = 2 * c->cfg.safety_hor + 0.1;
        hipLaunchKernelGGL(refine_kernel, dim3(blocks(n_ccells)), dim3(256), 0, st, L, Q, f.get(), p->iso, thr, unq, refine.get());
        hipLaunchKernelGGL(flag_kernel, dim3(blocks(n_nodes)), dim3(256), 0, st, L, Q, refine.get(), flag.get());
        DevBuf<int> fids, d_nsel;
        HIPCHK(c, fids.alloc((size_t)n_nodes));
        HIPCHK(c, d_nsel.alloc(1));
        size_t bytes = 0;
        hipcub::CountingInputIterator<int> it(0);
        HIPCHK(c, hipcub::DeviceSelect::Flagged(nullptr, bytes, it, flag.get(), fids.get(), d_nsel.get(), (int)n_nodes, st));
        {
            DevBuf<unsigned char> tmp;
            HIPCHK(c, tmp.alloc(bytes));
            HIPCHK(c, hipcub::DeviceSelect::Flagged(tmp.get(), bytes, it, flag.get(), fids.get(), d_nsel.get(), (int)n_nodes, st));
            int nsel = 0;
            HIPCHK(c, hipMemcpyAsync(&nsel, d_nsel.get(), sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            fine_points = nsel;
        }
        ISDF_TRY(field_nodes(c, N, d_T, d_C, L, fids.get(), fine_points, p->mode, f.get(), st));
    }
    HIPCHK(c, hipEventRecord(ev[1], st));

    unsigned long long cnt[4];
    ISDF_TRY(extract_mesh(c, s, L, f.get(), p->iso, st, cnt));
    HIPCHK(c, hipEventRecord(ev[2], st));
    HIPCHK(c, hipStreamSynchronize(st));
    s->nV = (long long)cnt[2]; s->nF = (long long)cnt[1]; s->have_mesh = true;
    if (info_out) {
        std::memset(info_out, 0, sizeof(*info_out));
        for (int a = 0; a < 3; a++) { info_out->dims[a] = (int)dims[a]; info_out->origin[a] = org[a]; }
        info_out->eps = eps;
        info_out->coarse_points = coarse_points;
        info_out->fine_points = fine_points;
        info_out->band_cells = (long long)cnt[0];
        info_out->n_vertices = s->nV;
        info_out->n_triangles = s->nF;
        info_out->unqualified_edges = (long long)cnt[3];
        float ms0 = 0.f, ms1 = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms0, ev[0], ev[1]));
        HIPCHK(c, hipEventElapsedTime(&ms1, ev[1], ev[2]));
        info_out->field_ms = ms0; info_out->mesh_ms = ms1;
    }
    return ISDF_OK;
}

extern "C" int isdf_lattice_mesh_build(isdf_ctx *c, const int32_t dims[3], const double origin[3], double eps, double iso, const double *f,
                                       isdf_swept_mesh_info *info_out) {
    // (arguments first, as in isdf_swept_mesh_build)
    if (!dims || !origin || !f) return fail(c, ISDF_ERR_INVALID_ARG, "lattice mesh: null dims, origin or field");
    if (!(eps > 0.0) || !std::isfinite(eps)) return fail(c, ISDF_ERR_INVALID_ARG, "lattice mesh: eps must be finite and > 0");
    if (!std::isfinite(iso)) return fail(c, ISDF_ERR_INVALID_ARG, "lattice mesh: iso must be finite");
    long long n_nodes = 1;
    for (int a = 0; a < 3; a++) {
        if (dims[a] < 2) return fail(c, ISDF_ERR_INVALID_ARG, "lattice mesh: dims must be >= 2 per axis");
        if (!std::isfinite(origin[a])) return fail(c, ISDF_ERR_INVALID_ARG, "lattice mesh: non-finite origin");
        n_nodes *= dims[a];
        if (n_nodes > MESH_MAX_NODES) return fail(c, ISDF_ERR_INVALID_ARG, "lattice mesh: more lattice nodes than the cap of 2^27");
    }
    if (!c) return fail(nullptr, ISDF_ERR_INVALID_ARG, "lattice mesh: null ctx");
    HIPCHK(c, hipSetDevice(c->device));
    SweptMeshState *s;
    ISDF_TRY(c->swm.make(c, &s));
    free_mesh_result(s);
    hipStream_t st = c->stream;
    Lattice L{dims[0], dims[1], dims[2], origin[0], origin[1], origin[2], eps};

    DevEvents<2> ev;
    ISDF_TRY(ev.ready(c));
    DevBuf<double> d_f;
    HIPCHK(c, d_f.alloc((size_t)n_nodes));
    HIPCHK(c, hipMemcpyAsync(d_f.get(), f, (size_t)n_nodes * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(ev[0], st));
    unsigned long long cnt[4];
    ISDF_TRY(extract_mesh(c, s, L, d_f.get(), iso, st, cnt));
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipStreamSynchronize(st));
    s->nV = (long long)cnt[2]; s->nF = (long long)cnt[1]; s->have_mesh = true;
    if (info_out) {
        std::memset(info_out, 0, sizeof(*info_out));
        for (int a = 0; a < 3; a++) { info_out->dims[a] = dims[a]; info_out->origin[a] = origin[a]; }
        info_out->eps = eps;
        info_out->band_cells = (long long)cnt[0];
        info_out->n_vertices = s->nV;
        info_out->n_triangles = s->nF;
        info_out->unqualified_edges = (long long)cnt[3];
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
        info_out->mesh_ms = ms;
    }
    return ISDF_OK;
}

extern "C" int isdf_swept_mesh_get(isdf_ctx *c, double *V_out, int capV, int32_t *F_out, int capF) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!c->swm || !c->swm->have_mesh) return fail(c, ISDF_ERR_STATE, "swept mesh: nothing built (isdf_swept_mesh_build)");
    SweptMeshState *s = c->swm.get();
    if (capV < s->nV || capF < s->nF) return fail(c, ISDF_ERR_OVERFLOW, "swept mesh: output capacity smaller than the mesh");
    if ((s->nV > 0 && !V_out) || (s->nF > 0 && !F_out)) return fail(c, ISDF_ERR_INVALID_ARG, "swept mesh: null output");
    HIPCHK(c, hipSetDevice(c->device));
    if (s->nV) HIPCHK(c, hipMemcpy(V_out, s->d_V, (size_t)s->nV * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (s->nF) HIPCHK(c, hipMemcpy(F_out, s->d_F, (size_t)s->nF * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ISDF_OK;
}

extern "C" int isdf_swept_mesh_release(isdf_ctx *c) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (c->swm) free_mesh_result(c->swm.get());
    return ISDF_OK;
}

extern "C" int isdf_write_obj(const char *path, const double *V, int nV, const int32_t *F, int nF) {
    if (!path || nV < 0 || nF < 0 || (nV > 0 && !V) || (nF > 0 && !F)) return ISDF_ERR_INVALID_ARG;
    for (long long k = 0; k < 3ll * nF; k++) if (F[k] < 0 || F[k] >= nV) return ISDF_ERR_INVALID_ARG;
    FILE *o = std::fopen(path, "wb");
    if (!o) return ISDF_ERR_INVALID_ARG;
    bool ok = true;
    // %.17g: every double reads back to the same bits (isdf_read_obj)
    for (int i = 0; i < nV && ok; i++) ok = std::fprintf(o, "v %.17g %.17g %.17g\n", V[3 * i], V[3 * i + 1], V[3 * i + 2]) > 0;
    for (int i = 0; i < nF && ok; i++) ok = std::fprintf(o, "f %d %d %d\n", F[3 * i] + 1, F[3 * i + 1] + 1, F[3 * i + 2] + 1) > 0;
    ok = (std::fclose(o) == 0) && ok;
    return ok ? ISDF_OK : ISDF_ERR_INVALID_ARG;
}
