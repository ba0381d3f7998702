// Front-end device code shared by the whole-map passes (frontend.hip) and the boxed refresh of the in-place map update
// (map_update.hip): the parameter block, one dword of the inflated bit-packed map, one voxel's word of the configuration space.
// Integer / bit work only: the two users produce the same bytes whatever flags they are compiled with.
#pragma once
#include "isdf_ctx.hpp"

namespace isdf {

struct FeParams {
    int k, n_att, side;          // kernel_size, attitudes, (k - 1) / 2
    double res, margin;
    int iX, iY, iZW;             // inflated map: X + 2h, Y + 2h, dwords per z-row (one spare dword at the end of every row)
    int X, Y, Z;
};

struct FeRow { unsigned off, word; };      // off = (i * iY + j) * iZW: where the tile row starts relative to the voxel's own row

inline FeParams fe_params(const isdf_ctx *c) {
    FeParams F{};
    F.k = c->fe.cfg.kernel_size; F.n_att = c->fe.xk * c->fe.yk; F.side = (F.k - 1) / 2;
    F.res = c->grid.res; F.margin = c->fe.margin;
    F.X = c->grid.X; F.Y = c->grid.Y; F.Z = c->grid.Z;
    F.iX = F.X + 2 * F.side; F.iY = F.Y + 2 * F.side; F.iZW = (F.Z + 2 * F.side + 31) / 32 + 1;
    return F;
}

// dword w of row (fx, fy) of the inflated map: bit b = voxel (fx - side, fy - side, 32 w + b - side) is inside the map and occupied
__device__ __forceinline__ unsigned fe_map_bits_word(const FeParams &F, const uint8_t *__restrict__ occ, int fx, int fy, int w) {
    const int x = fx - F.side, y = fy - F.side;
    unsigned v = 0;
    if (x >= 0 && x < F.X && y >= 0 && y < F.Y) {
        const uint8_t *row = occ + ((size_t)x * F.Y + y) * F.Z;
        for (int bit = 0; bit < 32; bit++) {
            const int z = (w << 5) + bit - F.side;
            if (z >= 0 && z < F.Z && row[z] == 1) v |= 1u << bit;
        }
    }
    return v;
}

// One lane's voxel (x, y, z) of the configuration space, called by every lane of a wavefront whose lanes hold consecutive z of one
// column; a lane past the end of its z range comes with valid = false, takes part in the ballots and writes nothing.
__device__ __forceinline__ void fe_cspace_voxel(const FeParams &F, const uint8_t *__restrict__ occ, const unsigned *__restrict__ bits,
                                                const FeRow *__restrict__ rows, const int *__restrict__ row_ptr, uint4 *__restrict__ out,
                                                int x, int y, int z, bool valid) {
    const int zc = valid ? z : F.Z - 1;
    const bool is_occ = occ[((size_t)x * F.Y + y) * F.Z + zc] == 1;
    const unsigned *base = bits + ((size_t)x * F.iY + y) * F.iZW + (zc >> 5);
    const int sh = zc & 31;
    const unsigned kmask = (F.k >= 32) ? 0xFFFFFFFFu : ((1u << F.k) - 1u);
    const bool work = valid && !is_occ;
    const int nq = (F.n_att + 127) >> 7;                  // 128-attitude groups = uint4 words per voxel
    for (int q = 0; q < nq; q++) {
        unsigned m[4] = {0u, 0u, 0u, 0u};
        const int a_end = min(F.n_att, (q + 1) << 7);
        for (int a = q << 7; a < a_end; a++) {
            const int r0 = row_ptr[a], r1 = row_ptr[a + 1];
            unsigned hit = work ? 0u : 1u;
            for (int r = r0; r < r1; r++) {
                if ((r & 7) == 0 && __ballot(hit == 0u) == 0ull) break;          // every lane has already collided (or has no work)
                const FeRow e = rows[r];                                           // wave-uniform
                const unsigned *p = base + e.off;
                const unsigned b0 = p[0], b1 = p[1];
                const unsigned mb = (sh ? ((b0 >> sh) | (b1 << (32 - sh))) : b0) & kmask;
                hit |= mb & e.word;
            }
            if (hit == 0u) m[(a >> 5) & 3] |= 1u << (a & 31);
        }
        if (valid) out[(((size_t)x * F.Y + y) * F.Z + z) * nq + q] = make_uint4(m[0], m[1], m[2], m[3]);
    }
}

}  // namespace isdf

// frontend.hip, for the map update's full path: the whole inflated map again from the ctx's occupancy, the whole configuration space
// again if there was one (device time of that pass in *cspace_ms), the host copy of the table marked stale
int isdf_frontend_refresh_map(isdf_ctx *c, double *cspace_ms);
// its first step alone, for the map shift's incremental path: the whole inflated map again on the ctx's stream (a built front end)
int isdf_frontend_map_bits(isdf_ctx *c);

// frontend_field.hip, for the in-place map changes: the cost-to-go field following a change in place - repaired after voxels closed
// (isdf_frontend_field_set_repair, mode 1) or lowered after voxels opened (isdf_frontend_field_set_reopen, mode 1).
// ..._wanted: the direction's mode is 1 and the field is valid and a fixed point (not status 2).  ..._begin enqueues the direction's
// mark over the box lo .. hi (null: the whole grid), closing: the reset, and the first list on the ctx's stream, after the
// configuration-space refresh; the caller synchronises the stream; ..._end, given the same box, runs the rounds and the counts.
// *kept = 0: a bit had moved against the direction, the field stays dropped.
namespace isdf { enum class FfChange { Closing, Opening }; }
bool isdf_field_change_wanted(const isdf_ctx *c, isdf::FfChange dir);
int isdf_field_change_begin(isdf_ctx *c, isdf::FfChange dir, const int lo[3], const int hi[3], hipEvent_t ev_start);
int isdf_field_change_end(isdf_ctx *c, isdf::FfChange dir, const int lo[3], const int hi[3], hipEvent_t ev_start, hipEvent_t ev_end, int *kept);
// ... and carried through a shift of the map window by s, which moves bits both ways (isdf_frontend_field_set_shift, mode 1; DESIGN
// 4.6.4).  ..._wanted, asked before the shift drops the field: the mode is 1, the field valid and a fixed point, there is a table, the
// goal cell stays inside the grid and not everything leaves.  ..._begin enqueues the translation and the closing phase's reset after
// the shift's configuration-space refresh and moves the goal cell; the caller synchronises the stream; ..._end runs the closing
// phase's rounds, then the opening direction over the box lo .. hi (null: the whole grid).  ev: four events, [0] for ..._begin.
// A field gated by the eroded known grid (isdf_frontend_field_build_known) is never carried through a shift, and with
// follow mode 0 (isdf_frontend_field_set_known_follow) it follows nothing: whatever can change K or the map calls
// isdf_field_known_changed first, which drops it (1: a field was dropped; an ungated field is not touched).  With follow mode 1
//  that call keeps a gated field that is valid, a fixed point and has its table - isdf_field_follow_wanted - and the
// calling driver must run the stages or drop the field itself (isdf_field_gate_drop: the unconditional drop, which the shift and
// isdf_map_known_enable call): isdf_field_change_wanted then answers for a gated field by the follow mode alone, in both directions,
// and isdf_field_change_begin re-erodes K at the field's own (radius, border) and marks with ballot(table) & E.
// isdf_field_follow_stage: one stage on its own - begin, the synchronisation, end -, for a change of K without a table refresh; a
// failure or a bit against the direction drops the field (*kept = 0).  isdf_field_follow_call: a new public call begins - the next
// followed stage starts a new isdf_field_follow_info.
// isdf_field_read_ready: what the field's getters answer before they read - ISDF_OK with a valid field (gated or not), else the
// status and the sentence of isdf_frontend_field_value; for a query elsewhere that reads c->fe.d_field (view_select.hip).
int isdf_field_read_ready(isdf_ctx *c);
int isdf_field_known_changed(isdf_ctx *c);
int isdf_field_gate_drop(isdf_ctx *c);
bool isdf_field_follow_wanted(const isdf_ctx *c);
void isdf_field_follow_call(isdf_ctx *c);
int isdf_field_follow_stage(isdf_ctx *c, isdf::FfChange dir, const int lo[3], const int hi[3], hipEvent_t ev_start, hipEvent_t ev_end, int *kept);
bool isdf_field_shift_wanted(const isdf_ctx *c, const int32_t s[3]);
int isdf_field_shift_begin(isdf_ctx *c, const int32_t s[3], hipEvent_t ev_start);
int isdf_field_shift_end(isdf_ctx *c, const int32_t s[3], const int lo[3], const int hi[3], const hipEvent_t ev[4]);
