// What the two directions of the in-place map change share on the host side (map_update.hip: voxels become occupied, map_clear.hip:
// voxels become free): the grow-only scratch, the hand-over record's size, the boxed front-end refresh and the clean-up after a failure.
#pragma once
#include "isdf_ctx.hpp"
#include "map_update_host.hpp"

namespace isdf {

// the update's hand-over record: 64 bytes, zeroed (box: empty) before every update
struct MuRecord {
    unsigned n_new;                     // voxels that became occupied (may exceed the list's capacity: the full path follows)
    unsigned esdf0;                     // bits of the ESDF's first value before the update: +inf = the map had no occupied voxel
    int lo[3], hi[3];                   // the dirty box
    unsigned long long lowered;         // mu_esdf_kernel: values that fell
    unsigned pad[6];
};
// the clear's count stage: 64 bytes, zeroed (box: empty) before every clear
struct McRecord {
    unsigned n_cleared;                 // voxels that became free (may exceed the list's capacity: the full path follows)
    unsigned pad0;
    int lo[3], hi[3];                   // the dirty box
    unsigned long long ignored;         // points whose voxel's count was 0
    unsigned pad[6];
};
// the clear's ESDF stage, the second 64 bytes
struct McEsdfRecord {
    int lo[3], hi[3];                   // the touched box
    unsigned any_occ, pad0;             // some voxel of the map is still occupied
    unsigned long long touched, raised;
    unsigned pad[4];
};
// the shift's translation stage (map_shift.hip): 64 bytes, zeroed before every shift
struct MshRecord {
    unsigned long long counts_left;     // sum of the kept counts of the voxels without a destination
    unsigned long long occupied_left;   // occupied voxels among them
    unsigned any_occ;                   // some voxel of the new window is occupied
    unsigned pad[11];
};
static_assert(sizeof(McRecord) == 64 && sizeof(McEsdfRecord) == 64 && sizeof(MuRecord) == 64 && sizeof(MshRecord) == 64, "each hand-over record is one 64-byte line");

}  // namespace isdf

struct MapUpdateState {
    isdf::DevBuf<void> d_in;                  // the call's points or voxel indices
    isdf::DevBuf<isdf::MuVoxel> d_list;       // the new (or cleared) voxels, in no defined order
    isdf::DevBuf<isdf::MuRecord> d_rec; isdf::PinBuf<isdf::MuRecord> h_rec;      // (the clear keeps two records of this size here, the scan three)
    isdf::DevBuf<uint4> d_pack; isdf::PinBuf<uint32_t> h_pack;          // the grown box of the configuration space on its way to the host table
    isdf::DevBuf<int> d_edt_a, d_edt_b;       // map_clear.hip: the slabs of the separable transform over the touched box
    isdf::DevBuf<unsigned> d_free_bits, d_hit_bits;     // map_scan.hip: one bit per voxel, the voxels a scan's rays pass / end in
    // map_shift.hip: where the translation writes; each then changes places with the ctx's own buffer (one more copy of the counts, the
    // occupancy and the configuration-space table stays allocated)
    isdf::DevBuf<unsigned> d_shift_counts, d_shift_cspace; isdf::DevBuf<uint8_t> d_shift_occ;
    hipEvent_t ev_scan[2] = {nullptr, nullptr};          // map_scan.hip: around the ray stage
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};          // [6], [7]: around the field's repair (update) or reopen (clear)
    ~MapUpdateState() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_scan) if (e) (void)hipEventDestroy(e);
    }
};

namespace isdf {

// map_update.hip
float mu_event_ms(hipEvent_t a, hipEvent_t b);
int mu_state(isdf_ctx *c, MapUpdateState **out);        // the ctx's scratch, created with its events on first use
// After a failure past the point where the occupancy moved: what was derived from the old map goes (as isdf_set_pointcloud drops
// it), the error message stays.  The occupancy and the counts are consistent with each other and stay.
void mu_drop_derived(isdf_ctx *c, bool voxels);
// The front end over the box of the changed voxels, on the ctx's stream: the dwords of the inflated bit map that cover `box`, the
// configuration-space words of `grown` if there is a table (*cspace_voxels) and, when the A* holds the table on the host, that box
// packed into S.d_pack (*patch, *pack_words: the caller copies it to S.h_pack and scatters it after its synchronisation).  The
// kernels recompute from the occupancy: the direction of the change does not show.  pack_offset (dwords): where in S.d_pack the box
// goes - a caller with several boxes (map_shift.hip) reserves S.d_pack and S.h_pack for all of them first, so that nothing grows here.
int mu_frontend_box_launch(isdf_ctx *c, MapUpdateState &S, const MuBox &box, const MuBox &grown, bool *patch, size_t *pack_words, long long *cspace_voxels,
                           size_t pack_offset = 0);
// Everything after the hand-over of a call that occupied (mu_, map_update.hip) or freed (mc_, map_clear.hip) at least one voxel: R is
// the count stage's record as the host read it, S.d_list the new (cleared) voxels, cap the list's capacity; the counts and the occupancy
// are the new map's already.  map_scan.hip runs both, the clear's first.  A failure: the caller calls mu_drop_derived.
int mu_refresh_products(isdf_ctx *c, MapUpdateState &S, const isdf_map_update_params &P, const MuRecord &R, unsigned cap, bool voxels, isdf_map_update_info &info);
int mc_refresh_products(isdf_ctx *c, MapUpdateState &S, const isdf_map_clear_params &P, const McRecord &R, unsigned cap, bool voxels, isdf_map_clear_info &info);

}  // namespace isdf
