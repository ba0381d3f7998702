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
static_assert(sizeof(MuRecord) == 64, "the hand-over record is one 64-byte line");

}  // namespace isdf

struct MapUpdateState {
    isdf::DevBuf<void> d_in;                  // the call's points or voxel indices
    isdf::DevBuf<isdf::MuVoxel> d_list;       // the new (or cleared) voxels, in no defined order
    isdf::DevBuf<isdf::MuRecord> d_rec; isdf::PinBuf<isdf::MuRecord> h_rec;      // (the clear keeps two records of this size here)
    isdf::DevBuf<uint4> d_pack; isdf::PinBuf<uint32_t> h_pack;          // the grown box of the configuration space on its way to the host table
    isdf::DevBuf<int> d_edt_a, d_edt_b;       // map_clear.hip: the slabs of the separable transform over the touched box
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};          // [6], [7]: around the field's repair (update) or reopen (clear)
    ~MapUpdateState() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
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
// kernels recompute from the occupancy: the direction of the change does not show.
int mu_frontend_box_launch(isdf_ctx *c, MapUpdateState &S, const MuBox &box, const MuBox &grown, bool *patch, size_t *pack_words, long long *cspace_voxels);

}  // namespace isdf
