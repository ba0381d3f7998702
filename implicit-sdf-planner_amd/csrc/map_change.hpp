// What the calls that change the map in place share (map_update.hip: voxels become occupied, map_clear.hip: voxels become free,
// map_scan.hip: both from one range scan, map_shift.hip: the window moves): the grow-only scratch, the typed hand-over records, the
// lane's "I changed a voxel" step and the host steps every driver goes through - begin, stage, hand-over, map changed, the front-end
// stage in its two halves (the shift) or whole with the cost-to-go field following the change (update, clear and, through them, the
// scan), the watch re-check, the ready checks.  The drivers call the steps in their own order; the steps are defined once, in
// map_change.hip.
#pragma once
#include "isdf_ctx.hpp"
#include "frontend_dev.hpp"
#include "map_update_host.hpp"

namespace isdf {

// A count stage's record (the update's, the clear's, and the scan's two): zeroed, box empty, before every stage
struct MapListRecord {
    unsigned n;                         // voxels that changed (may exceed the list's capacity: the full path follows)
    unsigned esdf0;                     // update: bits of the ESDF's first value before the update: +inf = the map had no occupied voxel
    int lo[3], hi[3];                   // the dirty box
    unsigned long long tally;           // update: values that fell (mu_esdf_kernel); clear: points whose voxel's count was 0
    unsigned pad[6];
};
// the clear's ESDF stage
struct McEsdfRecord {
    int lo[3], hi[3];                   // the touched box
    unsigned any_occ, pad0;             // some voxel of the map is still occupied
    unsigned long long touched, raised;
    unsigned pad[4];
};
// the scan's ray stage
struct MsRecord {
    unsigned long long n_skipped, n_hits, n_free, n_hit_voxels;
    int lo[3], hi[3];                   // the visited box
    unsigned long long newly_known;     // with a known grid (map_known.hip): the bits the scan's merge turned from 0 to 1
};
// the shift's translation stage
struct MshRecord {
    unsigned long long counts_left;     // sum of the kept counts of the voxels without a destination
    unsigned long long occupied_left;   // occupied voxels among them
    unsigned any_occ;                   // some voxel of the new window is occupied
    unsigned pad[11];
};
// every record of the family, one 64-byte line each: uploaded empty by map_stage, read back whole by every hand-over
struct MapRecords { MapListRecord list; McEsdfRecord esdf; MsRecord scan; MshRecord shift; };
static_assert(sizeof(MapListRecord) == 64 && sizeof(McEsdfRecord) == 64 && sizeof(MsRecord) == 64 && sizeof(MshRecord) == 64, "each hand-over record is one 64-byte line");

inline MapRecords map_records_empty() {
    MapRecords r{};
    for (int a = 0; a < 3; a++) { r.list.lo[a] = r.esdf.lo[a] = r.scan.lo[a] = 0x7FFFFFFF; r.list.hi[a] = r.esdf.hi[a] = r.scan.hi[a] = -1; }
    return r;
}

// the lane that changed voxel (x, y, z): the voxel goes to the list while there is room, the dirty box widens
__device__ __forceinline__ void map_list_append(MapListRecord *__restrict__ rec, MuVoxel *__restrict__ list, unsigned cap, int x, int y, int z) {
    const unsigned pos = atomicAdd(&rec->n, 1u);
    if (pos < cap) list[pos] = MuVoxel{(unsigned short)x, (unsigned short)y, (unsigned short)z, 0};
    atomicMin(&rec->lo[0], x); atomicMin(&rec->lo[1], y); atomicMin(&rec->lo[2], z);
    atomicMax(&rec->hi[0], x); atomicMax(&rec->hi[1], y); atomicMax(&rec->hi[2], z);
}

}  // namespace isdf

struct MapUpdateState {
    isdf::DevBuf<void> d_in;                  // the call's points or voxel indices
    isdf::DevBuf<isdf::MuVoxel> d_list;       // the new (or cleared) voxels, in no defined order
    isdf::RecPair<isdf::MapRecords> rec;
    isdf::DevBuf<uint4> d_pack; isdf::PinBuf<uint32_t> h_pack;          // the grown box of the configuration space on its way to the host table
    isdf::DevBuf<int> d_edt_a, d_edt_b;       // map_clear.hip: the slabs of the separable transform over the touched box
    isdf::DevBuf<unsigned> d_free_bits, d_hit_bits;     // map_scan.hip: one bit per voxel, the voxels a scan's rays pass / end in
    // map_shift.hip: where the translation writes; each then changes places with the ctx's own buffer (one more copy of the counts, the
    // occupancy and the configuration-space table stays allocated)
    isdf::DevBuf<unsigned> d_shift_counts, d_shift_cspace; isdf::DevBuf<uint8_t> d_shift_occ;
    isdf::DevEvents<2> ev_scan;                          // map_scan.hip: around the ray stage
    // [0], [1]: a count (translation) stage; [2], [3]: the ESDF stage; [4], [5]: the front-end stage; [6], [7]: the field's in-place
    // change inside map_frontend_stage, either direction (a scan's two stages use them one after the other); [6] .. [9]: the field
    // carried through a shift, its two phases
    isdf::DevEvents<10> ev;
};

namespace isdf {

// ---- the shared steps (map_change.hip), in the order a driver meets them
// ready: the three tests every entry point makes before anything moves; op names the operation in the message ("the map update")
// may_follow = false (the shift): a gated cost-to-go field is dropped whatever isdf_frontend_field_set_known_follow says
int map_change_ready(isdf_ctx *c, const char *op, const void *in, long long n, bool needs_counts, bool may_follow = true);
int map_voxels_in_grid(isdf_ctx *c, const int32_t *ijk, long long n);       // ISDF_ERR_INVALID_ARG for an index outside the grid
// begin: the ctx's device current, its scratch created with every event on first use
int map_begin(isdf_ctx *c, MapUpdateState **out);
// list capacity: the most entries a count stage can need, and the cap it is given
unsigned map_list_cap(long long max_voxels, unsigned long long n_in, unsigned long long n_vox);
// stage: S.d_in reserved for `in` and `in2` (one behind the other, either may be empty) and S.d_list for list_len entries (0: no list),
// the records uploaded empty, the input uploaded (a null `in` / `in2` with bytes: room is kept, nothing is uploaded - the caller fills it
// on the stream), ev_begin recorded.  Nothing allocates on a second call of the same size.
int map_stage(isdf_ctx *c, MapUpdateState &S, const void *in, size_t in_bytes, const void *in2, size_t in2_bytes, size_t list_len, hipEvent_t ev_begin);
// hand-over: ev_end recorded (null: none), the records to S.rec.host(), one synchronisation.  The kernels before it may have run, so a
// failure leaves "<op> hand-over: ..." in the ctx and drops what was derived from the old map.
int map_hand_over(isdf_ctx *c, MapUpdateState &S, hipEvent_t ev_end, const char *op, bool voxels);
// After a failure past the point where the occupancy moved: what was derived from the old map goes (as isdf_set_pointcloud drops
// it), the error message stays.  The occupancy and the counts are consistent with each other and stay.
void mu_drop_derived(isdf_ctx *c, bool voxels);
// map changed: the voxel forms' counts no longer describe the occupancy, the bit grid is stale, a valid cost-to-go field is dropped
// (returns 1 then: a driver that repairs it asks isdf_field_change_wanted - the shift: isdf_field_shift_wanted - first)
int map_changed(isdf_ctx *c, bool voxels);
// ... and what a refresh over a list decides before its first stage: the dirty box, grown for the front end, which products are
// refreshed (an ESDF that is switched off is dropped here) and whether a cap of the params is exceeded
struct MapRefresh { MuBox box, grown; bool do_esdf, do_fe, over; };
MapRefresh map_refresh_begin(isdf_ctx *c, const MapListRecord &R, unsigned cap, bool voxels, int refresh_esdf, int refresh_frontend, double full_fraction, int *field_dropped);
// The front-end stage, in two halves around the caller's synchronisation.  _launch: a front end that is switched off (!on) is
// released; ev[4] (stamp == false: the caller recorded it before work of its own); the whole-map refresh (full) or, per (box, grown)
// pair, the dwords of the inflated bit map that cover `box`, the configuration-space words of `grown` if there is a table and, when
// the A* holds the table on the host, that box packed into S.d_pack; ev[5]; the pack buffer on its way to S.h_pack.  The kernels
// recompute from the occupancy: the direction of the change does not show.  _finish, after the synchronisation: the boxes scattered
// into the host table, the stage's time.
struct MapFrontend {
    int n_boxes; MuBox grown[6];
    bool patch; size_t pack_total, pack_at[6];
    int refreshed, cspace_refreshed, host_table_patched; long long cspace_voxels; double ms;
};
int map_frontend_launch(isdf_ctx *c, MapUpdateState &S, bool on, bool full, const MuBox *boxes, const MuBox *grown, int n_boxes, MapFrontend &F, bool stamp = true);
void map_frontend_finish(isdf_ctx *c, MapUpdateState &S, MapFrontend &F);
// The whole stage of a change in one direction (dir: its voxels closed or opened) with the cost-to-go field following it around the one
// synchronisation: _launch over (M.box, M.grown) or the full map, the records on their way to S.rec.host(), when `follow` (the caller asked
// isdf_field_change_wanted before map_refresh_begin dropped the field) the field's begin over M.grown; the synchronisation; the
// field's end - its rounds read one word each -, and only then _finish: the host table is patched after them.  A field that followed:
// *field_dropped = 0.  F: for map_frontend_report.  field_more (nullable): a second box the field's stage covers with M.grown - where a
// scan's new known voxels can have moved a gated field's gate.
int map_frontend_stage(isdf_ctx *c, MapUpdateState &S, FfChange dir, bool follow, bool on, bool full, const MapRefresh &M, MapFrontend &F, int *field_dropped,
                       const MuBox *field_more = nullptr);
template <class Info> inline void map_frontend_report(const MapFrontend &F, Info &info) {       // the update's and the clear's info name these alike
    info.frontend_refreshed = F.refreshed; info.cspace_refreshed = F.cspace_refreshed; info.host_table_patched = F.host_table_patched;
    info.cspace_voxels_recomputed = F.cspace_voxels; info.frontend_ms = F.ms;
}
// watch re-check: removed or moved voxels cannot be subtracted from the kept report's piece minima, so an armed watch's trajectory is
// checked against the whole new map again and stays armed.  A failing check drops the report and fails the call.  *rechecked = armed.
int map_watch_recheck(isdf_ctx *c, bool armed, int32_t *rechecked);

// Everything after the hand-over of a call that occupied (mu_, map_update.hip) or freed (mc_, map_clear.hip) at least one voxel: R is
// the count stage's record as the host read it, S.d_list the new (cleared) voxels, cap the list's capacity; the counts and the occupancy
// are the new map's already.  map_scan.hip runs both, the clear's first.  A failure: the caller calls mu_drop_derived.
int mu_refresh_products(isdf_ctx *c, MapUpdateState &S, const isdf_map_update_params &P, const MapListRecord &R, unsigned cap, bool voxels, isdf_map_update_info &info);
int mc_refresh_products(isdf_ctx *c, MapUpdateState &S, const isdf_map_clear_params &P, const MapListRecord &R, unsigned cap, bool voxels, isdf_map_clear_info &info,
                        const MuBox *field_more = nullptr);      // field_more: map_frontend_stage's

// ---- the scan's stages for callers that bring their rays another way (map_scan.hip; depth_cam.hip's isdf_integrate_depth)
struct MsOrigin { int q[3]; };              // the sensor's tick
// produce: writes n_rays end points and n_rays hit bytes into the staged buffers with work on the ctx's stream; it runs after map_stage
// and before the trace, returns an isdf_status, and must leave the map alone
typedef int (*MsProduce)(isdf_ctx *c, float *d_xyz, uint8_t *d_hit, void *arg);
struct MsInput { const float *xyz; const uint8_t *hit; MsProduce produce; void *arg; };     // host arrays (hit nullable), or produce
int scan_check(isdf_ctx *c, const char *op, const double origin[3], const void *in, long long n, const isdf_map_scan_params *params, isdf_map_scan_params &P, MsOrigin &O);
int scan_integrate(isdf_ctx *c, const MsOrigin &O, const MsInput &in, long long n_rays, const isdf_map_scan_params &P, isdf_map_scan_info *info_out);

// ---- the known grid's hooks (map_known.hip), each called only while c->known.have
// the scan, after its trace: known |= free | hit over the dwords of the visited box of *d_scan, the new bits counted into it
int map_known_merge_launch(isdf_ctx *c, const unsigned *d_free_bits, const unsigned *d_hit_bits, MsRecord *d_scan);
void map_known_merged(isdf_ctx *c, const MsRecord &scan);       // ... and after the hand-over that brought the record back
// the shift, with its translation stage: the grid translated by s (clamped or not) into the second buffer; then the two change places
int map_known_shift_launch(isdf_ctx *c, const int32_t s[3]);
void map_known_shift_swap(isdf_ctx *c);

}  // namespace isdf
