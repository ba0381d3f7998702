// The host path the map's read-only queries share (host-only): map_raycast.hip, depth_cam.hip, view_gain.hip, map_known.hip and
// frontier_cluster.hip gate, count and report a call through these, so a query's file holds its rules, its kernels and the order of its own
// launches.  Nothing here launches a kernel, and nothing here is for one query alone.  The state on first use and the parameters'
// defaults are traj_call.hpp's, used where they are: a state needs no more than a ready(c).
#pragma once
#include "traj_call.hpp"
#include "map_scan_host.hpp"
#include <string>

namespace isdf {

// the ctx's map as the queries' kernels and MU_HD functions take it (without a map: zeros, and the call's state gate refuses)
inline MapGeom map_geom(const DevGrid &G) {
    const int dims[3] = {G.X, G.Y, G.Z};
    return map_geom(G.bmin, G.bmax, G.res, dims);
}

}  // namespace isdf

namespace map_query {

using traj_call::resolve;
using traj_call::state_of;

// ---- the gates.  Each entry point calls them in its own order among its argument checks; `what` is the call's own sentence.
inline int single_device(isdf_ctx *c, const char *what) {
    if (!c->peers.empty() || c->is_peer) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, what);
    return ISDF_OK;
}

// who: the sentence's subject ("casting rays")
inline int has_occupancy(isdf_ctx *c, const char *who) {
    if (!c->have_geom || !c->d_occ)
        return isdf_fail(c, ISDF_ERR_STATE, (std::string(who) + " needs an occupancy grid (isdf_set_grid with ISDF_GRID_OCCUPANCY, or isdf_set_pointcloud)").c_str());
    return ISDF_OK;
}

inline int has_known(isdf_ctx *c, const char *what) {
    if (!c->known.have) return isdf_fail(c, ISDF_ERR_STATE, what);
    return ISDF_OK;
}

// ---- the bracket round a counted launch.  With `count`: ev[0] before the launches and ev[1] after them; a call that counts into a
// record has it emptied before ev[0] and on its way to the host after ev[1].  Without: nothing.
inline int count_begin(isdf_ctx *c, bool count, const DevEvents<2> &ev, hipStream_t st) {
    if (count) HIPCHK(c, hipEventRecord(ev[0], st));
    return ISDF_OK;
}
template <typename Rec> int count_begin(isdf_ctx *c, bool count, const DevEvents<2> &ev, RecPair<Rec> &rec, hipStream_t st) {
    if (count) HIPCHK(c, rec.zero(st));
    return count_begin(c, count, ev, st);
}
inline int count_end(isdf_ctx *c, bool count, const DevEvents<2> &ev, hipStream_t st) {
    if (count) HIPCHK(c, hipEventRecord(ev[1], st));
    return ISDF_OK;
}
template <typename Rec> int count_end(isdf_ctx *c, bool count, const DevEvents<2> &ev, RecPair<Rec> &rec, hipStream_t st) {
    ISDF_TRY(count_end(c, count, ev, st));
    if (count) HIPCHK(c, rec.fetch(st));
    return ISDF_OK;
}

// the tail of a device form: with info_out the call's one synchronisation, then fill(info_out) from what the bracket brought back
template <typename Info, typename Fill> int info_after(isdf_ctx *c, Info *info_out, hipStream_t st, Fill fill) {
    if (!info_out) return ISDF_OK;
    HIPCHK(c, hipStreamSynchronize(st));
    fill(info_out);
    return ISDF_OK;
}

}  // namespace map_query
