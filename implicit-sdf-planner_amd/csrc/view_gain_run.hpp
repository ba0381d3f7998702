// What another query needs to score poses with the view gain (host-only): the state of view_gain.hip and the declarations of its
// checks and of its launches.  view_gain.hip defines them; view_cand.hip scores its dense pose table through them.
#pragma once
#include "map_query.hpp"
#include "view_gain_host.hpp"

// the host-pointer form's staging, the per-view table, the chunk's seen grids, the image without a return and the rows' pinned copy
struct ViewGainState {
    isdf::DevBuf<double> d_poses;
    isdf::DevBuf<isdf::VgView> d_views;
    isdf::DevBuf<long long> d_rows;
    isdf::DevBuf<unsigned> d_seen;
    isdf::DevBuf<uint16_t> d_zero;
    isdf::PinBuf<int64_t> h_rows;
    isdf::DevEvents<2> ev;
    int ready(isdf_ctx *c) { return ev.ready(c); }
};

namespace isdf {

// what the device and the host forms check and set up alike (c may be null: the host form)
int gain_setup(isdf_ctx *c, const isdf_depth_camera *cam, const void *poses, long long n_views, const isdf_view_gain_params *params, const void *rows, const MapGeom &M,
               isdf_view_gain_params &P, DcRays &base);

// the launches on st: the table, then per chunk the clear of its seen grids and the gain kernel; with want_info the rows' pinned copy too
int gain_run(isdf_ctx *c, ViewGainState *S, const DcRays &base, const MapGeom &M, const isdf_view_gain_params &P, const double *d_poses, long long n_views,
             long long *d_rows, bool want_info, int *chunks_out, hipStream_t st);

}  // namespace isdf
