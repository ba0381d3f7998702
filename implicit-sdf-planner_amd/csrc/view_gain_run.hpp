// What another query needs to score poses with the view gain (host-only): the state of view_gain.hip and the declarations of its
// checks and of its launches.  view_gain.hip defines them; view_cand.hip scores its dense pose table through them, view_select.hip its
// pose list - and takes each chunk's seen grids before the next chunk clears them.
#pragma once
#include "map_query.hpp"
#include "view_gain_host.hpp"
#include <functional>

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

// after a chunk's gain kernel, on the same stream: views view0 .. view0 + n - 1, whose seen grids (n_words each, one after the other)
// are live until the call returns - the seen grid of a scored view is its set of unknown voxels, that of any other is all zero
using GainChunkHook = std::function<int(long long view0, long long n, const unsigned *d_seen, long long n_words)>;

// the launches on st: the table, then per chunk the clear of its seen grids and the gain kernel (and after_chunk, where one is given); with
// want_info the rows' pinned copy too
int gain_run(isdf_ctx *c, ViewGainState *S, const DcRays &base, const MapGeom &M, const isdf_view_gain_params &P, const double *d_poses, long long n_views,
             long long *d_rows, bool want_info, int *chunks_out, hipStream_t st, const GainChunkHook *after_chunk = nullptr);

}  // namespace isdf
