// Private host-side context of the C ABI (not installed; include/isdf_accel.h keeps isdf_ctx opaque).
#pragma once
#include "isdf_internal.hpp"
#include "dev_buf.hpp"
#include "ctx_state.hpp"
#include "minco_host.hpp"
#include "midend_host.hpp"
#include <chrono>
#include <cstdlib>
#include <string>
#include <vector>

using namespace isdf;

using ProfEvent = DevEvents<4>;                 // start/stop of the dominant kernel, start/stop of the one after it
struct isdf_xchg;
struct SweptMeshState;          // swept_mesh.hip: scratch of the swept-volume field query and the last mesh
struct TrajCheckState;          // swept_field.hpp: the last clearance check's points below the margin
void traj_watch_disarm(isdf_ctx *c);                  // traj_watch.hip: the kept report is no longer folded across map updates (a new shape)
struct TrajLimitsState;         // traj_limits.hip: scratch of the dynamic-limits report and the state sampler
// traj_limits.hip, for callers that hold B trajectories on the device already: the report's two launches on `st` and nothing else (no
// event, copy or synchronisation; d_piece: B N x 12, d_info: B x ISDF_TL_INFO_WORDS doubles), and a trajectory's words -> its info
constexpr int ISDF_TL_INFO_WORDS = 4 * ISDF_LIMITS_CHANNELS;     // per channel: value, time, piece, pieces over the limit
int isdf_traj_limits_launch(isdf_ctx *c, int B, int N, const double *d_T, const double *d_C, const isdf_traj_limits_params *p, double *d_piece,
                            double *d_info, hipStream_t st);
void isdf_traj_limits_unpack(const isdf_config &cfg, const isdf_traj_limits_params *p, const double *words, isdf_traj_limits_info *info);
struct TrajRetimeState;         // traj_retime.hip: scratch of the retiming (ladder copies, piece rows, reports, search state)
struct TrajReallocState;        // traj_realloc.hip: scratch of the per-piece re-allocation (iterate, piece rows, reports, state)
struct MapUpdateState;          // map_change.hpp: scratch of the in-place map changes (input, new-voxel list, hand-over record, table staging)
struct MapRaycastState;         // map_raycast.hip: staging of the host-pointer ray cast, the counters' record and its pinned copy
struct DepthCamState;           // depth_cam.hip: staging of the depth camera's host-pointer forms, the counters' record and its pinned copy
struct ViewGainState;           // view_gain.hip: the view gain's poses, per-view table, rows, seen grids and zero image
struct FrontierClusterState;    // frontier_cluster.hip: the clusters' union-find, numbering and row scratch, the record and the pinned outputs
struct ViewCandState;           // view_cand.hip: the candidate views' rows, poses, dense table, targets' rows, the record and the pinned outputs
struct ViewSelectState;         // view_select.hip: the view selection's rows, per-view lists of set words, marginals, claimed grid, the record and the pinned outputs
int isdf_traj_check_ready(isdf_ctx *c);             // traj_check.hip: what isdf_traj_check needs of the ctx (shape, occupancy grid), or the error

// frontend_field.hip: the record of one in-place change of the cost-to-go field (voxels closed: the repair; opened: the reopen),
// one 64-byte line, uploaded empty before the change's kernels and read back after them
struct FfRecord {
    unsigned long long tau_bits;            // closing: the least finite d of a closed voxel, as its bits (+inf: none)
    unsigned long long changed;             // voxels closed / opened
    unsigned long long changed_reached;     // closing: of them, those that held a finite d
    unsigned long long premise_violated;    // a bit moved against the direction: the host drops the field
    unsigned long long reset, seeded;       // closing: voxels reset by the threshold, bricks that reset one
    unsigned long long goal_opened;         // opening: the goal cell opened
    unsigned long long opened_reached;      // opening: opened voxels with a finite d after the rounds
};
static_assert(isdf::LAZY_NO_MEMORY == ISDF_ERR_HIP, "the slot reports a failed new as isdf_create does");
static_assert(sizeof(FfRecord) == 64, "the field change's record is one 64-byte line");
inline FfRecord ff_record_empty() {
    FfRecord r{};
    r.tau_bits = 0x7FF0000000000000ull;
    return r;
}

// map_known.hip: the record of one get / fill / frontier call, one 64-byte line, uploaded empty before the kernel and read back after it
struct MkRecord {
    unsigned long long n;                   // get: known voxels; frontier: frontier voxels
    unsigned long long newly;               // fill: bits that went from 0 to 1
    int lo[3], hi[3];                       // the index box of the counted voxels
    unsigned long long gone;                // fill: bits that went from 1 to 0
    unsigned pad[4];
};
static_assert(sizeof(MkRecord) == 64, "the known grid's record is one 64-byte line");
int map_known_reset(isdf_ctx *c);           // map_known.hip: the map was replaced - with the mode on, all unknown at the new size

// known_erode.hip, for isdf_map_known_erode and the gated cost-to-go field: ..._check: the parameters' ranges;
// ..._radius: radius -1 resolved to the front end's footprint (ISDF_ERR_STATE without one); ..._launch: the passes, bracketed by the
// state's events and followed by the record's copy, on the ctx's stream - *d_E: the eroded grid's words, which stay until the next
// launch; ..._report: after a synchronisation of the stream, the info of the last launch.
struct KnownErodeState;
namespace isdf {
int known_erode_check(isdf_ctx *c, const isdf_known_erode_params &P);
int known_erode_radius(isdf_ctx *c, const isdf_known_erode_params &P, int *radius);
int known_erode_launch(isdf_ctx *c, int radius, int border, const unsigned **d_E);
void known_erode_report(isdf_ctx *c, int radius, int border, isdf_known_erode_info *out);
}

// What the swept-volume kernels need per point set (SweptParams): the optimizer step's (the ctx holds it) or the field query's
// (SweptMeshState holds its own: the query never shares scratch with the step).  The point arrays grow together.
struct SweptScratch {
    DevBuf<double> traj_duration, coarse_t, coarse_pose, task_buf;
    DevBuf<int> n_coarse, point_nr;
    DevBuf<unsigned> task_map, point_lmask, words;
    // the optimizer step only
    DevBuf<double> point_partial; DevBuf<int> point_piece; DevBuf<unsigned long long> point_stat;
    DevBuf<unsigned> scan_ticks; DevBuf<int> scan_order;       // a step's scan records (class | rank per point) / the dispatch order of the NEXT step's scan built from them
    size_t points = 0;
    // *regrown: the point arrays are new (and zeroed where the kernels count on it)
    int reserve(isdf_ctx *c, size_t n_points, bool with_step_arrays, bool *regrown = nullptr);
    void bind(SweptParams &P) const;          // every pointer above and max_coarse (not stats: the step's are the ctx's)
};

struct isdf_ctx {
    isdf_config cfg;
    int device = 0;
    std::string err;
    // grid
    DevGrid grid{};
    DevBuf<float> d_esdf;
    int mesh_info[16] = {0};                    // isdf_mesh_info: what isdf_set_shape found and decided about the installed mesh
    double mesh_rmax = 0.0;                     // mesh robots: largest body-frame vertex norm (the swept mesh's box margin)
    Lazy<SweptMeshState> swm;                   // isdf_swept_sdf / isdf_swept_mesh_*: own scratch, never the V1 step's
    Lazy<TrajCheckState> tck;                   // isdf_traj_check*: the kept report rows
    Lazy<TrajLimitsState> tlm;                  // isdf_traj_limits* / isdf_traj_sample*: own scratch (grows only)
    Lazy<TrajRetimeState> trt;                  // isdf_traj_retime*: own scratch (grows only)
    Lazy<TrajReallocState> tra;                 // isdf_traj_realloc*: own scratch (grows only)
    const double *v1_tstar_stage = nullptr;     // set by the host-direct V1 step for ONE eval_device_impl call (SweptParams::tstar_stage)
    DevBuf<double> d_esdf_stage;        // isdf_esdf_sample's staging (points | values | gradients): grows only, no allocation per call
    DevBuf<float> d_esdf_bricks; bool bricks_stale = true;     // the ESDF as 2 x 2 x 2-cell bricks with apron, one 128-byte line each (map_build.hip: scattered points)
    DevBuf<uint8_t> d_occ;                      // (allocated as whole dwords: the map update marks a voxel with a 32-bit atomic)
    // isdf_set_pointcloud's points per voxel and its sta_threshold, kept for isdf_update_pointcloud; gone after isdf_set_grid and after
    // an isdf_update_voxels that occupied a voxel (the counts no longer describe the occupancy)
    DevBuf<unsigned> d_counts; int counts_thr = 0;
    Lazy<MapUpdateState> mup;                   // isdf_update_pointcloud / isdf_update_voxels: own scratch (grows only)
    Lazy<MapRaycastState> mrc;                  // isdf_map_raycast*: own scratch (grows only)
    Lazy<DepthCamState> dcm;                    // isdf_depth_render* / isdf_depth_rays* / isdf_integrate_depth: own scratch (grows only)
    Lazy<ViewGainState> vgn;                    // isdf_view_gain*: own scratch (grows only)
    Lazy<FrontierClusterState> fcl;             // isdf_map_frontier_clusters: own scratch (grows only)
    Lazy<ViewCandState> vcd;                    // isdf_view_candidates: own scratch (grows only); it scores through vgn's
    Lazy<ViewSelectState> vsl;                  // isdf_view_select: own scratch (grows only); it scores through vgn's
    Lazy<KnownErodeState> ker;                  // isdf_map_known_erode / isdf_frontend_field_build_known: own scratch (grows only)
    DevBuf<unsigned> d_bits; bool bits_dirty = true;
    // the known grid (map_known.hip): one bit per voxel, 1 = some ray has visited it or the caller declared it known.  `on`
    // outlives maps (isdf_map_known_enable); d_bits holds n_words dwords while `have`; d_shift is where a window shift writes before the
    // two change places.  Everything else is scratch of isdf_map_known_get / _fill / isdf_map_frontier; all of it grows only.
    struct Known {
        bool on = false, have = false;
        size_t n_words = 0;
        DevBuf<unsigned> d_bits, d_shift;
        long long newly = 0, merges = 0;            // isdf_map_known_info's newly_known and merges
        DevBuf<unsigned> d_front; DevBuf<int> d_cnt, d_base; DevBuf<long long> d_list; DevBuf<unsigned char> d_scan_tmp;
        RecPair<MkRecord> rec; DevEvents<2> ev;
        // isdf_map_known_merge_ms: a developer's pair of events round the merge kernel, recorded only while asked for
        bool time_merge = false; DevEvents<2> ev_merge; double merge_ms = -1.0;
    } known;
    bool have_geom = false;
    unsigned long long grid_epoch = 0;          // counts isdf_set_grid / isdf_set_pointcloud: what was derived from voxel indices of an older grid is stale
    // shape
    DevShape shape{};
    isdf_shape shape_host{};
    bool have_shape = false;
    DevBuf<DevMesh> d_mesh; int mesh_depth = 0;     // levels of the mesh robot's hierarchy
    DevBuf<double> d_mesh_tri;
    DevBuf<float> d_mesh_trif;
    DevBuf<int> d_fwn_child;
    DevBuf<float> d_fwn_box, d_fwn_boxq;
    DevBuf<double> d_fwn_triq;
    DevBuf<int> d_mesh_flat;             // the flat slot table of a small mesh (DevMesh::flat)
    DevBuf<float> d_mesh_dl;             // the mesh kind's distance lattice (DevMesh::dl)
    DevBuf<double> d_shape_grid;         // ISDF_SHAPE_GRID: the sampled lattice
    DevBuf<isdf_shape_instr> d_shape_prog;       // ISDF_SHAPE_PROGRAM: the lowered instruction list (DevShape::prog)
    DevBuf<void> d_pose;                 // pose records of a non-fused integral step (bytes)
    // points (V1)
    DevBuf<double> d_points;
    int M = 0;
    DevBuf<double> d_tstar;          // internal lastTstar when the caller passes none
    DevBuf<unsigned> d_merge_bits;   // isdf_points_merge_check: one bit per voxel, set where a point of the set lies (grows only)
    // shard
    int rank = 0, world = 1;
    // per-step scratch
    DevBuf<double> d_acc; DevBuf<int> d_sample_info;      // result slots (ACC_STRIDE per sample, created all-ones) / 2 ints per sample
    SweepParams last_P{}; bool have_last_P = false;
    double last_exact_ms = 0.0;
    DevBuf<double> d_piece_cost;
    DevBuf<double> d_in;            // host-API staging: T | coeffs
    DevBuf<double> d_out;
    std::vector<double> h_out;
    DevBuf<unsigned long long> d_stats;
    isdf_stats last_stats{};
    bool stats_cached = false;
    // V1 scratch
    SweptScratch v1;
    long long scan_order_b = -1, scan_order_e = -1; unsigned long long scan_order_epoch = 0, points_epoch = 1;   // the shard of which points v1.scan_order is for
    DevBuf<double> d_hist;
    // profiling
    bool fuse_small = true;     // developer switch ISDF_NO_FUSE=1: always sweep + tail as two launches
    // developer / fallback switches, ALL read once per ctx in isdf_create (so a process can hold ctxs of either kind):
    // ISDF_NO_HOST_DIRECT=1 (isdf_eval and the callback take the copy path), ISDF_NO_BAR_WRITES=1 (host-direct steps fetch their
    // inputs from host-mapped memory instead of receiving them through the PCIe BAR), ISDF_NO_LPT=1 (plain dispatch order)
    bool env_no_direct = false, env_no_bar = false, env_no_lpt = false;
    int last_host_path = 0;     // isdf_host_path(): how the last host-array step crossed PCIe
    bool prof_on = false, prof_secondary = false; int prof_every = 1; long long prof_tick = 0;
    std::vector<ProfEvent> prof_events;
    size_t prof_used = 0;
    hipStream_t stream = nullptr;   // stream of the host API
    DevBuf<int> d_sample_map; size_t sample_map_n = 0;      // developer override of the tile sweep's dispatch order
    // longest-first order of fused single-launch steps: two generations of work classes and of orders, the geometry they belong to
    DevBuf<unsigned char> d_plan_cls; DevBuf<int> d_plan_map; DevBuf<unsigned short> d_plan_lr, d_plan_hist;
    long long plan_ns = -1, plan_geo = -1; int plan_nb = -1; int plan_k = 0; int plan_cur = 0; int n_cus = 0;
    size_t plan_ns_cap = 0, plan_np_cap = 0;        // samples / pieces per generation (the buffers hold two)
    DevBuf<unsigned long long> d_dbg; size_t dbg_used = 0;   // ISDF_DEBUG_TIMING=1 (developer tool)
    // full objective callback (costFunctionLmbm): MINCO on the host, sweeps on the device
    isdf_host::MincoS3 minco; bool have_traj = false; double rho = 0.0;
    std::vector<double> cb_T, cb_gdC, cb_gdT, cb_gradP, cb_gradT;
    PinBuf<double> h_eval_pin;      // pinned staging of isdf_eval: [inputs | outputs | statistics]
    // multi-device ctx, isdf_eval: the sum kernel writes the step's outputs, the statistics words and a completion word straight
    // into the pinned buffer (no download commands, no stream synchronisation: the calling thread spins on the word)
    double *mh_out = nullptr; unsigned long long *mh_words = nullptr; unsigned long long mh_seq = 0; DevBuf<unsigned> d_msum_blocks;
    bool env_multi_no_hostout = false;
    PinBuf<double> h_pin;           // pinned staging: [T | coeffs | out_a | out_b]
    DevBuf<double> d_cb;            // device twin of the staging buffer
    // host-direct steps (isdf_eval / isdf_cost_function on one GPU when the step is one fused launch): pinned, device-mapped
    // [inputs | outputs | one flag per trajectory]; the launch reads the inputs and writes the outputs over PCIe itself
    PinBuf<double> h_dir; size_t dir_in = 0, dir_out = 0, dir_flags = 0;
    DevBuf<double> d_stage;
    DevBuf<unsigned long long> d_stage_flags;
    unsigned long long dir_seq = 0;
    unsigned long long host_steps = 0, host_late = 0, host_late_spins = 0, host_late_mark = 0;      // isdf_host_info: host-mapped result hand-overs / those whose rows landed after the flag
    int bar_state = 0;          // 0: untested, 1: the host can write device memory through the PCIe BAR (verified), -1: it cannot
    bool dir_pending = false; int dir_nb = 0, dir_n = 0; bool cb_direct = false;
    PinBuf<double> h_v1_pin;     // host-direct swept-volume step: [out | statistics | flag | lastTstar], device-mapped
    double last_parts[4] = {0, 0, 0, 0};
    std::vector<double> cb_x; double cb_energy = 0.0; int cb_n_out = 1; bool cb_pending = false;
    // device half of the callback (csrc/minco_dev.hip): MINCO, energy, adjoint and chain rule in two small kernels either side
    // of the sweeps - a callback moves n doubles down and n + 5 up.  minco_mode 0: wherever it is faster (callback.hip
    // cb_device_minco), 1 (ISDF_HOST_MINCO=1): the host's band LU, bitwise the reference's elimination order, 2
    // (ISDF_DEVICE_MINCO=1): on the device whenever N <= CB_MAX_N
    int minco_mode = 0; int last_minco_path = 0;          // last_minco_path: 1 = the last callback ran MINCO on the device
    DevBuf<double> d_cbdev;         // [x | ends(18) | u | energy block]
    PinBuf<double> h_cbres;         // pinned, device-mapped: [x staging | cost, g, parts | flag]
    unsigned long long cb_seq = 0; bool cb_dev = false, cb_post_queued = false; bool cb_ends_dirty = true;
    double cb_ends[18] = {0};
    // mid end (csrc/midend.hip): the host form's state; the device form's scratch [x | ends | ref | T | coeffs | u | energy block |
    // penalty block] per trajectory and its pinned, device-mapped hand-over [inputs | cost, g, parts | one flag per trajectory]
    isdf_host::Midend mid_host;
    DevBuf<double> d_mid; PinBuf<double> h_mid; unsigned long long mid_seq = 0;
    // front end (csrc/frontend.hip): attitude kernels of the robot, inflated bit-packed occupancy, breadth-first order tables
    struct FrontEnd {
        isdf_frontend_config cfg{}; int xk = 0, yk = 0; double margin = 0.0; bool built = false;
        DevBuf<unsigned> d_rows, d_bits; DevBuf<double> d_rot;
        DevBuf<unsigned short> d_seq; DevBuf<int> d_seq_len; int seq_stride = 0;
        DevBuf<void> d_row_list; DevBuf<int> d_row_ptr; int n_row_list = 0;             // non-empty rows per attitude
        DevBuf<unsigned> d_cspace;                                                       // 4 dwords per voxel
        // the A* (isdf_frontend_astar_search): the table on the host, the breadth-first attitude orders, the last path
        unsigned *h_cspace = nullptr; bool h_cspace_valid = false, h_cspace_pinned = false;   // pinned when the host lets us (16 B per voxel), else pageable
        std::vector<unsigned short> h_seq; std::vector<int> h_seq_len;
        std::vector<double> path_xyz, path_rp;
        // the cost-to-go field (frontend_field.hip): d per voxel, free bits (one 64-bit word per 64 z), the active-brick list, the
        // [next round's flags | bricks seen], the counters and their pinned copy; all grow only, a new isdf_frontend_build drops them
        DevBuf<double> d_field; DevBuf<unsigned long long> d_field_free; DevBuf<int> d_field_list; DevBuf<unsigned> d_field_flags;
        DevBuf<unsigned long long> d_field_cnt; PinBuf<unsigned long long> h_field_cnt;
        bool field_valid = false, field_reachable = false; int field_goal[3] = {-1, -1, -1};
        // what an in-place change (the repair after a map update, the reopen after a clear) needs of the last build: its status and
        // round bound, the counts of free and of reached voxels as the last build / repair / reopen left them; the change's record on
        // the device and its pinned copy (uploaded empty, read back as the kernels left it); the opening direction's opened bits of the changed
        // box, one word per wavefront of the mark kernel
        int field_status = 0, field_max_rounds = 0; long long field_free_voxels = 0, field_reached_voxels = 0;
        RecPair<FfRecord> field_rep;
        DevBuf<unsigned long long> d_field_open;
        // the last repair's and the last reopen's report (field_repaired, field_reopened: there was one since the build)
        bool field_repaired = false; isdf_field_repair_info field_repair{};
        bool field_reopened = false; isdf_field_reopen_info field_reopen{};
        // the field carried through a shift of the map window: where the translated d and free bits are written; each
        // then changes places with d_field / d_field_free (one more copy of both stays allocated); the last carry's report
        DevBuf<double> d_field_shift; DevBuf<unsigned long long> d_field_free_shift;
        bool field_shifted = false; isdf_field_shift_info field_shift{};
        // the field gated by the eroded known grid (isdf_frontend_field_build_known): its free words carry free & E, so
        // whatever can change K or the map drops it (isdf_field_known_changed)
        bool field_gated = false; int field_gate_radius = 0, field_gate_border = 0;
        // ... unless it follows the change (isdf_frontend_field_set_known_follow): the report of the last followed call, which
        // its stages add to (follow_fresh: the next stage starts a new report), and the last stage's erosion info
        bool field_followed = false, follow_fresh = true; isdf_field_follow_info field_follow{};
    } fe;
    int field_repair_mode = 0;                  // isdf_frontend_field_set_repair: outlives isdf_frontend_build (fe is reset by it)
    int field_reopen_mode = 0;                  // isdf_frontend_field_set_reopen: likewise
    int field_shift_mode = 0;                   // isdf_frontend_field_set_shift: likewise
    int field_known_follow_mode = 0;            // isdf_frontend_field_set_known_follow: likewise
    bool gate_dropped = false;                  // map_change_ready dropped a gated field: the in-place change under way reports field_dropped = 1
    int traj_watch_mode = 0;                    // isdf_traj_check_set_watch: outlives the check (the watch itself: TrajCheckState::w)
    struct isdf_xchg *xchg = nullptr;           // peer-to-peer exchange of the multi-GPU path (csrc/xchg.hip)
    isdf_progress_fn progress = nullptr;        // isdf_set_progress: the optimizer drivers' progress / cancel hook
    void *progress_instance = nullptr;
    size_t progress_stride = 0;                 // batch: trajectory t's hook gets (char *)progress_instance + t * stride
    double xchg_timeout_ms = 2000.0;             // bound of the exchange's waits (isdf_xchg_set_timeout_ms), device wall clock
    // ONE host process driving SEVERAL devices (isdf_create_multi): this ctx is the lead (shard 0 of n on devices[0]) and owns
    // one plain ctx per further device (shard r of n).  Once-per-plan state set on the lead is replicated; a step launches every
    // shard on its own device's stream from the calling thread and sums the shards' packed outputs on the lead (one kernel
    // reading the peers' buffers over xGMI in rank order, or RCCL's all-reduce) - SURVEY 8(b) "Threading".
    std::vector<isdf_ctx *> peers;
    bool is_peer = false;                       // owned by a lead: not handed to the caller
    DevEvents<1> mev_in, mev_done;                        // lead: inputs ready on the caller's stream / the step's sum has run; peer: shard finished
    // mesh robots on the tile sweep: the queue of 64-voxel blocks between the scan launch and the exact launch
    DevBuf<unsigned> d_mq_entries, d_mq_count;
    DevBuf<int2> d_mq_items;
    DevBuf<double> d_mq_res;
    DevBuf<int> d_mq_sample_items, d_mq_sample_n;
    size_t mq_cap = 0, mq_samples_cap = 0;      // blocks / samples the queue was sized for ...
    int mq_kmax = 0;                            // ... and the blocks per sample (a change of it resizes the queue too)
    bool multi_pull = false;                              // lead: the peers read the lead's inputs in place (peer access both ways)
    bool msum_recorded = false;                           // lead: mev_done has been recorded at least once
    int multi_collective = 0;                   // ISDF_MULTI_*: how the shards' outputs are summed
    void *rccl_lib = nullptr; void *rccl_comm = nullptr;  // RCCL by dlopen (only when asked for): this device's communicator
    DevBuf<double> d_mpart;         // every shard of a multi-device step writes [packed outputs | 8 statistics as doubles] here
    DevBuf<double> d_mstage;        // lead, staged mode: the peers' parts copied next to each other
    // every buffer, event and lazily created state above frees itself (isdf_destroy makes the device current)
};
namespace isdf { struct XFuse; }
// xchg.hip: fills the in-kernel exchange block of a fused step when isdf_xchg_fuse is on (returns false: not requested;
// *err != ISDF_OK: requested but impossible for this launch)
bool isdf_xchg_fill(isdf_ctx *c, isdf::XFuse *xf, size_t pieces, int *err);
bool isdf_xchg_fuse_on(const isdf_ctx *c);     // isdf_xchg_fuse(ctx, 1) is in force
int isdf_reserve_sweep_buffers(isdf_ctx *c, long long total_pieces);   // isdf_host.hip: scratch of the integral sweep (grows only)
void isdf_xchg_reset_board(isdf_ctx *c);  // xchg.hip: empties this rank's board again (after an overflow)
int isdf_reset_result_slots(isdf_ctx *c); // isdf_host.hip: drains the device and empties every self-resetting slot again (after an overflow)
void isdf_xchg_release(isdf_ctx *c);          // xchg.hip: closes the peer mappings, frees the mailbox (isdf_destroy)
void isdf_frontend_release(isdf_ctx *c);      // frontend.hip: drops the tables (a new grid or shape)
namespace isdf {
// map_known.hip: the frontier stage of isdf_map_frontier and isdf_map_frontier_clusters - the set's words (the frontier, or the caller's
// set_bits) into known.d_front, their record handed over, and with want_list the scan into known.d_base and the list into known.d_list
int map_frontier_stage(isdf_ctx *c, const char *op, const uint32_t *set_bits, uint32_t *bits_out, bool want_list, long long capacity, const hipEvent_t *list_ev,
                       MkRecord *rec_out, bool *counted);
}
int isdf_mesh_lattice_build(isdf_ctx *c, isdf::DevMesh *hm, const double lo[3], const double hi[3], int n, float s_range_out[2]);      // shape_eval.hip: the mesh kind's distance lattice (DevMesh::dl)
int isdf_mesh_surface_valid(isdf_ctx *c, const double *d_tri, int nF, double extent, double tau_limit, int *valid_out, float defect_out[2]);      // shape_eval.hip: exact winding number 0 / 1 on both sides of every face

// every setter of once-per-plan state ends with this: the same call on every owned peer ctx (isdf_create_multi)
#define ISDF_REPLICATE(ctx, call)                                                                  \
    do {                                                                                           \
        for (isdf_ctx *p_ : (ctx)->peers) {                                                        \
            const int r_ = (call);                                                                 \
            if (r_ != ISDF_OK) { (ctx)->err = "device " + std::to_string(p_->device) + ": " + p_->err; return r_; } \
        }                                                                                          \
    } while (0)

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return ISDF_ERR_HIP;                                                                   \
        }                                                                                          \
    } while (0)

// the int-returning twin: a step that failed has recorded its message already, its code is handed on
#define ISDF_TRY(expr)                                                                             \
    do {                                                                                           \
        const int rc_ = (expr);                                                                    \
        if (rc_) return rc_;                                                                       \
    } while (0)

int isdf_fail(isdf_ctx *c, int code, const char *msg);      // records the message, returns code
void isdf_fill_flat(const isdf_config &cfg, isdf::FlatP &f);      // isdf_host.hip: the dynamics constants of a launch

// ---- shared between the host files (isdf_host.hip, shape_setup.hip, multi_dev.hip, host_step.hip, callback.hip)
inline bool env_is(const char *name, char ch) { const char *e = getenv(name); return e && e[0] == ch; }     // a one-character switch, read when called
// host-direct step: device-visible addresses of the pinned inputs / outputs / flags of this step
struct HostDirect { const double *T, *coeffs; double *out; unsigned long long *flags; unsigned long long seq; bool via_bar; };
constexpr int ISDF_DIRECT_NA = 1;        // eval_device_impl: the step cannot run host-direct (nothing was launched)
void shard_range(long long total, int rank, int world, long long &b, long long &e);     // isdf_host.hip: this rank's contiguous share [b, e)
// isdf_host.hip: one step of one device.  mode 0: the sweep cfg.variant names; 1: the swept-volume sweep; 2: the integral sweep with the collision term off
int eval_device_impl(isdf_ctx *c, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out,
                     double *d_tstar, hipStream_t st, int mode = 0, bool fixed_tstar = false, const HostDirect *hd = nullptr);
// isdf_host.hip: every sweep of the host paths goes through here (one device or several)
int sweep_dispatch(isdf_ctx *c, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out, double *d_tstar,
                   hipStream_t st, int mode = 0, bool fixed_tstar = false);
int fetch_stats(isdf_ctx *c);             // isdf_host.hip: the last launch's statistics words into last_stats (reads the sticky overflow word)
int clear_overflow(isdf_ctx *c);          // isdf_host.hip: clears the sticky overflow word, then isdf_reset_result_slots
void multi_release(isdf_ctx *c);          // multi_dev.hip: the multi-device ctx's events and communicator (isdf_destroy)
int multi_eval_device(isdf_ctx *c, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out,
                      double *d_tstar, hipStream_t st, int mode, bool fixed_tstar);      // multi_dev.hip: one step on every device, summed on the lead
int add_peer_stats(isdf_ctx *c);          // multi_dev.hip: the peers' pair statistics added to the lead's last_stats
bool direct_enabled(const isdf_ctx *c);   // host_step.hip: this ctx's small steps may run host-direct
int direct_launch(isdf_ctx *c, int nb, int n, const double *const *T, const double *const *coeffs, int first, hipStream_t st, int mode);     // host_step.hip: places the inputs, launches
int direct_wait(isdf_ctx *c, hipStream_t st, bool *overflow);      // host_step.hip: the host's side of that step's hand-over
bool bar_usable(isdf_ctx *c, double *d_buf, size_t n);             // host_step.hip: the host can write device memory through the PCIe BAR (probed once per ctx)
void host_rows_mark(double *p, size_t n);                          // host_step.hip: fills a host-mapped result area with the "not written yet" pattern
bool host_rows_wait(isdf_ctx *c, const double *p, size_t n, bool another_area_of_the_same_step = false);   // host_step.hip: waits until none of it is left
// the four counts of a step added to a running total (not the overflow word): from another isdf_stats / from a step's statistics words
static inline void stats_add(isdf_stats &t, const isdf_stats &s) {
    t.n_units += s.n_units; t.n_units_culled += s.n_units_culled; t.n_pairs += s.n_pairs; t.n_grad_pairs += s.n_grad_pairs;
}
static inline void stats_add(isdf_stats &t, const unsigned long long *w) {
    t.n_units += (int64_t)w[0]; t.n_units_culled += (int64_t)w[1]; t.n_pairs += (int64_t)w[2]; t.n_grad_pairs += (int64_t)w[3];
}

// The host's side of every hand-over through host-mapped memory (host_step.hip, callback.hip): spins until the completion word, its
// `mask` bits aside, equals seq.  Bounded: `seconds` after t0 (the clock is read every 0x4000 spins only) it drains the stream, looks
// once more and gives up.  *value: the word as last read.  The caller's acquire fence and host_rows_wait follow.
static inline bool host_flag_wait(const volatile unsigned long long *word, unsigned long long seq, unsigned long long mask,
                                  std::chrono::steady_clock::time_point t0, double seconds, hipStream_t st, unsigned long long *value) {
    for (unsigned spin = 0;; spin++) {
        *value = *word;
        if ((*value & ~mask) == seq) return true;
        if ((spin & 0x3FFFu) == 0x3FFFu && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) {
            (void)hipStreamSynchronize(st);
            *value = *word;
            return (*value & ~mask) == seq;
        }
    }
}
