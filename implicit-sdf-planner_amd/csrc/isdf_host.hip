// Host side of the C ABI (include/isdf_accel.h): context, device memory, launches.
// Replaces, for the two sweeps only, what TrajOptimizer holds around them in the reference
// (back_end_optimizer.hpp:59-62 parallel_points/lastTstar, :667-725 setParam/setEnvironment/setGridMap) and the
// shape registry lookup of sw_manager.hpp:74-123,:255-275.  No CPU compute path exists here.
#include "isdf_ctx.hpp"
#include <atomic>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include <new>

using namespace isdf;

namespace {
thread_local std::string g_create_error;
}

int isdf_fail(isdf_ctx *c, int code, const char *msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// --------------------------------------------------------------------------------------------------------------
// defaults (the analytic-shape registry: shape_setup.hip)
// --------------------------------------------------------------------------------------------------------------
extern "C" int isdf_abi_version(void) { return ISDF_ABI_VERSION; }
extern "C" size_t isdf_out_stride(int N) { return (size_t)1 + 19 * (size_t)N; }

extern "C" void isdf_config_default(isdf_config *c) {   // config_CappedCone.yaml (demo1)
    std::memset(c, 0, sizeof(*c));
    c->device = 0;
    c->variant = ISDF_V3_ESDF_TILE;
    c->kernel_size = 13;
    c->integral_intervs = 64;
    c->enable_dyn = 1;
    c->enable_pos = 1;
    c->enable_cull = 0;
    c->safety_hor = 0.866;
    c->weight_p = 4000.0;
    c->weight_v = c->weight_omg = c->weight_theta = 1000.0;
    c->vmax = 10.0; c->omgmax = 10.0; c->thetamax = 100.0;
    c->smoothing_eps = 1.0e-2;
    c->occ_thresh = 0.0;
    c->vehicle_mass = 0.61; c->grav_acc = 9.8; c->horiz_drag = 0.10; c->vert_drag = 0.10;
    c->paras_drag = 0.01; c->speed_eps = 1.0e-4;
}

// --------------------------------------------------------------------------------------------------------------
// lifetime
// --------------------------------------------------------------------------------------------------------------
extern "C" const char *isdf_last_error(const isdf_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

extern "C" int isdf_create(isdf_ctx **out, const isdf_config *cfg) {
    if (!out || !cfg) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (cfg->variant < ISDF_V1_SWEPT || cfg->variant > ISDF_V3_ESDF_TILE) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "bad variant");
    if (cfg->kernel_size < 1 || cfg->kernel_size > 512) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "kernel_size must be in [1,512]");
    if (cfg->integral_intervs < 1) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "integral_intervs must be >= 1");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return isdf_fail(nullptr, ISDF_ERR_NO_DEVICE, "no HIP device available (the product path has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "device ordinal out of range");
    isdf_ctx *c = new (std::nothrow) isdf_ctx();
    if (!c) return isdf_fail(nullptr, ISDF_ERR_HIP, "out of host memory");
    c->cfg = *cfg;
    c->device = cfg->device;
    {   // every environment switch of the host paths is read HERE, once per ctx
        auto on = [](const char *name) { return env_is(name, '1'); };
        c->fuse_small = !on("ISDF_NO_FUSE");
        c->env_no_direct = on("ISDF_NO_HOST_DIRECT");
        c->env_multi_no_hostout = on("ISDF_MULTI_NO_HOST_OUT");
        c->env_no_bar = on("ISDF_NO_BAR_WRITES");
        c->env_no_lpt = on("ISDF_NO_LPT");
        c->minco_mode = on("ISDF_HOST_MINCO") ? 1 : (on("ISDF_DEVICE_MINCO") ? 2 : 0);
    }
    if (hipSetDevice(c->device) != hipSuccess || c->d_stats.alloc(8, 0x00) != hipSuccess ||
        c->v1.traj_duration.alloc(1, 0x00) != hipSuccess || c->v1.n_coarse.alloc(1) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) {
        delete c;
        return isdf_fail(nullptr, ISDF_ERR_HIP, "device initialisation failed");
    }
    *out = c;
    return ISDF_OK;
}

extern "C" int isdf_destroy(isdf_ctx *c) {
    if (!c) return ISDF_OK;
    for (isdf_ctx *p : c->peers) { p->is_peer = false; (void)isdf_destroy(p); }
    c->peers.clear();
    (void)hipSetDevice(c->device);
    multi_release(c);
    (void)hipDeviceSynchronize();
    c->prof_events.clear();
    isdf_frontend_release(c);
    isdf_xchg_release(c);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;               // every buffer frees itself (dev_buf.hpp), with this ctx's device current
    return ISDF_OK;
}

// --------------------------------------------------------------------------------------------------------------
// once-per-plan state
// --------------------------------------------------------------------------------------------------------------
extern "C" int isdf_set_grid(isdf_ctx *c, const void *vox, int dtype, int nx, int ny, int nz, const double origin[3],
                             const double bmax[3], double res, int kind) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!vox || !origin || nx < 1 || ny < 1 || nz < 1 || !(res > 0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad grid arguments");
    if (dtype < ISDF_U8 || dtype > ISDF_F64) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad dtype");
    if (kind != ISDF_GRID_OCCUPANCY && kind != ISDF_GRID_ESDF) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad grid kind");
    HIPCHK(c, hipSetDevice(c->device));
    isdf_frontend_release(c);       // the inflated bit-packed map was built from the previous grid
    c->d_counts.release();          // a point cloud's counts describe its own occupancy only
    const size_t n = (size_t)nx * ny * nz;
    if (c->have_geom && (c->grid.X != nx || c->grid.Y != ny || c->grid.Z != nz)) {
        // new geometry: drop the other grid kind, it no longer matches
        c->d_esdf.release();
        c->d_occ.release();
    }
    c->grid.X = nx; c->grid.Y = ny; c->grid.Z = nz; c->grid.res = res;
    for (int a = 0; a < 3; a++) {
        c->grid.bmin[a] = origin[a];
        const int dim = a == 0 ? nx : (a == 1 ? ny : nz);
        c->grid.bmax[a] = bmax ? bmax[a] : origin[a] + dim * res;
    }
    c->have_geom = true;
    c->grid_epoch++;
    if (kind == ISDF_GRID_ESDF) {
        std::vector<float> tmp;
        const float *src = nullptr;
        if (dtype == ISDF_F32) src = (const float *)vox;
        else {
            tmp.resize(n);
            if (dtype == ISDF_F64) for (size_t i = 0; i < n; i++) tmp[i] = (float)((const double *)vox)[i];
            else for (size_t i = 0; i < n; i++) tmp[i] = (float)((const uint8_t *)vox)[i];
            src = tmp.data();
        }
        ISDF_TRY(c->d_esdf.renew(c, n));
        HIPCHK(c, hipMemcpy(c->d_esdf, src, n * sizeof(float), hipMemcpyHostToDevice));
    } else {
        std::vector<uint8_t> tmp(n);
        if (dtype == ISDF_U8) for (size_t i = 0; i < n; i++) tmp[i] = ((const uint8_t *)vox)[i] != 0;
        else if (dtype == ISDF_F32) for (size_t i = 0; i < n; i++) tmp[i] = ((const float *)vox)[i] != 0;
        else for (size_t i = 0; i < n; i++) tmp[i] = ((const double *)vox)[i] != 0;
        ISDF_TRY(c->d_occ.renew(c, (n + 3) & ~(size_t)3));
        HIPCHK(c, hipMemcpy(c->d_occ, tmp.data(), n, hipMemcpyHostToDevice));
    }
    c->grid.esdf = c->d_esdf;
    c->bricks_stale = true;
    c->grid.occ = c->d_occ;
    c->bits_dirty = true;
    if (int rc = map_known_reset(c)) return rc;         // a new map: nothing of it has been seen
    ISDF_REPLICATE(c, isdf_set_grid(p_, vox, dtype, nx, ny, nz, origin, bmax, res, kind));
    return ISDF_OK;
}

extern "C" int isdf_set_points(isdf_ctx *c, const double *xyz, int M) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (M < 0 || (M > 0 && !xyz)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad points");
    HIPCHK(c, hipSetDevice(c->device));
    c->d_points.release();
    c->d_tstar.release();
    c->M = M;
    c->points_epoch++;
    if (c->v1.words) HIPCHK(c, hipMemset(c->v1.words, 0, 8 * sizeof(unsigned)));
    if (M > 0) {
        HIPCHK(c, c->d_points.alloc((size_t)3 * M));
        HIPCHK(c, hipMemcpy(c->d_points, xyz, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(c, c->d_tstar.alloc((size_t)M, 0x00));   // lastTstar starts at 0 (plan_manager.cpp:254)
    }
    ISDF_REPLICATE(c, isdf_set_points(p_, xyz, M));
    return ISDF_OK;
}

extern "C" int isdf_set_shard(isdf_ctx *c, int rank, int world) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (world < 1 || rank < 0 || rank >= world) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad shard");
    if (!c->peers.empty() || c->is_peer) return isdf_fail(c, ISDF_ERR_STATE, "a multi-device ctx (isdf_create_multi) shards by itself");
    c->rank = rank; c->world = world;
    return ISDF_OK;
}

// --------------------------------------------------------------------------------------------------------------
// per-step evaluation
// --------------------------------------------------------------------------------------------------------------
void shard_range(long long total, int rank, int world, long long &b, long long &e) {
    const long long q = total / world, r = total % world;
    b = rank * q + (rank < r ? rank : r);
    e = b + q + (rank < r ? 1 : 0);
}

int isdf_hip_fail(isdf_ctx *c, const char *what, hipError_t e) {
    if (c) c->err = std::string(what) + ": " + hipGetErrorString(e);
    return ISDF_ERR_HIP;
}
extern "C" void isdf_debug_live_bytes(long long out[2]) {
    if (!out) return;
    for (int k = 0; k < 2; k++) out[k] = isdf::g_live_bytes[k].load(std::memory_order_relaxed);
}
extern "C" long long isdf_debug_live_events(void) { return isdf::g_live_events.load(std::memory_order_relaxed); }

void isdf_fill_flat(const isdf_config &cfg, FlatP &f) {
    f.mass = cfg.vehicle_mass; f.grav = cfg.grav_acc; f.dh = cfg.horiz_drag; f.dv = cfg.vert_drag;
    f.cp = cfg.paras_drag; f.veps = cfg.speed_eps; f.dh_over_m = f.dh / f.mass;
}

static int prof_begin(isdf_ctx *c, hipStream_t st, ProfEvent **ev) {
    *ev = nullptr;
    if (!c->prof_on) return ISDF_OK;
    if ((c->prof_tick++ % c->prof_every) != 0) return ISDF_OK;
    if (c->prof_used == c->prof_events.size()) {
        ProfEvent p;
        ISDF_TRY(p.ready(c));
        c->prof_events.push_back(std::move(p));
    }
    *ev = &c->prof_events[c->prof_used++];
    return ISDF_OK;
}

// scratch of the integral sweep for `total_pieces` pieces per launch (grows only; the batched optimizer reserves its largest
// round up front so that no round reallocates while another is in flight)
int isdf_reserve_sweep_buffers(isdf_ctx *c, long long total_pieces) {
    const size_t n_samples = (size_t)total_pieces * (c->cfg.integral_intervs + 1);
    // result slots are created EMPTY (all-ones, tile_sweep.hip SLOT_EMPTY); every step leaves them empty again
    if (c->d_acc.capacity() < n_samples * ACC_STRIDE) {
        int rc = c->d_acc.reserve(c, n_samples * ACC_STRIDE, 0xFF);
        if (!rc) rc = c->d_sample_info.reserve(c, n_samples * 2);
        if (rc) { c->d_acc.release(); return rc; }
        HIPCHK(c, hipDeviceSynchronize());
    }
    if (c->d_piece_cost.capacity() < (size_t)total_pieces) {         // piece-cost slots: created EMPTY like the collision sums' slots
        ISDF_TRY(c->d_piece_cost.reserve(c, (size_t)total_pieces, 0xFF));
        HIPCHK(c, hipDeviceSynchronize());
    }
    return ISDF_OK;
}

// The result slots empty themselves only when their single consumer takes them.  Once a bounded wait has expired (overflow
// word, NaN cost) a producer may still publish late into a slot nobody takes any more, and the NEXT step would consume that
// stale value without any flag being raised.  Whoever sees the overflow word calls this: drain, then every slot empty again.
int isdf_reset_result_slots(isdf_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (c->d_acc) HIPCHK(c, hipMemset(c->d_acc, 0xFF, c->d_acc.capacity() * sizeof(double)));
    if (c->d_piece_cost) HIPCHK(c, hipMemset(c->d_piece_cost, 0xFF, c->d_piece_cost.capacity() * sizeof(double)));
    isdf_xchg_reset_board(c);
    HIPCHK(c, hipDeviceSynchronize());
    for (isdf_ctx *p : c->peers) {                  // a multi-device ctx: the peers' sticky overflow words and slots as well
        const int rc = isdf_reset_result_slots(p);
        if (rc) { c->err = p->err; return rc; }
        HIPCHK(c, hipMemset(p->d_stats + 4, 0, sizeof(unsigned long long)));
    }
    if (!c->peers.empty()) HIPCHK(c, hipSetDevice(c->device));
    return ISDF_OK;
}
// what everyone who has read the sticky overflow word does next
int clear_overflow(isdf_ctx *c) {
    HIPCHK(c, hipMemset(c->d_stats + 4, 0, sizeof(unsigned long long)));
    return isdf_reset_result_slots(c);
}

// staging of a host-direct step that fetches its inputs from host-mapped memory
static int ensure_stage(isdf_ctx *c, size_t total_pieces) {
    const size_t n_groups = (total_pieces + STAGE_G - 1) / STAGE_G;
    const int rc = c->d_stage.reserve(c, total_pieces * 19);
    return rc ? rc : c->d_stage_flags.reserve(c, n_groups, 0x00);
}

// ISDF_DEBUG_TIMING=1 (developer tool): `need` zeroed words for this step's launches; *out stays null when the switch is off
static int debug_timing_buffer(isdf_ctx *c, size_t need, hipStream_t st, unsigned long long **out) {
    if (!env_is("ISDF_DEBUG_TIMING", '1')) return ISDF_OK;
    ISDF_TRY(c->d_dbg.reserve(c, need));
    HIPCHK(c, hipMemsetAsync(c->d_dbg, 0, need * sizeof(unsigned long long), st));
    c->dbg_used = need;
    *out = c->d_dbg;
    return ISDF_OK;
}

int SweptScratch::reserve(isdf_ctx *c, size_t n_points, bool with_step_arrays, bool *regrown) {
    if (regrown) *regrown = false;
    if (!traj_duration) HIPCHK(c, traj_duration.alloc(1, 0x00));
    if (!n_coarse) HIPCHK(c, n_coarse.alloc(1));
    if (!coarse_t) {
        HIPCHK(c, coarse_t.alloc((size_t)SWEPT_MAX_COARSE));
        HIPCHK(c, coarse_pose.alloc((size_t)SWEPT_MAX_COARSE * 12));
    }
    if (points >= n_points) return ISDF_OK;
    points = 0;                                    // the whole group grows together
    if (with_step_arrays) {
        HIPCHK(c, point_partial.alloc(n_points * PARTIAL_STRIDE));
        HIPCHK(c, point_piece.alloc(n_points));
        HIPCHK(c, point_stat.alloc(n_points));
        HIPCHK(c, scan_ticks.alloc(n_points, 0x00));
        HIPCHK(c, scan_order.alloc(n_points));
    }
    HIPCHK(c, point_nr.alloc(n_points, 0x00));       // "scan passes last step": none yet
    HIPCHK(c, task_buf.alloc(n_points * SWEPT_MAX_RANGES * SWEPT_TASK_STRIDE));
    HIPCHK(c, task_map.alloc(n_points * SWEPT_MAX_RANGES));
    HIPCHK(c, point_lmask.alloc(n_points, 0x00));
    if (!words) HIPCHK(c, words.alloc(SWEPT_WORDS));
    HIPCHK(c, hipMemset(words, 0, SWEPT_WORDS * sizeof(unsigned)));
    points = n_points;
    if (regrown) *regrown = true;
    return ISDF_OK;
}
void SweptScratch::bind(SweptParams &P) const {
    P.traj_duration = traj_duration;
    P.coarse_t = coarse_t; P.coarse_pose = coarse_pose; P.n_coarse = n_coarse; P.max_coarse = SWEPT_MAX_COARSE;
    P.point_partial = point_partial; P.point_piece = point_piece; P.point_stat = point_stat;
    P.point_nr = point_nr; P.task_buf = task_buf; P.task_map = task_map; P.words = words; P.point_lmask = point_lmask;
}

// the swept-volume step (V1): prepare, sweep, back-prop + sums - or, the minimisers given, the fixed kernel and the sums
static int v1_step(isdf_ctx *c, const isdf_config &cfg, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out,
                   double *d_tstar, hipStream_t st, bool fixed_tstar) {
    if (n_traj != 1) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "the swept-volume sweep takes one trajectory");
    if (isdf_xchg_fuse_on(c)) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "the in-kernel exchange belongs to the integral sweep (V2/V3)");
    if (c->M <= 0) {                 // no obstacle points: nothing to add
        HIPCHK(c, hipMemsetAsync(d_out, 0, (size_t)n_traj * isdf_out_stride(N) * sizeof(double), st));
        HIPCHK(c, hipMemsetAsync(c->d_stats, 0, 8 * sizeof(unsigned long long), st));
        return ISDF_OK;
    }
    // (no clearing here: the prepare / fixed kernel zeroes the statistics words and the reduction writes every output)
    long long b, e;
    shard_range(c->M, c->rank, c->world, b, e);
    SweptParams P{};
    P.shape = c->shape;
    isdf_fill_flat(cfg, P.flat);
    P.N = N; P.M = c->M; P.point_begin = (int)b; P.point_end = (int)e;
    P.safety_hor = cfg.safety_hor; P.weight_p = cfg.weight_p;
    P.T = d_T; P.coeffs = d_coeffs; P.points = c->d_points;
    P.tstar = (d_tstar && !fixed_tstar) ? d_tstar : c->d_tstar;
    P.tstar_stage = fixed_tstar ? nullptr : c->v1_tstar_stage;
    c->v1_tstar_stage = nullptr;
    bool regrown;
    ISDF_TRY(c->v1.reserve(c, (size_t)c->M, true, &regrown));
    if (regrown) c->scan_order_b = c->scan_order_e = -1;
    c->v1.bind(P);
    // The scan's dispatch order, longest first.  Mesh robots: sorted in this step's prepare kernel from last step's durations.  Analytic
    // robots: written by step k's back-prop kernel for step k + 1 - valid only for the same shard of the same points.
    const bool scan_lpt = !c->env_no_lpt && !fixed_tstar;
    const bool sort_here = c->shape.kind == ISDF_SHAPE_MESH;
    P.scan_ticks = scan_lpt ? c->v1.scan_ticks.get() : nullptr; P.scan_order_out = scan_lpt ? c->v1.scan_order.get() : nullptr; P.scan_sort_here = (scan_lpt && sort_here) ? 1 : 0;
    const bool order_valid = sort_here || (c->scan_order_b == (long long)b && c->scan_order_e == (long long)e && c->scan_order_epoch == c->points_epoch);
    P.scan_order = (scan_lpt && order_valid) ? c->v1.scan_order.get() : nullptr;
    // (what scan_order will hold once this step's launches are QUEUED; until then it counts as unwritten - a failure in between must
    // not leave the next step scanning through an order nobody wrote)
    const long long order_b = sort_here ? -1 : b, order_e = sort_here ? -1 : e;
    if (scan_lpt) { c->scan_order_b = c->scan_order_e = -1; }
    P.direct_records = fixed_tstar ? 1 : 0;
    ISDF_TRY(c->d_hist.reserve(c, (size_t)N));
    P.hist = c->d_hist;
    P.stats = c->d_stats;
    P.dbg = nullptr;
    ISDF_TRY(debug_timing_buffer(c, (size_t)c->M * 7 + (size_t)(N + 1) * 8, st, &P.dbg));
    if (fixed_tstar) {               // the minimisers are given (isdf_eval_swept_at_tstar): no search
        launch_swept_fixed(P, d_tstar, st);
        launch_swept_reduce(P, d_out, st);
        HIPCHK(c, hipGetLastError());
        return ISDF_OK;
    }
    launch_swept_prepare(P, st);
    ProfEvent *ev;
    ISDF_TRY(prof_begin(c, st, &ev));
    launch_swept_sweep(P, st, ev ? (*ev)[0] : nullptr, ev ? (*ev)[1] : nullptr);
    const bool ev2 = ev && c->prof_secondary;
    if (ev2) { HIPCHK(c, hipEventRecord((*ev)[2], st)); }
    launch_swept_reduce(P, d_out, st);
    if (ev2) { HIPCHK(c, hipEventRecord((*ev)[3], st)); }
    HIPCHK(c, hipGetLastError());
    if (scan_lpt) { c->scan_order_b = order_b; c->scan_order_e = order_e; c->scan_order_epoch = c->points_epoch; }
    return ISDF_OK;
}

// the bit-packed occupancy (z, x and y words) of the tile sweep's row scans, rebuilt after a new grid
static int rebuild_bit_grids(isdf_ctx *c, const isdf_config &cfg, SweepParams &P, hipStream_t st) {
    const int zw = (c->grid.Z + 31) / 32, xw = (c->grid.X + 31) / 32, yw = (c->grid.Y + 31) / 32;
    const size_t nwz = (size_t)c->grid.X * c->grid.Y * zw, nwx = (size_t)c->grid.Y * c->grid.Z * xw, nwy = (size_t)c->grid.X * c->grid.Z * yw;
    ISDF_TRY(c->d_bits.reserve(c, nwz + nwx + nwy));
    c->grid.ZW = zw; c->grid.XW = xw; c->grid.YW = yw;
    c->grid.bits = c->d_bits; c->grid.bits_x = c->d_bits + nwz; c->grid.bits_y = c->d_bits + nwz + nwx;
    launch_build_bits(c->grid, cfg.variant == ISDF_V3_ESDF_TILE ? 1 : 0, cfg.occ_thresh, c->d_bits, st);
    launch_build_bits_xy(c->grid, cfg.variant == ISDF_V3_ESDF_TILE ? 1 : 0, cfg.occ_thresh, c->d_bits + nwz, c->d_bits + nwz + nwx, st);
    c->bits_dirty = false;
    P.grid = c->grid;
    return ISDF_OK;
}

// Dispatch order built on the device from the work of earlier steps (tile_sweep.hip, plan_wave): a resident (fused) launch
// gives the heaviest samples to the workgroups that are first on their CU; every other launch groups samples of like weight
// into workgroups and dispatches the heaviest first.  Pieces [pb, pe) of total_pieces are this shard's.
static int plan_order(isdf_ctx *c, const isdf_config &cfg, SweepParams &P, bool fused, long long pb, long long pe, long long total_pieces, hipStream_t st) {
    const int N = P.N;
    P.plan_cls_in = nullptr; P.plan_cls_out = nullptr; P.plan_map_out = nullptr; P.plan_zone = 0; P.plan_group = 1;
    P.plan_lr_in = P.plan_hist_in = nullptr; P.plan_lr_out = P.plan_hist_out = nullptr;
    const int K1 = cfg.integral_intervs + 1;
    const long long n_loc = pe - pb, ns_local = n_loc * K1;
    const int nb = (int)((ns_local + 3) / 4);
    P.n_sweep_blocks = nb;                  // (launch_sweep sets it again for its own copy; the tail launch needs it for the order it writes)
    if (c->n_cus == 0) { hipDeviceProp_t pr; c->n_cus = (hipGetDeviceProperties(&pr, c->device) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256; }
    const bool no_plan = c->env_no_lpt;
    // (not for the mesh kind: the cost of a mesh sample is its hierarchy walks, which the pair count does not predict -
    // measured 230 -> 256 us per step with the order on, 20-face mesh)
    bool plan = cfg.enable_pos && !no_plan && !P.sample_map && K1 <= 128 && nb > c->n_cus && ns_local < (1LL << 28) && c->shape.kind != ISDF_SHAPE_MESH;
    long long group = n_loc;
    int zone = 0;
    if (plan) {
        if (fused) {
            // resident launch: zones; the exchange inside a fused multi-GPU launch keeps the plain order
            plan = P.xf.world <= 1 && pb == 0 && pe == total_pieces && ns_local <= PLAN_GROUP_MAX_SAMPLES;
            zone = c->n_cus;
        } else if (nb <= sweep_resident_blocks(P, c->n_cus) && ns_local <= PLAN_GROUP_MAX_SAMPLES) {
            zone = c->n_cus;          // a two-launch step whose sweep is resident anyway (a 50-piece shard): zones as well
        } else if (ns_local > PLAN_GROUP_MAX_SAMPLES) {
            // a batch: every trajectory is sorted by itself (the shard must hold whole trajectories)
            group = N;
            plan = (long long)N * K1 <= PLAN_GROUP_MAX_SAMPLES && pb % N == 0 && pe % N == 0;
        }
    }
    if (!plan) { c->plan_k = 0; return ISDF_OK; }
    const size_t ns_cap = (size_t)4 * nb, np_cap = (size_t)n_loc;
    if (c->plan_ns_cap < ns_cap || c->plan_np_cap < np_cap) {       // two generations of each, with floors
        HIPCHK(c, hipStreamSynchronize(st));
        c->plan_ns_cap = c->plan_np_cap = 0; c->plan_k = 0; c->plan_cur = 0;
        const size_t nsc = std::max(ns_cap, (size_t)4096), npc = std::max(np_cap, (size_t)256);
        HIPCHK(c, c->d_plan_cls.alloc(2 * nsc));
        HIPCHK(c, c->d_plan_map.alloc(2 * nsc));
        HIPCHK(c, c->d_plan_lr.alloc(2 * nsc));
        HIPCHK(c, c->d_plan_hist.alloc(2 * npc * PLAN_CLASSES));
        c->plan_ns_cap = nsc; c->plan_np_cap = npc;
    }
    // the records of earlier steps are laid out by piece: they only carry over to a launch of the same geometry
    const long long geo = ((long long)n_loc << 32) | ((long long)K1 << 20) | ((long long)(fused ? 1 : 0) << 19) | (long long)(group & 0x7FFFF);
    if (c->plan_ns != ns_local || c->plan_nb != nb || c->plan_geo != geo) { c->plan_k = 0; c->plan_ns = ns_local; c->plan_nb = nb; c->plan_geo = geo; }
    // The order is rebuilt once per cycle of PLAN_CYCLE steps (the trajectory moves little between optimizer steps, and
    // building costs the step 0.4 us): step 0 of a cycle - the sweep leaves the classes; step 1 - the tail workgroups
    // turn them into records; step 2 - into the order, written into the buffer NOT in use; from step 3 on the launches
    // run in it.  Single copies of classes / records suffice: each is written in one step and read in the next.
    constexpr int PLAN_CYCLE = 8;
    const int k = c->plan_k, ph = k % PLAN_CYCLE;
    const size_t nsc = c->plan_ns_cap;
    P.plan_zone = zone;
    P.plan_group = (int)group;
    if (ph == 0) P.plan_cls_out = c->d_plan_cls;
    if (ph == 1) { P.plan_cls_in = c->d_plan_cls; P.plan_lr_out = c->d_plan_lr; P.plan_hist_out = c->d_plan_hist; }
    if (ph == 2) { P.plan_lr_in = c->d_plan_lr; P.plan_hist_in = c->d_plan_hist; P.plan_map_out = c->d_plan_map + (size_t)(1 - c->plan_cur) * nsc; }
    if (ph == 3) c->plan_cur = 1 - c->plan_cur;          // the order written by the previous step is complete
    if (k >= 3) P.sample_map = c->d_plan_map + (size_t)c->plan_cur * nsc;
    if (c->plan_k < (1 << 30)) c->plan_k++;
    return ISDF_OK;
}

// Mesh robots: the exact pass runs as its own launch over a queue of 64-voxel blocks (every block an independent work item:
// the launch is balanced over the whole device instead of ending on its heaviest workgroup).  Sized for the worst case the
// geometry allows - every voxel of the robot's inflated bounding box (or of the tile, if smaller) occupied; beyond the budget
// below the exact pass stays inside the sweep kernel (ISDF_MESH_QUEUE=0 forces that).
static int mesh_queue(isdf_ctx *c, const isdf_config &cfg, SweepParams &P, size_t ns_loc) {
    const double k3 = (double)cfg.kernel_size * cfg.kernel_size * cfg.kernel_size;
    double vox = k3;
    if (c->shape.prune_rows) {
        double v = 1.0;
        for (int a = 0; a < 3; a++) v *= ((double)c->shape.bbox_hi[a] - (double)c->shape.bbox_lo[a] + 2.2 * cfg.safety_hor) / P.grid.res + 3.0;
        vox = std::min(k3, v * 1.8);                  // (rows are pruned by the box's extent on the WORLD axes: up to sqrt(3) per axis for a rotated box)
    }
    const int kmax = (int)(k3 / 16.0) + 2;            // items are 16 voxels (tile_sweep.hip MQ_BLOCK)
    const size_t per_sample = (size_t)(vox / 16.0) + 2;
    const size_t cap = ns_loc * per_sample;
    const size_t bytes = cap * (16 * 4 + 8 + 80) + ns_loc * ((size_t)kmax * 4 + 4);
    // budget: 1 GiB per ctx (ISDF_MESH_QUEUE_MAX_MB overrides).  A launch whose worst case needs more keeps the exact pass inside
    // the sweep kernel (whose 64-voxel blocks partition a sample's sums differently: equal to rounding, not bitwise)
    static const size_t mq_budget = [] { const char *e = getenv("ISDF_MESH_QUEUE_MAX_MB"); const long v = e ? atol(e) : 0; return (size_t)(v > 0 ? v : 1024) << 20; }();
    if (ns_loc == 0 || bytes > mq_budget || cap >= 0x7fffffffull) return ISDF_OK;
    if (c->mq_cap < cap || c->mq_samples_cap < ns_loc || c->mq_kmax != kmax) {
        HIPCHK(c, hipDeviceSynchronize());               // (an earlier step may still be reading the old queue)
        c->mq_cap = 0; c->mq_samples_cap = 0;
        c->d_mq_entries.release(); c->d_mq_items.release(); c->d_mq_res.release(); c->d_mq_sample_items.release(); c->d_mq_sample_n.release();
        HIPCHK(c, c->d_mq_entries.alloc(cap * 16));
        HIPCHK(c, c->d_mq_items.alloc(cap));
        HIPCHK(c, c->d_mq_res.alloc(cap * 10));
        HIPCHK(c, c->d_mq_sample_items.alloc(ns_loc * (size_t)kmax));
        HIPCHK(c, c->d_mq_sample_n.alloc(ns_loc));
        if (!c->d_mq_count) HIPCHK(c, c->d_mq_count.alloc(4));
        c->mq_cap = cap; c->mq_samples_cap = ns_loc; c->mq_kmax = kmax;
    }
    P.mq_entries = c->d_mq_entries; P.mq_items = c->d_mq_items; P.mq_res = c->d_mq_res;
    P.mq_sample_items = c->d_mq_sample_items; P.mq_sample_n = c->d_mq_sample_n; P.mq_count = c->d_mq_count;
    P.mq_cap = (unsigned)c->mq_cap; P.mq_kmax = kmax;
    return ISDF_OK;
}

// mode 0: the sweep cfg.variant names; 1: the swept-volume sweep; 2: the integral sweep with the collision term off
// (modes 1 + 2 together are what costFunctionLmbm runs for the reference's live configuration)
int eval_device_impl(isdf_ctx *c, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out,
                     double *d_tstar, hipStream_t st, int mode, bool fixed_tstar, const HostDirect *hd) {
    isdf_config cfg = c->cfg;
    if (mode == 1) cfg.variant = ISDF_V1_SWEPT;
    if (mode == 2) { cfg.variant = ISDF_V3_ESDF_TILE; cfg.enable_pos = 0; }
    c->stats_cached = false;
    if (n_traj < 1 || N < 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "n_traj and N must be >= 1");
    if (!d_T || !d_coeffs || !d_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null device buffer");
    if (!c->have_shape && (cfg.variant == ISDF_V1_SWEPT || cfg.enable_pos)) return isdf_fail(c, ISDF_ERR_STATE, "shape not set");
    HIPCHK(c, hipSetDevice(c->device));

    if (cfg.variant == ISDF_V1_SWEPT) return hd ? ISDF_DIRECT_NA : v1_step(c, cfg, n_traj, N, d_T, d_coeffs, d_out, d_tstar, st, fixed_tstar);

    // ---- V2 / V3 integral sweep
    // the tile sweep's mesh walks keep MESH_Q_LEVELS levels of frames in LDS: a deeper hierarchy (a strongly unbalanced mesh)
    // would index past them - refused here, not corrupted there (the swept-volume sweep takes such meshes: wave-cooperative walks)
    if (cfg.enable_pos && c->shape.kind == ISDF_SHAPE_MESH && c->mesh_depth > isdf::MESH_Q_LEVELS)
        return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "mesh hierarchy deeper than 12 levels: the tile sweep (V2 / V3) does not take it (the swept-volume sweep does)");
    if (cfg.enable_pos) {
        if (!c->have_geom) return isdf_fail(c, ISDF_ERR_STATE, "grid not set");
        if (cfg.variant == ISDF_V3_ESDF_TILE && !c->d_esdf) return isdf_fail(c, ISDF_ERR_STATE, "V3 needs an ESDF grid");
        if (cfg.variant == ISDF_V2_OCC_TILE && !c->d_occ) return isdf_fail(c, ISDF_ERR_STATE, "V2 needs an occupancy grid");
    }
    const long long total_pieces = (long long)n_traj * N;
    long long pb, pe;
    shard_range(total_pieces, c->rank, c->world, pb, pe);
    const size_t n_samples = (size_t)total_pieces * (cfg.integral_intervs + 1);
    const size_t ns_loc = (size_t)(pe - pb) * (cfg.integral_intervs + 1);
    { int rc0 = isdf_reserve_sweep_buffers(c, total_pieces); if (rc0) return rc0; }
    int rc = ISDF_OK;
    SweepParams P{};
    P.grid = c->grid;
    if (!c->have_geom) { P.grid.X = P.grid.Y = P.grid.Z = 1; P.grid.res = 1.0; }
    P.shape = c->shape;
    isdf_fill_flat(cfg, P.flat);
    P.variant = cfg.variant; P.K = cfg.integral_intervs; P.enable_dyn = cfg.enable_dyn; P.enable_pos = cfg.enable_pos;
    P.enable_cull = cfg.enable_cull;
    P.n_traj = n_traj; P.N = N; P.piece_begin = (int)pb; P.piece_end = (int)pe;
    P.bd_half = cfg.kernel_size * P.grid.res / 2;
    P.safety_hor = cfg.safety_hor; P.weight_p = cfg.weight_p; P.weight_v = cfg.weight_v; P.weight_omg = cfg.weight_omg;
    P.weight_theta = cfg.weight_theta;
    P.vel_sqr_max = cfg.vmax * cfg.vmax; P.omg_sqr_max = cfg.omgmax * cfg.omgmax; P.theta_max = cfg.thetamax;
    P.mu = cfg.smoothing_eps; P.inv_mu = 1.0 / cfg.smoothing_eps; P.inv_K = 1.0 / cfg.integral_intervs;
    P.occ_thresh = (float)cfg.occ_thresh;
    P.cull_threshold = 0.0;
    if (cfg.variant == ISDF_V3_ESDF_TILE && cfg.enable_cull && c->shape.bound_radius > 0)
        P.cull_threshold = c->shape.bound_radius + cfg.safety_hor + std::sqrt(3.0) * P.grid.res + (cfg.occ_thresh > 0 ? cfg.occ_thresh : 0.0);   // a qualifying voxel lies within occ_thresh of an occupied one
    P.T = d_T; P.coeffs = d_coeffs; P.acc = c->d_acc; P.sample_info = c->d_sample_info; P.piece_cost = c->d_piece_cost;
    P.out = d_out; P.stats = c->d_stats;
    P.dbg = nullptr;
    P.sample_map = (c->d_sample_map && c->sample_map_n == 4 * ((ns_loc + 3) / 4)) ? c->d_sample_map.get() : nullptr;
    P.dbg_flags = 0;
    if (const char *e = getenv("ISDF_DEBUG_FLAGS")) P.dbg_flags = atoi(e);
    rc = debug_timing_buffer(c, n_samples * 8 + (size_t)total_pieces * 4 + 4, st, &P.dbg);
    if (rc) return rc;
    if (cfg.enable_pos && c->bits_dirty) { rc = rebuild_bit_grids(c, cfg, P, st); if (rc) return rc; }
    c->last_P = P; c->have_last_P = true;
    ProfEvent *ev;
    rc = prof_begin(c, st, &ev);
    if (rc) return rc;
    if (ev && !cfg.enable_pos) { ev = nullptr; c->prof_used--; }      // no dominant kernel in a dynamics-only step
    const bool ev2 = ev && c->prof_secondary;
    // a small step (one trajectory) is ONE launch: the tail's workgroups ride behind the sweep's (tile_sweep.hip, FUSED)
    const bool fused = c->fuse_small && !ev2 && sweep_can_fuse(P);
    {   // multi-GPU step with the exchange inside the step's launches (isdf_xchg_fuse)
        int xerr = ISDF_OK;
        if (isdf_xchg_fill(c, &P.xf, (size_t)total_pieces, &xerr)) {
            if (xerr != ISDF_OK) return xerr;
            // a step that is not one fused launch carries the exchange in its tail launch (tail_kernel_xf); a step without a
            // collision term has no sweep launch either way
        }
    }
    if (hd) {
        if (!fused || P.xf.world > 1 || P.dbg) return ISDF_DIRECT_NA;
        { int rc1 = ensure_stage(c, (size_t)total_pieces); if (rc1) return rc1; }
        P.out = hd->out; P.host_flag = hd->flags; P.seq = hd->seq;
        if (!hd->via_bar) { P.host_T = hd->T; P.host_coeffs = hd->coeffs; P.stage = c->d_stage; P.stage_flags = c->d_stage_flags; }
        c->last_P = P;
    }
    rc = plan_order(c, cfg, P, fused, pb, pe, total_pieces, st);
    if (rc) return rc;
    if (!fused && cfg.enable_pos) {                 // the poses of a non-fused launch come from pose_kernel (tile_sweep.hip)
        const size_t need = ns_loc * sweep_pose_bytes();
        if (c->d_pose.capacity() < need) {
            HIPCHK(c, hipStreamSynchronize(st));
            rc = c->d_pose.reserve(c, need);
            if (rc) return rc;
        }
        P.poses = c->d_pose;
    }
    P.mq_items = nullptr;
    if (c->shape.kind == ISDF_SHAPE_MESH && cfg.enable_pos && !fused && !env_is("ISDF_MESH_QUEUE", '0')) {
        rc = mesh_queue(c, cfg, P, ns_loc);
        if (rc) return rc;
    }
    launch_sweep(P, st, ev ? (*ev)[0] : nullptr, ev ? (*ev)[1] : nullptr, fused);
    if (!fused) launch_tail(P, st, ev2 ? (*ev)[2] : nullptr, ev2 ? (*ev)[3] : nullptr);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

// every sweep of the host paths goes through here
int sweep_dispatch(isdf_ctx *c, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out, double *d_tstar,
                   hipStream_t st, int mode, bool fixed_tstar) {
    // (a one-device ctx created with the RCCL collective takes the multi-device path too: the all-reduce of a world of one)
    if (!c->peers.empty() || c->rccl_comm) return multi_eval_device(c, n_traj, N, d_T, d_coeffs, d_out, d_tstar, st, mode, fixed_tstar);
    return eval_device_impl(c, n_traj, N, d_T, d_coeffs, d_out, d_tstar, st, mode, fixed_tstar);
}

extern "C" int isdf_eval_device(isdf_ctx *c, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out,
                                double *d_tstar, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (c->is_peer) return isdf_fail(c, ISDF_ERR_STATE, "this ctx belongs to a multi-device ctx");
    return sweep_dispatch(c, n_traj, N, d_T, d_coeffs, d_out, d_tstar, (hipStream_t)stream);
}

// The swept-volume sweep's back-prop with the minimisers GIVEN: for every obstacle point the robot SDF and its body-frame
// gradient are evaluated at d_tstar[pt] instead of being searched for (a negative / NaN entry = "no interval qualified").
extern "C" int isdf_eval_swept_at_tstar(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, double *d_out,
                                        const double *d_tstar, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!d_tstar) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null t* buffer");
    // (a multi-device ctx would return its lead's shard only: refused, as the header says)
    if (!c->peers.empty() || c->is_peer || c->rccl_comm) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "isdf_eval_swept_at_tstar on a multi-device ctx");
    return eval_device_impl(c, 1, N, d_T, d_coeffs, d_out, const_cast<double *>(d_tstar), (hipStream_t)stream, 1, true);
}

int fetch_stats(isdf_ctx *c) {
    unsigned long long h[8];
    if (c->cfg.variant != ISDF_V1_SWEPT && c->have_last_P) {
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, hipMemset(c->d_stats, 0, 4 * sizeof(unsigned long long)));   // keep [4] = overflow flag
        launch_stats(c->last_P, nullptr);
        HIPCHK(c, hipDeviceSynchronize());
    }
    HIPCHK(c, hipMemcpy(h, c->d_stats, sizeof(h), hipMemcpyDeviceToHost));
    c->last_stats.n_units = (int64_t)h[0]; c->last_stats.n_units_culled = (int64_t)h[1];
    c->last_stats.n_pairs = (int64_t)h[2]; c->last_stats.n_grad_pairs = (int64_t)h[3];
    c->last_stats.overflow = (int32_t)h[4];
    if (h[4]) {                                                                       // sticky until read
        const int rr = clear_overflow(c);                                               // a late producer must not feed the next step
        if (rr) return rr;
    }
    return ISDF_OK;
}

// --------------------------------------------------------------------------------------------------------------
// instrumentation
// --------------------------------------------------------------------------------------------------------------
extern "C" int isdf_profile_enable(isdf_ctx *c, int on) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    c->prof_on = on != 0;          // on = N > 0: instrument every N-th launch (event records cost GPU time)
    c->prof_secondary = on > 0 && (on & ISDF_PROFILE_SECONDARY) != 0;
    on &= ~ISDF_PROFILE_SECONDARY;
    c->prof_every = on > 0 ? on : 1;
    c->prof_tick = 0;
    c->prof_used = 0;
    return ISDF_OK;
}

extern "C" int isdf_profile_read(isdf_ctx *c, int *n, double *mean_ms) {
    if (!c || !n || !mean_ms) return ISDF_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    double sum = 0.0, sum2 = 0.0;
    for (size_t i = 0; i < c->prof_used; i++) {
        HIPCHK(c, hipEventSynchronize(c->prof_events[i][c->prof_secondary ? 3 : 1]));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->prof_events[i][0], c->prof_events[i][1]));
        sum += ms;
        if (c->prof_secondary) {
            HIPCHK(c, hipEventElapsedTime(&ms, c->prof_events[i][2], c->prof_events[i][3]));
            sum2 += ms;
        }
    }
    *n = (int)c->prof_used;
    *mean_ms = c->prof_used ? sum / c->prof_used : 0.0;
    c->last_exact_ms = c->prof_used ? sum2 / c->prof_used : 0.0;
    c->prof_used = 0;
    return ISDF_OK;
}

extern "C" int isdf_profile_read_secondary(isdf_ctx *c, double *mean_ms) {
    if (!c || !mean_ms) return ISDF_ERR_INVALID_ARG;
    *mean_ms = c->last_exact_ms;
    return ISDF_OK;
}

// developer tool (not declared in the ABI header): copies the timing words of the last step when ISDF_DEBUG_TIMING=1
extern "C" long long isdf_debug_timing(isdf_ctx *c, unsigned long long *out, long long cap) {
    if (!c || !c->d_dbg) return 0;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    const long long n = (long long)c->dbg_used < cap ? (long long)c->dbg_used : cap;
    if (out && n > 0) (void)hipMemcpy(out, c->d_dbg, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    return (long long)c->dbg_used;
}

extern "C" int isdf_get_stats(isdf_ctx *c, isdf_stats *out) {
    if (!c || !out) return ISDF_ERR_INVALID_ARG;
    if (!c->stats_cached) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipDeviceSynchronize());
        int rc = fetch_stats(c);
        if (rc) return rc;
        rc = add_peer_stats(c);
        if (rc) return rc;
    }
    *out = c->last_stats;
    return ISDF_OK;
}

// developer tool (not declared in the ABI header): dispatch order of the tile sweep's samples (a permutation of 0..n-1)
extern "C" int isdf_debug_set_sample_map(isdf_ctx *c, const int *map, long long n) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->d_sample_map.release(); c->sample_map_n = 0;
    if (!map || n <= 0) return ISDF_OK;
    if (c->d_sample_map.alloc((size_t)n) != hipSuccess) return ISDF_ERR_HIP;
    (void)hipMemcpy(c->d_sample_map, map, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
    c->sample_map_n = (size_t)n;
    return ISDF_OK;
}

// developer tool (not declared in the ABI header): the longest-first dispatch order the NEXT fused step would use
// (4 * workgroups entries, -1 = none); returns the number of consecutive steps the plan has been running, 0 = inactive
extern "C" int isdf_debug_plan_map(isdf_ctx *c, int *out, long long cap) {
    if (!c || c->plan_k < 4 || !c->d_plan_map) return 0;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    const long long n = 4LL * c->plan_nb < cap ? 4LL * c->plan_nb : cap;
    if (out && n > 0) (void)hipMemcpy(out, c->d_plan_map + (size_t)c->plan_cur * c->plan_ns_cap, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
    return c->plan_k;
}

// developer tool (not declared in the ABI header): per-sample (exact pairs, active pairs | culled << 31) of the last integral step
extern "C" long long isdf_debug_sample_info(isdf_ctx *c, int *out, long long cap) {
    if (!c || !c->d_sample_info || !c->have_last_P) return 0;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    const long long n = (long long)(c->last_P.piece_end - c->last_P.piece_begin) * (c->last_P.K + 1);
    const long long m = 2 * n < cap ? 2 * n : cap;
    if (out && m > 0) (void)hipMemcpy(out, c->d_sample_info, (size_t)m * sizeof(int), hipMemcpyDeviceToHost);
    return n;
}

// developer tool (not declared in the ABI header): the HIP runtime's pending error of the calling thread, without clearing it
extern "C" const char *isdf_debug_peek_hip_error(void) { return hipGetErrorString(hipPeekAtLastError()); }
