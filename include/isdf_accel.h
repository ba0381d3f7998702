/*
 * isdf_accel.h — C ABI of the MI355X-native collision cost/gradient engine.
 *
 * This is the drop-in boundary for ONE hot path of ZJU-FAST-Lab/Implicit-SDF-Planner: the per-optimizer-step
 * sweeps that TrajOptimizer::costFunctionLmbm calls
 *   (src/planner_algorithm/include/planner_algorithm/back_end_optimizer.hpp:386-391 and :399-405).
 * Plain C, plain pointers and sizes; no Eigen / torch / C++ types cross it.  Every entry point returns
 * ISDF_OK (0) or a negative isdf_status and never throws; isdf_last_error() gives the message.
 *
 * Conventions (SURVEY.md §8 "Conventions"):
 *   N  = pieces of one trajectory,  K = integralIntervs (K+1 samples per piece),  M = obstacle points.
 *   coeffs = the optimizer's Eigen::MatrixX3d, 6N x 3, COLUMN-major: element (r,c) at data[c*6N + r];
 *            rows 6i..6i+5 are the ascending-power coefficients c0..c5 of piece i (minco.hpp:402,545).
 *   gradC  has the same layout; gradT and T have N entries.
 *   Outputs of the host entry points are ACCUMULATED (+=) into caller-owned storage, exactly like
 *   addSaftyPenaOnSweptVolumeParallel / addTimeIntPenaltyParallel (back_end_optimizer.hpp:557-562, :432-438).
 *   A ctx may be used by one host thread at a time (the reference's LMBM trampolines are process-global
 *   statics, lmbm.cpp:4-6, so the reference is not re-entrant either).
 */
#ifndef ISDF_ACCEL_H
#define ISDF_ACCEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISDF_ABI_VERSION 1

typedef enum isdf_status {
    ISDF_OK = 0,
    ISDF_ERR_INVALID_ARG = -1,
    ISDF_ERR_NO_DEVICE = -2,     /* no usable HIP device: the product path has NO CPU fallback */
    ISDF_ERR_HIP = -3,           /* a HIP runtime call failed; see isdf_last_error */
    ISDF_ERR_STATE = -4,         /* grid / shape / points not set for the requested sweep */
    ISDF_ERR_OVERFLOW = -5,      /* a bounded device-side work list overflowed (result NOT valid) */
    ISDF_ERR_UNSUPPORTED = -6
} isdf_status;

/* Which sweep isdf_eval runs.  V1 is the reference's live path, V2 its dormant integral path, V3 the
 * ESDF-tile kernel of BASELINE.json's north_star (SURVEY.md §8 "Variants", Appendix A.3-A.5). */
typedef enum isdf_variant {
    ISDF_V1_SWEPT = 1,     /* addSaftyPenaOnSweptVolumeParallel, back_end_optimizer.hpp:557-649            */
    ISDF_V2_OCC_TILE = 2,  /* addTimeIntPenaltyParallel :432-554 with grad_cost_p :766-824 (occupancy tile)  */
    ISDF_V3_ESDF_TILE = 3  /* same sweep, voxel qualifies iff esdf <= occ_thresh, optional whole-tile cull   */
} isdf_variant;

typedef enum isdf_grid_kind { ISDF_GRID_OCCUPANCY = 0, ISDF_GRID_ESDF = 1 } isdf_grid_kind;
typedef enum isdf_dtype { ISDF_U8 = 0, ISDF_F32 = 1, ISDF_F64 = 2 } isdf_dtype;

/* Robot-shape plugin kinds = the analytic-shape registry of
 * src/swept_volume/include/swept_volume/sw_manager.hpp:74-123 plus Box/Ball/mesh.
 * params[] meaning per kind (reference constants are what isdf_shape_default() fills in):
 *   TORUS              [0]=major radius (2.5 | Torus_big 3.5) [1]=minor radius (0.3)            Shape.hpp:824-893
 *   CAPPEDTORUS        [0]=sc.x (sin(40 rad)) [1]=sc.y (cos(40 rad)) [2]=ra 3.5 [3]=rb 0.3      Shape.hpp:895-931
 *   CAPPEDCONE         [0]=ra 2 [1]=rb 0.8 [2..4]=a (0,0,-1) [5..7]=b (0,0,1)                   Shape.hpp:933-998
 *   ROUNDEDCONE        [0]=r1 1.5 [1]=r2 0.6 [2]=h 4.5                                          Shape.hpp:1000-1047
 *   WIREFRAMEBOX       [0..2]=size (1.8,2.5,3.5) [3]=thickness 0.1                              Shape.hpp:1049-1103
 *   BENDLINEAR         [0]=capsule half length (2 | _big 3.2) [1]=radius (0.25 | _big 0.45)     Shape.hpp:1105-1234
 *   TWISTBOX           [0..2]=size (2,2,2) [3]=k (pi/6)                                         Shape.hpp:1236-1288
 *   BENDBOX            [0..2]=size (2,2,2) [3]=k (0.5)                                          Shape.hpp:1290-1341
 *   TABLE              [0..2]=a1 [3..5]=b1 [6..8]=a2 [9..11]=b2                                 Shape.hpp:1343-1405
 *   TREFOIL            [0]=r 3.5 [1],[2]=box half sizes 0.2 [3]=rounding 0.05 [4]=scale 0.4     Shape.hpp:1442-1515
 *   SMOOTHDIFFERENCE   [0..2]=box size (3,3,0.5) [3]=sphere radius 1 [4]=k 0.25                 Shape.hpp:1517-1570
 *   SMOOTHINTERSECTION [0..2]=box size (3,3,0.5 | _big 9,9,1.5) [3]=radius (1 | 3) [4]=k 0.25   Shape.hpp:1572-1682
 *   CSG                [0]=sphere r 3 [1]=box edge 4.5 [2]=cylinder r 1.5                       Shape.hpp:1684-2317
 *   BOX                [0..2]=half extents (conf.box_x/y/z)                                     Shape.hpp:2320-2390
 *   BALL               [0]=radius (Point == radius 0)                                           Shape.hpp:603-665
 *   MESH               triangle soup: sign from the fast winding number, distance to the closest triangle
 *                                                                                               Shape.cpp:105-151 */
typedef enum isdf_shape_kind {
    ISDF_SHAPE_TORUS = 0,
    ISDF_SHAPE_CAPPEDTORUS = 1,
    ISDF_SHAPE_CAPPEDCONE = 2,
    ISDF_SHAPE_ROUNDEDCONE = 3,
    ISDF_SHAPE_WIREFRAMEBOX = 4,
    ISDF_SHAPE_BENDLINEAR = 5,
    ISDF_SHAPE_TWISTBOX = 6,
    ISDF_SHAPE_BENDBOX = 7,
    ISDF_SHAPE_TABLE = 8,
    ISDF_SHAPE_TREFOIL = 9,
    ISDF_SHAPE_SMOOTHDIFFERENCE = 10,
    ISDF_SHAPE_SMOOTHINTERSECTION = 11,
    ISDF_SHAPE_CSG = 12,
    ISDF_SHAPE_BOX = 13,
    ISDF_SHAPE_BALL = 14,
    ISDF_SHAPE_MESH = 15,
    ISDF_SHAPE_GRID = 16,   /* a body-frame lattice of (unit gradient, distance) sampled from ANY host shape: isdf_set_shape_grid */
    ISDF_SHAPE_PROGRAM = 17,/* a composition from the CSG class's op library (Shape.hpp:1684-2317) as an instruction list: isdf_set_shape_program */
    ISDF_SHAPE_KIND_COUNT = 18
} isdf_shape_kind;

/* How getonlyGrad1 / getSDFwithGrad1 form the body-frame gradient. */
typedef enum isdf_grad_mode {
    ISDF_GRAD_DEFAULT = 0,      /* what the reference class of this kind does                                  */
    ISDF_GRAD_CENTRAL = 1,      /* DEFINE_USEFUL_FUNCTION: central difference dx=5e-6, normalised Shape.hpp:32-88 */
    ISDF_GRAD_BOX_FORWARD = 2,  /* Box::getonlyGrad1: forward difference dx=0.01, NOT normalised  Shape.hpp:2363-2377 */
    ISDF_GRAD_ANALYTIC_BALL = 3,/* Ball/Point: p / |p|                                           Shape.hpp:622-630 */
    ISDF_GRAD_GRID = 4          /* ISDF_SHAPE_GRID: trilinear blend of the nodes' gradients, normalised Shape.hpp:520-553 */
} isdf_grad_mode;

typedef struct isdf_shape {
    int32_t kind;          /* isdf_shape_kind */
    int32_t grad_mode;     /* isdf_grad_mode */
    double params[16];
    double trans[3];       /* yaml poly_params xyz; every analytic SDF first maps p -> (p - trans) * Rotate */
    double rotate[9];      /* row-major 3x3 Rotate = yaw*pitch*roll (Shape.cpp:38-43)                       */
    double bound_radius;   /* >0: a radius R with sdf(p) >= |p| - R for every body-frame point p (enables the V3
                              whole-tile cull); 0 disables the cull for this shape                            */
    double bbox_center[3]; /* body-frame box with sdf(p) >= distance(p, box) for every p outside it, i.e. the   */
    double bbox_half[3];   /* shape lies inside the box and its SDF never under-estimates by more than the box  */
                           /* does.  All bbox_half > 0 lets the scan prune voxel rows that cannot reach the      */
                           /* penalty band; zeros disable the pruning.  Results are identical either way.        */
    /* MESH only (already transformed into the body frame exactly as Generalshape's constructor does).  For a CLOSED mesh
       isdf_set_shape also samples a lattice of node-to-surface distances on the device (a few milliseconds, 4 MB): the tile
       sweep's pre-filter for this kind (it drops listed voxels that provably carry no penalty; results agree to rounding with
       and without it) and the swept-volume scans' way of telling which samples need a hierarchy query at all (bitwise the same
       results).  ISDF_NO_F32_FILTER=1 builds none. */
    const double *mesh_vertices;  /* nV x 3 row-major */
    const int32_t *mesh_faces;    /* nF x 3 row-major */
    int32_t n_vertices;
    int32_t n_faces;
} isdf_shape;

/* Mirrors the Config fields the hot path reads (src/utils/include/utils/config.hpp; yaml in
 * src/plan_manager/config).  Defaults of isdf_config_default() are config_CappedCone.yaml (demo1). */
typedef struct isdf_config {
    int32_t device;            /* HIP device ordinal                                                        */
    int32_t variant;           /* isdf_variant                                                              */
    int32_t kernel_size;       /* tile edge in voxels; bd = kernel_size * occupancy_resolution (:692)        */
    int32_t integral_intervs;  /* K                                                                         */
    int32_t enable_dyn;        /* 1: velocity / body-rate / tilt penalties of addTimeIntPenaltyParallel      */
    int32_t enable_pos;        /* 1: add the collision term grad_cost_p to that sweep (V2/V3)                */
    int32_t enable_cull;       /* V3: skip a pose whose trilinear esdf(pos) proves every penalty is zero     */
    int32_t reserved0;
    double safety_hor;
    double weight_p, weight_v, weight_omg, weight_theta;
    double vmax, omgmax, thetamax;
    double smoothing_eps;      /* mu of smoothedL1 in the integral sweep (V1 hard-codes 0.01, :851)          */
    double occ_thresh;         /* V3: voxel qualifies iff esdf <= occ_thresh (0 == "occupied")               */
    double vehicle_mass, grav_acc, horiz_drag, vert_drag, paras_drag, speed_eps;   /* flatness.hpp:36-51 */
} isdf_config;

typedef struct isdf_ctx isdf_ctx;   /* opaque; owns all device state */

/* ---- lifetime -------------------------------------------------------------------------------------------- */
void isdf_config_default(isdf_config *cfg);
int isdf_shape_default(isdf_shape *shape, int kind);       /* reference constants for an analytic kind   */
int isdf_shape_from_name(isdf_shape *shape, const char *obj_stem); /* registry lookup, sw_manager.hpp:74-123,
                                                              e.g. "RoundedCone", "Torus_big"; <0 if the
                                                              stem is not an analytic shape (=> mesh)     */
int isdf_create(isdf_ctx **out, const isdf_config *cfg);
/* ONE host process driving n_devices GPUs (SURVEY.md 8(b) "Threading"; the reference's caller is one ROS process,
 * back_end_optimizer.hpp:386-391,399-405): the returned ctx is used EXACTLY like a single-device one - cfg.device is ignored,
 * devices[0] is where device-resident arguments of isdf_eval_device live.  Once-per-plan state (isdf_set_grid / _shape /
 * _points / _pointcloud / _generate_esdf / _gather_points) is replicated on every device; every step (isdf_eval,
 * isdf_eval_device, isdf_cost_function[_lmbm], isdf_optimize_lbfgs) shards the constraint points by piece (V2 / V3) or by
 * obstacle point (V1) like isdf_set_shard would, queues every shard on its own device's stream FROM THE CALLING THREAD (no host
 * threads are created) and sums the shards' packed [cost | gradT | gradC] on devices[0] - ONE exchange per sweep:
 *   ISDF_MULTI_PEER_SUM  a kernel on devices[0] reading the peers' buffers over xGMI in rank order (default when peer access
 *                        exists; bitwise reproducible),
 *   ISDF_MULTI_STAGED    peer copies to devices[0] + the same sum (no peer access needed),
 *   ISDF_MULTI_RCCL      one ncclAllReduce(sum, ncclDouble) over all devices (environment ISDF_MULTI_COLLECTIVE=rccl; librccl.so
 *                        is dlopen-ed then - the library itself does not link RCCL; needs DISTINCT devices).
 * A device may be listed more than once (the shards then share it: how the single-GPU tests drive this path).
 * Not available on such a ctx: isdf_set_shard, isdf_xchg_*, isdf_optimize_lbfgs_batch, isdf_eval_swept_at_tstar. */
#define ISDF_MULTI_NONE 0
#define ISDF_MULTI_PEER_SUM 1
#define ISDF_MULTI_STAGED 2
#define ISDF_MULTI_RCCL 3
int isdf_create_multi(isdf_ctx **out, const isdf_config *cfg, const int *devices, int n_devices);
int isdf_multi_info(const isdf_ctx *ctx, int *n_devices_out, int *collective_out);
/* What isdf_set_shape found and decided about the installed MESH robot (all zero for another kind):
 *   [0] faces  [1] nodes of the winding-number hierarchy  [2] its depth  [3] 1: one swept-volume task per workgroup (quad walks)
 *   [4] 1: every edge is shared by two faces with opposite directions (closed, consistently oriented)
 *   [5] 1: the EXACT winding number is 0 / 1 on the two sides of every face (the surface bounds a solid: no nested sheets of one
 *       orientation, no overlapping or inverted bodies, no tears) - or becomes so within a tenth of the lattice's reach of the face:
 *       a DEFECT pocket of known thickness ([12], [13]; the reference's Trefoil.obj has 18 folded sliver faces), which the lattice's
 *       users allow for; 0: it is not; -1: not tested (no lattice wanted)
 *   [6..8] nodes of the distance lattice per axis (0: none - the mesh failed [4], [5] or the measured range below, or
 *       ISDF_NO_F32_FILTER=1; every query then walks the hierarchy, results are the same bits)
 *   [9], [10] 1e6 x the smallest / largest |1 - 2 w| the reference's approximate winding number took at the lattice's sample
 *       points away from the surface (nodes, cell centres, edge midpoints; a lattice is kept only for 0.96 ... 1.04)
 *   [11] (node, child) slots of the FLAT evaluation small meshes get in the swept-volume sweep (<= 64 slots: the reference's
 *       12- to 20-face robots; 0: the hierarchy is walked).
 *   [12] 1e9 x the thickness (m) of the thickest defect pocket found next to a face (0: a clean surface)  [13] 1e3 x the largest
 *       |1 - 2 w| inside one  [14], [15] 0.
 * Replaces: nothing (the reference builds its libigl structures without checks, Shape.cpp:60-103). */
int isdf_mesh_info(const isdf_ctx *ctx, int info_out[16]);
int isdf_destroy(isdf_ctx *ctx);
const char *isdf_last_error(const isdf_ctx *ctx);          /* ctx may be NULL: last create() failure      */
int isdf_abi_version(void);

/* ---- once-per-plan state (replaces TrajOptimizer::setGridMap / setEnvironment and the parallel_points
 *      assembly of plan_manager.cpp:232-254) ------------------------------------------------------------------ */
/* voxels: nx*ny*nz values, z fastest: addr = ix*ny*nz + iy*nz + iz (GridMap3D.h:194).
 * origin = boundary_xyzmin; boundary_max = boundary_xyzmax (NULL => origin + n*resolution; the reference
 * sizes the grid as ceil((max-min)/res), Gridmap3D.cpp:29-31, so max may lie inside the last voxel).
 * An occupancy grid and an ESDF grid may both be set (same geometry); V2 reads the former, V3 the latter. */
int isdf_set_grid(isdf_ctx *ctx, const void *voxels, int dtype, int nx, int ny, int nz,
                  const double origin[3], const double boundary_max[3], double resolution, int grid_kind);
int isdf_set_shape(isdf_ctx *ctx, const isdf_shape *shape);
/* ---- a robot shape the library has never seen: the reference's plugin promise is "subclass Generalshape, add a constructor to
 * the registry" (Shape.hpp:469-472, sw_manager.hpp:74-123); device code cannot call host virtuals, so such a shape comes in the
 * form the reference itself tabulates at start-up: BasicShape::initShape (Shape.hpp:361-404) fills num_sdf_map, a body-frame
 * lattice of NumSDFGridCell {unit gradient, distance} with node (i, j, k) at (-nd/2 + i*nres) per axis, ceil(nd / nres) nodes
 * per axis, by calling the shape's own getSDFwithGrad1 once per node; getonlySDFNum / getonlyGrad1Num / getSDFwithGrad1Num
 * (:481-600) sample it trilinearly (value: 1e20 outside the lattice; gradient: blend of the 8 nodes' gradients, normalised;
 * zero outside).  ISDF_SHAPE_GRID is exactly that sampler on the device - a documented APPROXIMATION of the shape it was
 * sampled from (error O(nres^2 x curvature) on the distance), exact parity with the reference's *Num functions.
 * isdf_set_shape_grid: cells = nx*ny*nz x 4 doubles (gx, gy, gz, distance), address (i*ny + j)*nz + k like toAddr (:466);
 * grid_min = position of node (0,0,0); bound_radius / bbox_* as in isdf_shape (0 / zeros: derived from the lattice box, which is
 * always valid because the sampler returns 1e20 outside it).
 * isdf_set_shape_sampled: builds the cells the way initShape does, by calling `fn` (== getSDFwithGrad1 of any host class:
 * returns the distance, writes the gradient) at every node, then installs them. */
typedef double (*isdf_sdf_with_grad_fn)(void *user, const double p_rel[3], double grad_out[3]);
int isdf_set_shape_grid(isdf_ctx *ctx, const double *cells, int nx, int ny, int nz, const double grid_min[3], double nres,
                        double bound_radius, const double *bbox_center, const double *bbox_half);
int isdf_set_shape_sampled(isdf_ctx *ctx, isdf_sdf_with_grad_fn fn, void *user, double ndx, double ndy, double ndz, double nres,
                           double bound_radius, const double *bbox_center, const double *bbox_half);

/* ---- composed robot shapes: the op library of the reference's CSG class (Shape.hpp:1684-2317) as a device program --------
 * A reference-side Generalshape written with that construction kit maps to a flat instruction list (1 .. ISDF_PROGRAM_MAX_INSTR
 * instructions) that the device evaluates at a body-frame point p.  It is a stack machine: a working point q (starts as p) and a
 * value stack of depth <= ISDF_PROGRAM_MAX_DEPTH.  A DOMAIN instruction rewrites q; a PRIMITIVE pushes its SDF at q and resets q
 * to p; a UNARY instruction rewrites the top of the stack; a BINARY one pops d2 (top), then d1, and pushes one value.  A valid
 * program ends with exactly one value.  A transform that wraps a whole subtree in the reference is written in front of EVERY
 * primitive of that subtree, outermost first (the order the nested closures apply them); transforms are never pre-multiplied, so
 * the arithmetic stays operation for operation.  Every formula is an exact analytic SDF expression: the gradient is the central
 * difference of DEFINE_USEFUL_FUNCTION (Shape.hpp:32-88), ISDF_GRAD_CENTRAL.
 * Parameters p[] per opcode (vectors take three slots) and the lines they restate:
 *   primitives   SPHERE radius, centre :1724 | CAPSULE a, b, radius :1734 | BOX size, centre :1748 | ROUNDED_BOX size, radius :1761
 *                WIREFRAME_BOX size, thickness :1774 (as written there: q is formed from p, not from the shifted point as the
 *                WireframeBox CLASS does, :1076 - the two differ) | TORUS r1, r2 :1799 (xy plane) | CYLINDER radius :1812
 *                CAPPED_CYLINDER a, b, radius :1823 | ROUNDED_CYLINDER ra, rb, h :1851 | CAPPED_CONE ra, rb, a, b :1864
 *                ROUNDED_CONE r1, r2, h :1886 | ELLIPSOID size :1902 | PYRAMID h :1913 | TETRAHEDRON r :1941 | OCTAHEDRON r :1953
 *                DODECAHEDRON r :1962 | ICOSAHEDRON r :1978
 *   domain       TRANSLATE offset :1996 | SCALE factor :2006 (q / factor; the reference's "x min(factor)" is the unary MUL after
 *                the subtree) | ROTATE angle, axis :2021 | ROTATE_TO a, b :2043 (resolved on the host to nothing, to
 *                rotate(pi, perpendicular(a)) or to rotate(acos(a.b), b x a); the rotation matrices are built once on the host)
 *                TWIST k :2198 | BEND k :2215
 *   unary        MUL m :2015 | NEGATE :2250 | DILATE r :2259 | ERODE r :2268 | SHELL thickness :2277
 *   binary       UNION k :2087 | DIFFERENCE k :2134 | INTERSECTION k :2178 (the hard min / max form exactly when k == 0.0)
 *                BLEND k :2232 (one operand: k d2 + (1 - k) d1)
 * Of the reference's vector overloads only the fold of unionOp (:2061) has a meaning of its own - a chain of UNIONs - and blendOp
 * folds the same way.  The vector differenceOp / intersectionOp (:2110-2132, :2155-2176) return inside their loop after the first
 * operand: they ARE the binary forms and are not offered separately.
 * isdf_set_shape_program installs the program in place of isdf_set_shape (which rejects this kind as it rejects GRID).
 * trans / rotate (NULL: none) are the body offset (p - trans) * Rotate that precedes every class formula - for the front end's
 * kernels the order is offset, R_obj, program.  bound_radius / bbox_center / bbox_half (NULL: zeros) mean what they mean in
 * isdf_shape: zeros disable the cull and the row pruning, results are identical either way.  The fp32 pre-filter of the tile sweep
 * is off for this kind.  The whole program is validated BEFORE the ctx is touched; ISDF_ERR_INVALID_ARG (message in
 * isdf_last_error; the installed shape stays installed and usable) for: an unknown opcode, a stack underflow, a depth above 8, a
 * final depth other than 1, fewer than 1 or more than 64 instructions, a non-finite parameter, a zero SCALE factor, a CAPSULE /
 * CAPPED_CYLINDER / CAPPED_CONE with a == b, a ROUNDED_CONE with h == 0, a smoothing k < 0.
 * isdf_shape_program_eval_host: the same arithmetic in plain C++ on the host - no ctx, no device; n_points x 3 body-frame points,
 * sdf_out[n_points] and grad_out[n_points x 3] (either may be NULL).  The same validation applies: ISDF_ERR_INVALID_ARG, and
 * isdf_shape_program_validate gives the message. */
#define ISDF_PROGRAM_MAX_INSTR 64
#define ISDF_PROGRAM_MAX_DEPTH 8
typedef enum isdf_shape_op {
    ISDF_OP_SPHERE = 1, ISDF_OP_CAPSULE = 2, ISDF_OP_BOX = 3, ISDF_OP_ROUNDED_BOX = 4, ISDF_OP_WIREFRAME_BOX = 5, ISDF_OP_TORUS = 6,
    ISDF_OP_CYLINDER = 7, ISDF_OP_CAPPED_CYLINDER = 8, ISDF_OP_ROUNDED_CYLINDER = 9, ISDF_OP_CAPPED_CONE = 10,
    ISDF_OP_ROUNDED_CONE = 11, ISDF_OP_ELLIPSOID = 12, ISDF_OP_PYRAMID = 13, ISDF_OP_TETRAHEDRON = 14, ISDF_OP_OCTAHEDRON = 15,
    ISDF_OP_DODECAHEDRON = 16, ISDF_OP_ICOSAHEDRON = 17,
    ISDF_OP_TRANSLATE = 32, ISDF_OP_SCALE = 33, ISDF_OP_ROTATE = 34, ISDF_OP_ROTATE_TO = 35, ISDF_OP_TWIST = 36, ISDF_OP_BEND = 37,
    ISDF_OP_MUL = 48, ISDF_OP_NEGATE = 49, ISDF_OP_DILATE = 50, ISDF_OP_ERODE = 51, ISDF_OP_SHELL = 52,
    ISDF_OP_UNION = 64, ISDF_OP_DIFFERENCE = 65, ISDF_OP_INTERSECTION = 66, ISDF_OP_BLEND = 67
} isdf_shape_op;
typedef struct isdf_shape_instr {
    int32_t op;            /* isdf_shape_op */
    int32_t reserved;      /* 0 */
    double p[9];           /* the opcode's parameters in the order listed above; unused slots are ignored */
} isdf_shape_instr;
int isdf_set_shape_program(isdf_ctx *ctx, const isdf_shape_instr *instr, int n, const double *trans, const double *rotate,
                           double bound_radius, const double *bbox_center, const double *bbox_half);
int isdf_shape_program_eval_host(const isdf_shape_instr *instr, int n, const double *trans, const double *rotate,
                                 const double *xyz, long long n_points, double *sdf_out, double *grad_out);
/* the validation alone: ISDF_OK, or ISDF_ERR_INVALID_ARG with the message in err_out (nullable; err_cap bytes incl. the 0) */
int isdf_shape_program_validate(const isdf_shape_instr *instr, int n, char *err_out, int err_cap);

int isdf_set_points(isdf_ctx *ctx, const double *xyz, int M);   /* V1: M x 3 row-major obstacle points  */
/* Multi-GPU: this ctx evaluates only its share of the constraint points (pieces for V2/V3, obstacle points
 * for V1); outputs of all ranks SUM to the full result (one all-reduce of [cost|gradT|gradC] per step). */
int isdf_set_shard(isdf_ctx *ctx, int rank, int world_size);

/* ---- once-per-plan map products, built on the device ------------------------------------------------------------ */
/* Point cloud -> occupancy grid (PCSmapManager::rcvGlobalMapHandler, src/map_manager/src/PCSmap_manager.cpp:87-200):
 * xyz = n_points x 3 floats (pcl::PointXYZ).  bmin/bmax NULL => the tight box of the cloud ("measure boundary",
 * :110-141).  Grid size ceil((max-min)/res) (Gridmap3D.cpp:29-31); a voxel is occupied iff it collected >=
 * sta_threshold points; points outside the box count for voxel (0,0,0) like getGridIndex does (:137-140).
 * Replaces any grid set before.  dims_out (nullable) receives nx, ny, nz. */
int isdf_set_pointcloud(isdf_ctx *ctx, const float *xyz, long long n_points, const double *bmin, const double *bmax,
                        double resolution, int sta_threshold, int dims_out[3]);
/* Occupancy -> unsigned ESDF in metres (GridMap3D::generateESDF3d, Gridmap3D.cpp:361-414: the exact Euclidean distance
 * to the nearest occupied voxel centre, res*sqrt(d2)); installs it as the ISDF_GRID_ESDF grid (float32). */
int isdf_generate_esdf(isdf_ctx *ctx);
/* Download a grid (out may be NULL to query the geometry only).  dtype must be ISDF_F32 for the ESDF, ISDF_U8 for the
 * occupancy grid. */
int isdf_get_grid(isdf_ctx *ctx, int grid_kind, void *out, int dtype, int dims_out[3], double origin_out[3], double bmax_out[3]);
/* Obstacle-point set of the swept-volume sweep (plan_manager.cpp:232-254): for every waypoint, the occupied voxel
 * centres inside the box [w - half + offset, w + half + offset] that are outside the previous waypoint's box
 * [w_prev - half, w_prev + half] (getPointsInAABBOutOfLastOne, PCSmap_manager.h:182-216; the first "previous" is
 * (999,999,999)), united over the waypoints.  Installs the set like isdf_set_points (ordered by voxel index; the
 * reference's unordered_map order is unspecified) and resets lastTstar to 0.  offset may be NULL. */
int isdf_gather_points(isdf_ctx *ctx, const double *waypoints, int n_waypoints, const double half[3], const double *offset,
                       int *M_out);
/* Copies up to `capacity` points (M x 3 row-major) and returns M (>= 0), or a negative isdf_status. */
int isdf_get_points(isdf_ctx *ctx, double *xyz_out, int capacity);

/* The environment ESDF sampled at n WORLD points (xyz: n x 3 row-major): value_out[i] = GridMap3D::getSDFValue(pos)
 * (src/map_manager/include/map_manager/GridMap3D.h:114-146), grad_out[i] (n x 3) the analytic gradient of the trilinear interpolant
 * as getSDFValueWithGrad returns it (:155-193) - including the reference's quirks: base cell of pos - res/2, a position outside
 * the map reads cell (0,0,0) (Gridmap3D.cpp:137-140), an invalid corner reads 0 (:535-542).  Needs an ESDF grid (isdf_set_grid
 * with ISDF_GRID_ESDF, or isdf_generate_esdf).  Either output may be NULL.  Bit for bit the reference's doubles on the float32
 * grid.  The _device form takes device pointers and a stream (asynchronous). */
int isdf_esdf_sample(isdf_ctx *ctx, const double *xyz, long long n, double *value_out, double *grad_out);
int isdf_esdf_sample_device(isdf_ctx *ctx, const double *d_xyz, long long n, double *d_value_out, double *d_grad_out, void *stream);
/* The same for points in NO particular order (a point cloud, random queries): sampled from a bricked copy of the ESDF - 2 x 2 x 2-cell
 * bricks with their one-voxel apron, one 128-byte line each, so the eight corners of any cell come from ONE line instead of four
 * z-rows (4x the grid's memory, built once per map on first use).  Same arithmetic on the same values: results bit for bit those
 * of isdf_esdf_sample.  Points along a trajectory are better served by the plain form (neighbours share their lines). */
int isdf_esdf_sample_scattered(isdf_ctx *ctx, const double *xyz, long long n, double *value_out, double *grad_out);
int isdf_esdf_sample_scattered_device(isdf_ctx *ctx, const double *d_xyz, long long n, double *d_value_out, double *d_grad_out, void *stream);

/* The installed robot shape by itself, on n BODY-FRAME points (p_rel: n x 3 row-major): sdf_out[i] =
 * BasicShape::getonlySDF(pos_rel) and grad_out[i] (n x 3) = getonlyGrad1(pos_rel) (Shape.hpp:32-57: central difference
 * dx = 5e-6, normalised; Box :2363-2377; Ball :622-625; mesh Generalshape Shape.cpp:105-139: (1 - 2 w) * distance with
 * w = igl::fast_winding_number(fwn_bvh, 2.0, ...)).  Either output may be NULL.  Evaluated on the device. */
int isdf_shape_eval(isdf_ctx *ctx, const double *p_rel, int n, double *sdf_out, double *grad_out);

/* The float atan2 inside the mesh kind's winding number, evaluated on the HOST (no device needed; for tests): the reference's
 * UTsignedSolidAngleTri ends in the C library's atan2f (FastWindingNumberForSoups.h:325-326, :6083) and the swept-volume
 * argmin is sensitive to its last bit, so the device restates glibc's algorithm (sysdeps/ieee754/flt-32/e_atan2f.c,
 * s_atanf.c) operation for operation; out[i] = that function at (y[i], x[i]). */
int isdf_mesh_atan2f(const float *y, const float *x, long long n, float *out);

/* ---- per-step evaluation ----------------------------------------------------------------------------------- */
/* Host entry point, synchronous, drop-in for the reference sweeps.  n_traj trajectories (1 in the reference);
 * N[b] pieces each; T[b] -> N[b] doubles; coeffs[b] -> 6N[b] x 3 column-major.
 * cost_inout[b], gradT_inout[b][..], gradC_inout[b][..] are ACCUMULATED.  tstar_inout (V1 only, may be NULL,
 * n_traj == 1): lastTstar[M], read and written like TrajOptimizer::lastTstar (:59-62, :576-578). */
int isdf_eval(isdf_ctx *ctx, int n_traj, const int *N, const double *const *T,
              const double *const *coeffs, double *cost_inout, double *const *gradT_inout,
              double *const *gradC_inout, double *tstar_inout);

/* How the LAST host-array step (isdf_eval, isdf_cost_function) crossed PCIe - for callers that want to know which of the
 * boundary's latencies they are getting (INTEGRATION.md "Boundary cost"):
 *   COPY           one H2D copy, the launches, one D2H copy, one stream synchronisation (batches, V1, mesh robots, small-BAR
 *                  systems with ISDF_NO_HOST_DIRECT=1, any step that is not one fused launch)
 *   DIRECT_MAPPED  ONE launch: its first workgroups fetch the inputs from host-mapped memory, its last store the results and a
 *                  completion flag into host-mapped memory (no large PCIe BAR, or ISDF_NO_BAR_WRITES=1)
 *   DIRECT_BAR     ONE launch: the CPU has written the inputs straight into device memory through the PCIe BAR (verified per
 *                  ctx by a kernel-visible probe), results and flag as above
 * The three environment switches ISDF_NO_HOST_DIRECT / ISDF_NO_BAR_WRITES / ISDF_NO_FUSE are read once per ctx, in isdf_create.
 * Replaces nothing in the reference (its sweeps run in the caller's address space). */
#define ISDF_HOST_PATH_COPY 0
#define ISDF_HOST_PATH_DIRECT_MAPPED 1
#define ISDF_HOST_PATH_DIRECT_BAR 2
/*   DEVICE_CALLBACK  isdf_cost_function with its MINCO half on the device: x goes down (through the BAR, or fetched from
 *                  host-mapped memory), (cost, g) and a completion word come back into host-mapped memory; no copy commands */
#define ISDF_HOST_PATH_DEVICE_CALLBACK 3
int isdf_host_path(const isdf_ctx *ctx);
/* The DIRECT_* and DEVICE_CALLBACK hand-overs end with the kernel storing results and then a completion word into host-mapped
 * memory.  Those are separate PCIe writes from different wavefronts: the word can be visible to the CPU before every result is
 * (seen on MI355X for the FIRST step of a ctx, about one fresh process in twenty: cost and word there, the gradient rows still
 * zero).  The host therefore fills the result area with an all-ones pattern no result can have before the launch and, once the
 * word is there, waits until none of it is left.  info_out: [0] hand-overs so far, [1] how many of them had results still
 * missing when the word arrived, [2] polls spent waiting for those; [3..7] reserved (0). */
int isdf_host_info(const isdf_ctx *ctx, int64_t info_out[8]);
/* Developer entry: the bytes the library's own buffers hold at this moment, process-wide - out[0] device memory, out[1] pinned
 * host memory (every ctx, every scratch and temporary; not the exchange's IPC mailbox, not the A* table).  Both return to
 * what they were once every ctx created since has been destroyed. */
void isdf_debug_live_bytes(long long out[2]);
/* ... and the HIP events the library holds at this moment, process-wide, under the same rule. */
long long isdf_debug_live_events(void);

/* Device-resident entry point, asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 * stream).  All trajectories have N pieces.  d_T: n_traj*N, d_coeffs: n_traj * (6N x 3 col-major),
 * d_out: n_traj * (1 + N + 18N) doubles, OVERWRITTEN with [cost | gradT | gradC(col-major)] per trajectory
 * (shard-partial sums when a shard is set).  d_tstar: V1 only, M doubles, may be NULL.
 * Results change hands between workgroups through self-resetting slots behind BOUNDED waits (forward progress of a launch is
 * not something the hardware contract promises): a wait that expires never hangs the stream - it raises the overflow word
 * and leaves a NaN cost.  isdf_eval reports that as ISDF_ERR_OVERFLOW by itself; a caller of THIS entry point must look:
 * a non-finite d_out[0], or isdf_get_stats(...).overflow != 0 (reading it drains the device, clears the word and empties
 * every slot again, so that a producer that published late cannot feed the next step; the in-kernel exchange of a
 * multi-GPU step should be switched off after an overflow, isdf_xchg_fuse(ctx, 0)).
 * Steps of one ctx share its scratch (result slots, the dispatch order the device derives from earlier steps): they have to
 * execute one after the other - the same stream, or streams ordered by events as isdf_optimize_lbfgs_batch does. */
int isdf_eval_device(isdf_ctx *ctx, int n_traj, int N, const double *d_T, const double *d_coeffs,
                     double *d_out, double *d_tstar, void *stream);
size_t isdf_out_stride(int N);   /* 1 + N + 18N */
/* The swept-volume sweep with the minimisers GIVEN instead of searched for: obstacle point k is evaluated at time
 * d_tstar[k] (M doubles on the device; a negative or NaN entry means "no time interval qualified": min sdf = 10, no penalty,
 * sw_manager.hpp:717) - i.e. lines :578-646 of addSaftyPenaOnSweptVolumeParallel after getSDFofSweptVolume returned
 * (getSDFAtTimeStamp sw_manager.hpp:550-556 + getGradPrelAtTimeStamp :566-572 at that time).  Same output as
 * isdf_eval_device; the ctx's internal lastTstar takes the given values.  Use: re-evaluating cost / gradient at minimisers found elsewhere (the
 * argmin over t is a chain of accept/reject comparisons; this entry point isolates the arithmetic behind it). */
int isdf_eval_swept_at_tstar(isdf_ctx *ctx, int N, const double *d_T, const double *d_coeffs, double *d_out,
                             const double *d_tstar, void *stream);
/* the same with host arrays, synchronous, ACCUMULATING into cost / gradT[N] / gradC[18N] like isdf_eval (tstar: M doubles) */
int isdf_eval_swept_at_tstar_host(isdf_ctx *ctx, int N, const double *T, const double *coeffs, const double *tstar,
                                  double *cost_inout, double *gradT_inout, double *gradC_inout);

/* ---- swept-volume field and mesh ------------------------------------------------------------------------------ */
/* The swept-volume SDF of a trajectory at arbitrary points: getSDFofSweptVolume (sw_manager.hpp:710-747) per point, the
 * query the V1 collision term binds, with the ctx's shape (any kind) and config (safety_hor, flatness constants), on any
 * single-device ctx whatever cfg.variant is (a multi-device ctx: ISDF_ERR_UNSUPPORTED).  The trajectory is passed as
 * isdf_eval takes it: N durations, 6N x 3 column-major coefficients; a total of 300 s or more is ISDF_ERR_INVALID_ARG.
 *   PLANNER  exactly the collision term's query: coarse 0.2 s table, qualification sdf < 2 safety_hor + 0.1, quirks q1-q3,
 *            the 0.02 s fine scan and the sign descent.  A point with no qualifying interval reads value 10, t* = -1.
 *   CLOSED   the same with the trajectory's end included: one more coarse sample at t = duration, and a run still in range
 *            after it is kept (upper bound = duration) instead of dropped.  Where all of a point's in-range runs close before
 *            the end it equals PLANNER bit for bit; elsewhere it is <= PLANNER.  The mesh needs it (end cap, short trajectories).
 * The query has scratch of its own: the V1 step's points, lastTstar, duration state, dispatch records and overflow word are
 * not touched.  Points go through in chunks (1.5 KB of interval slots each), so millions can be queried.  A point with more
 * than 32 intervals: ISDF_ERR_OVERFLOW.  tstar_out may be NULL.  The device form synchronises `stream` before it returns. */
#define ISDF_SWEPT_FIELD_PLANNER 0
#define ISDF_SWEPT_FIELD_CLOSED  1
int isdf_swept_sdf(isdf_ctx *ctx, int N, const double *T, const double *coeffs, const double *xyz, long long n,
                   int mode, double *value_out, double *tstar_out);
int isdf_swept_sdf_device(isdf_ctx *ctx, int N, const double *d_T, const double *d_coeffs, const double *d_xyz,
                          long long n, int mode, double *d_value_out, double *d_tstar_out, void *stream);
/* The surface mesh of the swept volume (sw_calculate::calculation / getmesh, reached from calculateSwept sw_manager.hpp:225-237):
 * the field above on a lattice of spacing eps, marching tetrahedra on the Kuhn split (six tetrahedra per cell around its main
 * diagonal).  Inside is f < iso; a vertex lies on a lattice edge (7 per node: +x +y +z +xy +xz +yz +xyz), placed by linear
 * interpolation; triangles face towards larger f (outwards).  Vertices are numbered by ascending edge id (node * 7 + dir, node
 * = (i * ny + j) * nz + k), triangles come in cell order (z fastest), then tetrahedron order: the output is bitwise
 * reproducible, and the narrow band gives the dense mesh.  Coordinates: node (i, j, k) lies at origin + i * eps per axis, and the
 * vertex of the edge from node p in direction d (offsets 0 / 1 per axis) at p + t * (d * eps) with t = (iso - f0) / (f1 - f0),
 * f0 = f(p), f1 = f(p + d) - each operation rounded on its own (no fused multiply-add).  A vertex exists where f0 < iso differs
 * from f1 < iso and the edge lies in a cell whose eight corners were all evaluated.
 * Box: use_bbox, or the trajectory's positions grown by R + iso + 2 eps (R: bound_radius of the shape; mesh robots: their
 * largest vertex norm; none known: ISDF_ERR_INVALID_ARG), snapped to multiples of eps; more than 2^27 lattice nodes:
 * ISDF_ERR_INVALID_ARG.  Narrow band (band = B > 0): the field on every B-th node, then on the nodes of the coarse cells whose
 * corners change sign about iso or all lie within lipschitz * sqrt(3) * B * eps of it - a corner farther away proves the cell's
 * side of iso (exact for a field with that Lipschitz bound; a corner without a qualifying interval, value 10, counts as the
 * value 2 safety_hor + 0.1 there: that it is not within the qualification radius is all it proves); band = 0 evaluates every
 * node. */
typedef struct isdf_swept_mesh_params {
    double eps;          /* lattice spacing (m), > 0 (the reference's yaml eps: 0.05-0.15); default 0.1                */
    double iso;          /* level to extract, >= 0 (0 = the swept volume, > 0 = an inflated one); default 0           */
    int32_t mode;        /* ISDF_SWEPT_FIELD_CLOSED (default) or ISDF_SWEPT_FIELD_PLANNER                              */
    int32_t band;        /* coarse factor B of the narrow band (default 4); 0 = evaluate every lattice node            */
    double lipschitz;    /* bound L on the field's Lipschitz constant, > 0, used to cull coarse cells (default 1)      */
    int32_t use_bbox;    /* nonzero: the lattice covers [bmin, bmax] (snapped outwards to eps) instead of the derived box */
    int32_t reserved;
    double bmin[3], bmax[3];
} isdf_swept_mesh_params;
typedef struct isdf_swept_mesh_info {
    int32_t dims[3];             /* lattice nodes per axis                                                              */
    int32_t reserved;
    double origin[3];            /* position of node (0, 0, 0)                                                          */
    double eps;
    int64_t coarse_points;       /* field queries on the coarse lattice (0 without a band)                              */
    int64_t fine_points;         /* field queries of the fine batch (every node without a band)                         */
    int64_t band_cells;          /* lattice cells with all eight corners evaluated (the cells the extraction visits)     */
    int64_t n_vertices, n_triangles;
    int64_t unqualified_edges;   /* sign-changing edges with an end that found no qualifying interval (value 10): nonzero
                                    means the qualification radius 2 safety_hor + 0.1 was too small for this iso         */
    double field_ms, mesh_ms;    /* device time of the field queries / of the extraction (events on the ctx's stream)    */
} isdf_swept_mesh_info;
void isdf_swept_mesh_params_default(isdf_swept_mesh_params *p);
/* builds the mesh on the device and keeps it in the ctx (replacing the previous one); T / coeffs are host arrays */
int isdf_swept_mesh_build(isdf_ctx *ctx, int N, const double *T, const double *coeffs,
                          const isdf_swept_mesh_params *p, isdf_swept_mesh_info *info_out);
/* copies the last mesh out: V_out capV x 3, F_out capF x 3 (zero based); ISDF_ERR_OVERFLOW (nothing written) if too small */
int isdf_swept_mesh_get(isdf_ctx *ctx, double *V_out, int capV, int32_t *F_out, int capF);
int isdf_swept_mesh_release(isdf_ctx *ctx);      /* frees the kept mesh */
/* marching tetrahedra (the rule of isdf_swept_mesh_build) on a caller's field: f[(i*ny + j)*nz + k], host array, NaN = node not
 * evaluated (a cell with such a corner is skipped, as in the narrow band).  Needs a ctx only: no shape, grid or trajectory.
 * dims >= 2 per axis, at most 2^27 nodes, eps finite and > 0, iso finite (negative allowed), no null pointer - else
 * ISDF_ERR_INVALID_ARG.  Result kept and fetched like the swept mesh (isdf_swept_mesh_get / _release); info: dims, origin, eps,
 * band_cells, n_vertices, n_triangles, unqualified_edges, mesh_ms; the field counters are 0. */
int isdf_lattice_mesh_build(isdf_ctx *ctx, const int32_t dims[3], const double origin[3], double eps, double iso,
                            const double *f, isdf_swept_mesh_info *info_out);

/* ---- trajectory clearance check -------------------------------------------------------------------------------- */
/* SweptVolumeManager::isTrajCollide (sw_manager.hpp:764: a stub, "currently always returns false"), the verdict generateTraj asks
 * for once the back end has finished (plan_manager.cpp, end of generateTraj): how close the swept volume of a trajectory comes to
 * any occupied voxel centre of the WHOLE map - not only to the points isdf_gather_points collected around the A* path.
 * The map is the ctx's occupancy grid (isdf_set_grid with ISDF_GRID_OCCUPANCY, or isdf_set_pointcloud; none:
 * ISDF_ERR_INVALID_ARG); obstacle points are voxel centres (index + 0.5) * res + origin, each operation rounded on its own.  The
 * trajectory is passed as isdf_eval takes it.  Rules as for isdf_swept_sdf: any single-device ctx whatever cfg.variant is, a
 * multi-device ctx ISDF_ERR_UNSUPPORTED, 300 s or more ISDF_ERR_INVALID_ARG, a point with more than 32 intervals
 * ISDF_ERR_OVERFLOW; own scratch - the V1 step's points, lastTstar, duration state and the kept swept mesh are not touched.
 * Three steps on the device: the occupied voxels within far_r = R + (2 safety_hor + 0.1) of some coarse (0.2 s)
 * sample of the trajectory (R: isdf_shape.bound_radius; mesh robots: their largest vertex norm, band x 1.05) are selected in
 * ascending voxel index - every other point reads 10 / -1 from the field query, so nothing is lost; a shape without a radius
 * takes every occupied voxel (culled = 0) -, put through the field query in `mode`, and reduced.  The report is the field
 * query's answer at voxel centres, bit for bit and the same bytes on every run; it is not a continuous certificate between them. */
typedef struct isdf_traj_check_params {
    double margin;       /* level below which a point is reported; negative (default) = cfg.safety_hor, the level below which the
                            V1 term charges; above 2 safety_hor + 0.1 the query cannot answer: ISDF_ERR_INVALID_ARG            */
    int32_t mode;        /* ISDF_SWEPT_FIELD_PLANNER (default: the collision term's own query) or ISDF_SWEPT_FIELD_CLOSED       */
    int32_t reserved;
} isdf_traj_check_params;
typedef struct isdf_traj_check_info {
    int64_t occupied_in_box;     /* occupied voxels of the selection box (the samples' box grown by far_r; all of the grid if !culled) */
    int64_t candidates;          /* voxels put through the field query                                                         */
    int64_t qualified;           /* candidates with a qualifying interval (value != 10)                                        */
    int64_t n_below_margin;      /* qualified candidates with value < margin: the rows isdf_traj_check_get returns             */
    int64_t n_penetrating;       /* ... with value < 0                                                                         */
    double min_clearance;        /* smallest value (10: nothing qualified); ties go to the lowest voxel index                  */
    double min_tstar;            /* its t* (-1: nothing qualified)                                                             */
    double min_point[3];         /* its voxel centre                                                                           */
    int64_t min_voxel;           /* its voxel index (x * ny + y) * nz + z (-1: nothing qualified)                              */
    int32_t min_piece;           /* the piece min_tstar lies in (Trajectory::locatePieceIdx; -1: nothing qualified)            */
    int32_t culled;              /* 1: candidates selected by the bounding sphere; 0: the shape has none, every occupied voxel  */
    double margin, far_r;        /* the margin in force; the selection radius (0 if !culled)                                   */
    double select_ms, field_ms, reduce_ms;       /* device time of the three steps (events on the stream)                      */
} isdf_traj_check_info;
void isdf_traj_check_params_default(isdf_traj_check_params *p);
/* params NULL = defaults.  piece_min_out (N doubles or NULL): per piece the smallest value among the points whose t* lies in it
 * (10: none).  The points below the margin are kept in the ctx (replacing the previous check's) until released. */
int isdf_traj_check(isdf_ctx *ctx, int N, const double *T, const double *coeffs, const isdf_traj_check_params *params,
                    isdf_traj_check_info *info_out, double *piece_min_out);
/* the same with the trajectory (and the per-piece array, or NULL) on the device; synchronises `stream` before it returns */
int isdf_traj_check_device(isdf_ctx *ctx, int N, const double *d_T, const double *d_coeffs, const isdf_traj_check_params *params,
                           isdf_traj_check_info *info_out, double *d_piece_min_out, void *stream);
/* the last check's points below the margin in voxel order, rows_out capacity x 5: (x, y, z, value, t*); ISDF_ERR_OVERFLOW
 * (nothing written) if capacity < n_below_margin */
int isdf_traj_check_get(isdf_ctx *ctx, double *rows_out, long long capacity);
int isdf_traj_check_release(isdf_ctx *ctx);      /* frees the kept rows */
/* isTrajCollide (sw_manager.hpp:764) as plan_manager.cpp calls it: 1 = some occupied voxel centre lies inside the swept volume
 * (n_penetrating > 0 at the default parameters), 0 = none, negative = isdf_status */
int isdf_traj_collide(isdf_ctx *ctx, int N, const double *T, const double *coeffs);

/* ---- the kept report folded across map updates ---------------------------------------------------------------- */
/* Occupancy only grows under isdf_update_* (isdf_clear_pointcloud / isdf_clear_voxels take voxels out and re-check an armed watch
 * against the whole map instead, see there), the field query answers every point on its own, and every quantity of the report is a
 * sum, a minimum or a voxel-ordered list.  So the check on an updated map is the kept report of the old map merged with a report over only the voxels
 * the update made occupied - the same bytes as isdf_traj_check on the updated map, for work proportional to the update.
 * isdf_traj_check_set_watch: mode 0 (default) - an update leaves the kept report alone (stale, its voxel ids still valid); mode 1 -
 * every successful isdf_traj_check[_device] (those of isdf_optimize_lbfgs_checked, the retiming and the re-allocation included) arms a
 * watch: the ctx keeps the trajectory, the margin and mode in force, the report, the N piece minima and the rows with their voxel
 * ids, and from then on every isdf_update_pointcloud / isdf_update_voxels that occupies a voxel folds the new voxels in, on both of
 * the update's paths, on the ctx's stream after the map products and the field repair of the same call.  Afterwards
 * isdf_traj_check_get, isdf_points_merge_check and isdf_traj_check_watch_info answer as after isdf_traj_check on the updated map.  An
 * update that occupies nothing folds nothing.  The watch is disarmed by isdf_traj_check_release, by isdf_set_grid /
 * isdf_set_pointcloud, by a new shape or shape program, and by a failing step of the fold - the update then fails as a whole, as a
 * failing field repair makes it, and the kept report is dropped, never left half-merged.  The mode outlives the check.
 * Other modes: ISDF_ERR_INVALID_ARG; a multi-device ctx: ISDF_ERR_UNSUPPORTED. */
int isdf_traj_check_set_watch(isdf_ctx *ctx, int mode);
typedef struct isdf_traj_watch_info {
    int64_t updates_folded;      /* updates folded into the report since the watch was armed                                      */
    int64_t new_voxels;          /* the last folded update: voxels it occupied                                                    */
    int64_t new_in_box, new_candidates, new_qualified, new_below_margin, new_penetrating;   /* ... their share of the report's sums */
    double new_min_clearance;    /* the minimum over the NEW voxels alone (10: none qualified) ...                                */
    double new_min_tstar;        /* ... its t* (-1), voxel index (-1) and piece (-1).  path 2: those of the report when min_changed, */
    int64_t new_min_voxel;       /*     else 10 / -1 / -1 / -1 (the whole map was checked, not the new voxels apart)              */
    int32_t new_min_piece;
    int32_t path;                /* 0 nothing folded yet; 1 the new voxels came from the update's list; 2 the kept trajectory was  */
                                 /*   checked against the whole map again (the update's list was cut at max_new_voxels)           */
    int32_t min_changed;         /* 1: the folded global minimum came from this update                                            */
    int32_t reserved;
    double select_ms, field_ms, reduce_ms, merge_ms;     /* device time of the fold's steps (events on the ctx's stream)          */
} isdf_traj_watch_info;
/* The current folded report, the N piece minima of the watched trajectory (piece_min_out may be NULL) and the record of the last
 * fold (last_out may be NULL).  ISDF_ERR_STATE when no watch is armed. */
int isdf_traj_check_watch_info(isdf_ctx *ctx, isdf_traj_check_info *report_out, double *piece_min_out, isdf_traj_watch_info *last_out);
void isdf_traj_check_watch_sizes(int sizes_out[1]);      /* sizeof of the struct above, for mirrors of this header              */
/* The merge rule in plain host code, no ctx and no device: two reports over DISJOINT voxel sets of one trajectory of N pieces - info
 * words, N piece minima (NULL: all 10), n_below_margin rows of 5 doubles and their ascending voxel ids each - into the report of the
 * union.  Integer sums add; the minimum is the lexicographic (value, voxel index) with -1 for "none"; piece minima are element-wise
 * minima; rows interleave by ascending voxel id; culled, margin, far_r and the times are a's.  rows_out / vox_out hold `capacity`
 * rows (ISDF_ERR_OVERFLOW if fewer than the sum; both may be NULL when the sum is 0).  Lists that are not ascending or share an id:
 * ISDF_ERR_INVALID_ARG.  The device fold calls the same functions (csrc/traj_watch_host.hpp). */
int isdf_traj_check_fold_host(int N, const isdf_traj_check_info *a, const double *piece_min_a, const double *rows_a, const int64_t *vox_a,
                              const isdf_traj_check_info *b, const double *piece_min_b, const double *rows_b, const int64_t *vox_b,
                              isdf_traj_check_info *out, double *piece_min_out, double *rows_out, int64_t *vox_out, long long capacity);

/* ---- dynamic limits of a trajectory -------------------------------------------------------------------------------- */
/* The back end keeps the vehicle inside vmax / omgmax / thetamax only through soft penalties at K + 1 samples per piece
 * (back_end_optimizer.hpp:453-536), so a finished trajectory can exceed them, between the samples or at them.  These entry
 * points say by how much: the counterpart of Trajectory::getMaxVelRate / getMaxAccRate / checkMaxVelRate / checkMaxAccRate
 * (trajectory.hpp:253-390, :631-680) extended to the body rate, tilt and thrust of the flatness map, and of the per-time
 * state SweptVolumeManager::getStateOnTrajStamp (sw_manager.hpp:307-341) hands out.  Conventions of the penalty: psi = 0, the
 * vehicle constants of the ctx's isdf_config, pieces located by Trajectory::locatePieceIdx (trajectory.hpp:545-563: a junction
 * time belongs to the earlier piece, a stamp below 0 is evaluated on the first piece and one above sum(T) on the last),
 * trajectory arrays as isdf_eval takes them.
 *
 * Channels:  0 speed |vel|   1 acceleration |acc|   2 body rate |omg| of optimizated_forward (flatness.hpp:88-148)
 *            3 tilt acos(1 - 2 (q1^2 + q2^2)) (back_end_optimizer.hpp:505-508)
 *            4 largest / 5 smallest thrust `thr` of FlatnessMap::forward (flatness.hpp:203-206)
 *
 * isdf_traj_sample: the state at n time stamps, rows of ISDF_TRAJ_SAMPLE_ROW doubles pos3 | vel3 | acc3 | jer3 | quat4 | omg3 | thr.
 *
 * isdf_traj_limits: per piece and channel, `samples` + 1 uniform coarse samples; a golden-section search starts on
 * [s_(j-1), s_(j+1)] at every interior sample that is no smaller than both neighbours and, with one-sided brackets, at both end
 * samples, and stops when its bracket is shorter than tol_t * T_i (64 iterations at most).  Its result is the largest value it
 * EVALUATED with the time of that evaluation, never an interval midpoint; a piece reports the largest result (ties: the smallest
 * time), a trajectory the largest piece (ties: the smallest time, then the earlier piece).  Channels 0-2 are maximised in squared
 * form and reported as the square root, channel 5 is channel 4 minimised.  The report is therefore a LOWER bound of the true
 * extremum that is never below a coarse sample: a peak narrower than two coarse intervals can be missed, and it is no
 * certificate between the evaluated times.  Same bytes on every run; a trajectory's rows do not depend on its place in a batch.
 * Any single-device ctx whatever cfg.variant is; a multi-device ctx ISDF_ERR_UNSUPPORTED; N < 1, a null array or a duration that
 * is not positive and finite ISDF_ERR_INVALID_ARG.  Own scratch (grows only): the step's state, lastTstar, the kept clearance
 * rows and the swept mesh are not touched.  Two launches per call for any B.  A report costs what its longest
 * chain of dependent evaluations costs, about a millisecond on the device whatever N is: for ONE trajectory of a few dozen pieces
 * isdf_traj_limits_host on one thread is as fast or faster; the device forms pay off for hundreds of pieces, for batches, and
 * where the trajectory already lives on the device. */
#define ISDF_LIMITS_CHANNELS 6
#define ISDF_LIMIT_SPEED 0
#define ISDF_LIMIT_ACC 1
#define ISDF_LIMIT_OMG 2
#define ISDF_LIMIT_TILT 3
#define ISDF_LIMIT_THRUST_MAX 4
#define ISDF_LIMIT_THRUST_MIN 5
#define ISDF_TRAJ_SAMPLE_ROW 20
typedef struct isdf_traj_limits_params {
    int32_t samples;     /* coarse intervals per piece; <= 0 (default): 4 * cfg.integral_intervs                                  */
    int32_t reserved;
    double tol_t;        /* a search stops when its bracket is shorter than tol_t * T_i; <= 0 or NaN (default 2^-26): 2^-26         */
    double max_acc, max_thrust, min_thrust;      /* limits of channels 1, 4, 5; NaN (default): not judged.  Channels 0, 2, 3 are
                                                    judged against cfg.vmax, cfg.omgmax, cfg.thetamax                             */
} isdf_traj_limits_params;
typedef struct isdf_traj_limits_info {
    double value[ISDF_LIMITS_CHANNELS];          /* the extreme value of the channel                                              */
    double time[ISDF_LIMITS_CHANNELS];           /* the global time it was evaluated at                                           */
    double limit[ISDF_LIMITS_CHANNELS];          /* the limit in force (NaN: not judged)                                          */
    int32_t piece[ISDF_LIMITS_CHANNELS];         /* the piece it lies in                                                          */
    int32_t n_pieces_over[ISDF_LIMITS_CHANNELS]; /* pieces whose own extreme value is STRICTLY beyond the limit (0: not judged)   */
    int32_t judged;      /* bit ch: the channel has a limit                                                                        */
    int32_t feasible;    /* bit ch: it has one and value[ch] is not strictly beyond it; all is well when feasible == judged        */
    int32_t samples;     /* the coarse intervals per piece in force                                                                */
    int32_t reserved;
    double tol_t;        /* the tolerance in force                                                                                 */
    double device_ms;    /* device time of the launches (events on the stream); 0 for the host form                               */
} isdf_traj_limits_info;
void isdf_traj_limits_params_default(isdf_traj_limits_params *p);
/* params NULL = defaults.  piece_out (N x 12 doubles or NULL): per piece, [2 ch] the value and [2 ch + 1] the global time of channel ch */
int isdf_traj_limits(isdf_ctx *ctx, int N, const double *T, const double *coeffs, const isdf_traj_limits_params *params,
                     isdf_traj_limits_info *info_out, double *piece_out);
/* the same with the trajectory (and the per-piece array, or NULL) on the device; synchronises `stream` before it returns */
int isdf_traj_limits_device(isdf_ctx *ctx, int N, const double *d_T, const double *d_coeffs, const isdf_traj_limits_params *params,
                            isdf_traj_limits_info *info_out, double *d_piece_out, void *stream);
/* B trajectories of N pieces each (T: B x N, coeffs: B x 6N x 3 column-major each, host arrays) -> B infos, piece_out B x N x 12 or NULL */
int isdf_traj_limits_batch(isdf_ctx *ctx, int B, int N, const double *T, const double *coeffs, const isdf_traj_limits_params *params,
                           isdf_traj_limits_info *infos_out, double *piece_out);
/* the same rules in plain host code: needs no ctx and no device (csrc/traj_limits_host.hpp); agrees with the device to rounding */
int isdf_traj_limits_host(const isdf_config *cfg, int N, const double *T, const double *coeffs, const isdf_traj_limits_params *params,
                          isdf_traj_limits_info *info_out, double *piece_out);
/* rows_out: n x ISDF_TRAJ_SAMPLE_ROW */
int isdf_traj_sample(isdf_ctx *ctx, int N, const double *T, const double *coeffs, long long n, const double *t, double *rows_out);
int isdf_traj_sample_device(isdf_ctx *ctx, int N, const double *d_T, const double *d_coeffs, long long n, const double *d_t,
                            double *d_rows_out, void *stream);
int isdf_traj_sample_host(const isdf_config *cfg, int N, const double *T, const double *coeffs, long long n, const double *t,
                          double *rows_out);
/* sizeof of the two structs above as the library was compiled (the Python mirror checks itself against them) */
void isdf_traj_limits_sizes(int out[2]);

/* ---- retiming a trajectory to its dynamic limits --------------------------------------------------------------------- */
/* What a caller can DO with an infeasible limits report: slow the whole trajectory down uniformly until the report is feasible.
 * The reference has no counterpart (trajectory.hpp:253-390, :631-680 only report).
 *
 * Scaling by s > 0:  T'_i = s * T_i, and the coefficient of t^k of every piece and axis becomes c_k / p_k with p_0 = 1,
 * p_k = p_(k-1) * s - plain IEEE operations, never contracted, so host and device give the same bytes and s = 1 returns the input
 * bit for bit.  The path keeps its geometry; speed falls as 1/s, acceleration as 1/s^2, jerk as 1/s^3, body rate, tilt and thrust
 * move towards hover.
 * Feasible at s, F(s):  feasible == judged in the report isdf_traj_limits* gives for the scaled arrays under params.limits - by
 * definition the existing entry point's report, no numerics of its own.
 * Ladder:  a round with bracket [a, b] evaluates `ladder` = L candidates s_0 = a, s_(L-1) = b exactly and
 * s_i = a + (b - a) * i / (L - 1) in between (the product, then the quotient, then the sum).
 * Pick:  i* = the smallest i such that F(s_j) holds for EVERY j >= i (a suffix, which guards against an F that is not monotone;
 * `nonmonotone` is set when any round saw a feasible candidate below an infeasible one).
 * Rounds:  round 0 uses [s_lo, s_hi].  F(s_hi) fails: status 2 (not reachable), the result is the candidate s_hi.  i* == 0 in
 * round 0: status 1, the result is s_lo.  Otherwise the next round's bracket is [s_(i*-1), s_(i*)], `rounds` rounds in all,
 * status 0.  The result is always an EVALUATED candidate; scale_below is the largest infeasible candidate evaluated below it (NaN:
 * none), so after R rounds scale - scale_below <= (s_hi - s_lo) / (L - 1)^R up to rounding.  A later round evaluates its
 * bracket's two ends again (the same bytes, the same verdict); `candidates` counts them.
 *
 * Errors as for isdf_traj_limits*, and ISDF_ERR_INVALID_ARG for: s_lo not positive or not finite, s_hi not finite or <= s_lo,
 * ladder outside 2..64, rounds outside 1..4, B * ladder * N above ISDF_TRAJ_RETIME_MAX_PIECES, check != 0 in the batch form.
 * check = 1 needs what isdf_traj_check needs (shape, occupancy grid, a total below 300 s at s_hi in the host-array form); its
 * absence is reported before anything is computed.  The result then goes through isdf_traj_check_device with the default
 * parameters (margin cfg.safety_hor, PLANNER mode) and the ctx keeps THAT check's rows: a slower vehicle tilts less, so the
 * clearance a planner found by tilting through a gap has to be looked at again.  Without check the kept rows, the step's points
 * and lastTstar are not touched.  The output arrays must not overlap the inputs.
 * On the device: 1 + 4 * rounds launches for any B, no host synchronisation between rounds, one at the end (with
 * check = 0); nothing is decided by an atomic; own scratch that grows only; the same bytes on every run; a trajectory's result
 * does not depend on its place in a batch.  The device forms report a duration that is not positive and finite only at that
 * one synchronisation (the outputs are then undefined). */
#define ISDF_TRAJ_RETIME_MAX_PIECES (1 << 20)
#define ISDF_RETIME_OK 0             /* scale is the smallest feasible candidate of the last round's ladder                    */
#define ISDF_RETIME_AT_LOWER 1       /* s_lo is feasible already (and every candidate above it): scale == s_lo                 */
#define ISDF_RETIME_NOT_REACHABLE 2  /* s_hi is not feasible: the result is the candidate s_hi, limits says what still binds    */
typedef struct isdf_traj_retime_params {
    double s_lo, s_hi;   /* round 0's bracket (defaults 1 and 8)                                                                    */
    int32_t ladder;      /* candidates per round, 2..64 (default 32)                                                                */
    int32_t rounds;      /* 1..4 (default 3)                                                                                        */
    int32_t check;       /* 1: the result goes through the clearance check (not in the batch form)                                  */
    int32_t reserved;
    isdf_traj_limits_params limits;
} isdf_traj_retime_params;
typedef struct isdf_traj_retime_info {
    double scale;        /* the factor of the returned arrays                                                                       */
    double scale_below;  /* the largest infeasible candidate evaluated below it (NaN: none)                                         */
    int32_t status;      /* ISDF_RETIME_*                                                                                           */
    int32_t rounds;      /* rounds that decided something for this trajectory (1 for status 1 and 2)                                */
    int32_t candidates;  /* limits reports that decided it: ladder * rounds (the device forms launch every round for every trajectory)      */
    int32_t nonmonotone; /* 1: some round saw a feasible candidate below an infeasible one                                          */
    int32_t binding;     /* bit ch: channel ch is judged and infeasible at scale_below (0: no scale_below)                          */
    int32_t checked;     /* 1: `check` is filled                                                                                    */
    double duration_in, duration_out;    /* the durations summed in order, before and after                                         */
    isdf_traj_limits_info limits;        /* the report at `scale` (device_ms: 0)                                                    */
    isdf_traj_check_info check;
    double device_ms;    /* device time of the launches without the check's (events on the stream); 0 for the host form             */
} isdf_traj_retime_info;
void isdf_traj_retime_params_default(isdf_traj_retime_params *p);
/* params NULL = defaults.  T_out: N, coeffs_out: 6N x 3 column-major (both required) */
int isdf_traj_retime(isdf_ctx *ctx, int N, const double *T, const double *coeffs, const isdf_traj_retime_params *params,
                     double *T_out, double *coeffs_out, isdf_traj_retime_info *info_out);
/* every array on the device; synchronises `stream` once, before it returns (check = 1: the check synchronises as it always does) */
int isdf_traj_retime_device(isdf_ctx *ctx, int N, const double *d_T, const double *d_coeffs, const isdf_traj_retime_params *params,
                            double *d_T_out, double *d_coeffs_out, isdf_traj_retime_info *info_out, void *stream);
/* B trajectories of N pieces each (host arrays, laid out as isdf_traj_limits_batch takes them): own brackets and status each */
int isdf_traj_retime_batch(isdf_ctx *ctx, int B, int N, const double *T, const double *coeffs, const isdf_traj_retime_params *params,
                           double *T_out, double *coeffs_out, isdf_traj_retime_info *infos_out);
/* the same rules in plain host code over isdf_traj_limits_host: no ctx, no device, params.check ignored */
int isdf_traj_retime_host(const isdf_config *cfg, int N, const double *T, const double *coeffs, const isdf_traj_retime_params *params,
                          double *T_out, double *coeffs_out, isdf_traj_retime_info *info_out);
/* the scaling alone */
int isdf_traj_scale_host(int N, const double *T, const double *coeffs, double s, double *T_out, double *coeffs_out);
/* sizeof of the two structs above as the library was compiled */
void isdf_traj_retime_sizes(int out[2]);

/* ---- re-allocating piece durations to the dynamic limits --------------------------------------------------------------- */
/* Uniform retiming lets the worst piece set the pace of the whole flight.  Re-allocation slows down only the pieces that are over
 * a limit, keeps the path points and solves MINCO again for the new durations, until the limits report is clean.
 * The reference has no counterpart: its back end holds vmax / omgmax / thetamax through soft penalties at K + 1 samples per piece
 * (back_end_optimizer.hpp:453-536) and its Trajectory class only reports (trajectory.hpp:253-390, :631-680).
 *
 * Inputs:  N pieces; head_pva[9] and tail_pva[9] = position | velocity | acceleration (3 each); the N - 1 inner waypoints Q,
 * point-major as isdf_pack_variables takes them (N = 1: not read, may be NULL); durations T[N].
 * Solve:  C(T) is the MINCO (s = 3) trajectory through Q with durations T and the given end states, in the junction-state form of
 * csrc/minco_pcr.hpp (junction rows, parallel cyclic reduction, quintic Hermite pieces): no gradient, no energy.
 * Evaluate:  the report isdf_traj_limits* gives for (T_k, C(T_k)) under params.limits - the existing rules, no numerics of its own.
 * Iterate k is feasible when feasible == judged.
 * Piece factor:  for piece i and a judged channel ch whose per-piece value is STRICTLY beyond its limit, rho = value / limit for
 * speed, body rate, tilt and largest thrust, sqrt(value / limit) for acceleration, limit / value for the smallest thrust when
 * value > 0 and f_max otherwise.  f_i = min(f_max, (1 + headroom) * max_ch rho), never below 1; f_i = 1 exactly when no channel of
 * the piece is over; a ratio that is NaN or infinite gives f_max.  A channel that is not judged is ignored.
 * Update:  T_(k+1),i = T_k,i * f_i - one product, never contracted.  Durations never shrink.
 * Rounds:  iterates k = 0 .. rounds are evaluated; the first feasible one is the result, status ISDF_REALLOC_OK and info.rounds = k
 * (k = 0: ISDF_REALLOC_ALREADY, T_out is T bit for bit).  Iterate `rounds` still infeasible: ISDF_REALLOC_NOT_REACHED, the result is
 * that iterate and info.limits says what still binds - isdf_traj_retime takes it from there.
 *
 * Errors as for isdf_traj_limits*, and ISDF_ERR_INVALID_ARG for: rounds outside 1..16, headroom negative or not finite, f_max not
 * finite or <= 1, check != 0 in the batch form, outputs overlapping inputs (host-array forms), N above 400 in the ctx forms (the
 * solve kernel's rows sit in LDS; isdf_traj_realloc_host takes any N).  check = 1 needs what isdf_traj_check needs (shape, occupancy
 * grid; in the host-array form a total below 300 s of the input): its absence is reported before anything is computed.  The path
 * between the waypoints moves when durations change, so the result then goes, still on the device, through isdf_traj_check_device
 * with the default parameters and the ctx keeps THAT check's rows; without check the kept rows are not touched.
 * On the device: at most 4 * (rounds + 1) launches for any B, nothing on the host between them, one synchronisation at the end (with
 * check = 0); nothing is decided by an atomic; own scratch that grows only; the same bytes on every run; a trajectory's result does
 * not depend on its place in a batch.  A trajectory that is done keeps its durations, and later rounds reproduce its bytes.  The
 * device forms report a duration that is not positive and finite only at that one synchronisation (the outputs are then
 * undefined).  The device solve and the host solve agree to rounding (the pin of minco_pcr.hpp: 1e-10 relative), not bit for bit. */
#define ISDF_TRAJ_REALLOC_MAX_ROUNDS 16
#define ISDF_TRAJ_REALLOC_MAX_N 400
#define ISDF_REALLOC_OK 0            /* iterate `rounds` >= 1 is the first feasible one                                        */
#define ISDF_REALLOC_ALREADY 1       /* the input's own durations are feasible: T_out is T bit for bit                          */
#define ISDF_REALLOC_NOT_REACHED 2   /* iterate params.rounds is still infeasible: it is the result, limits says what binds     */
typedef struct isdf_traj_realloc_params {
    int32_t rounds;      /* updates at most, 1..16 (default 8)                                                                      */
    int32_t check;       /* 1: the result goes through the clearance check (not in the batch form)                                  */
    double headroom;     /* eta >= 0 (default 0.02): a piece over a limit is slowed by (1 + eta) times its ratio                    */
    double f_max;        /* > 1 (default 2): the largest factor of one piece in one round                                           */
    isdf_traj_limits_params limits;
} isdf_traj_realloc_params;
typedef struct isdf_traj_realloc_info {
    int32_t status;      /* ISDF_REALLOC_*                                                                                          */
    int32_t rounds;      /* index k of the returned iterate = updates applied                                                       */
    int32_t pieces_changed;      /* pieces with T_out,i != T_i                                                                      */
    int32_t binding;     /* bit ch: channel ch was over its limit on some piece of some evaluated iterate                           */
    int32_t checked;     /* 1: `check` is filled                                                                                    */
    int32_t reserved;
    double duration_in, duration_out;    /* the durations summed in order, before and after                                         */
    double max_factor;   /* the largest T_out,i / T_i                                                                               */
    isdf_traj_limits_info limits;        /* the report of the returned arrays (device_ms: 0)                                        */
    isdf_traj_check_info check;
    double device_ms;    /* device time of the launches without the check's (events on the stream); 0 for the host form             */
} isdf_traj_realloc_info;
void isdf_traj_realloc_params_default(isdf_traj_realloc_params *p);
/* params NULL = defaults.  T_out: N, coeffs_out: 6N x 3 column-major (both required) */
int isdf_traj_realloc(isdf_ctx *ctx, int N, const double *head_pva, const double *tail_pva, const double *Q, const double *T,
                      const isdf_traj_realloc_params *params, double *T_out, double *coeffs_out, isdf_traj_realloc_info *info_out);
/* every array on the device; synchronises `stream` once, before it returns (check = 1: the check synchronises as it always does) */
int isdf_traj_realloc_device(isdf_ctx *ctx, int N, const double *d_head_pva, const double *d_tail_pva, const double *d_Q, const double *d_T,
                             const isdf_traj_realloc_params *params, double *d_T_out, double *d_coeffs_out,
                             isdf_traj_realloc_info *info_out, void *stream);
/* B trajectories of N pieces each (host arrays): heads B x 9, tails B x 9, Q B x (N - 1) x 3, T B x N; T_out B x N, coeffs_out
 * B x 6N x 3 column-major each; every trajectory has its own status */
int isdf_traj_realloc_batch(isdf_ctx *ctx, int B, int N, const double *heads, const double *tails, const double *Q, const double *T,
                            const isdf_traj_realloc_params *params, double *T_out, double *coeffs_out, isdf_traj_realloc_info *infos_out);
/* the same rules in plain host code over isdf_traj_limits_host and the host loops of csrc/minco_pcr.hpp: no ctx, no device, any N,
 * params.check ignored */
int isdf_traj_realloc_host(const isdf_config *cfg, int N, const double *head_pva, const double *tail_pva, const double *Q, const double *T,
                           const isdf_traj_realloc_params *params, double *T_out, double *coeffs_out, isdf_traj_realloc_info *info_out);
/* the solve alone: coeffs_out = C(T), 6N x 3 column-major */
int isdf_traj_minco_host(int N, const double *head_pva, const double *tail_pva, const double *Q, const double *T, double *coeffs_out);
/* sizeof of the two structs above as the library was compiled */
void isdf_traj_realloc_sizes(int out[2]);

/* ---- the clearance report merged into the obstacle-point set ---------------------------------------------------------- */
/* Where the reference only warns that the optimised trajectory collides (plan_manager.cpp:306-309), the report can be fed back:
 * the points the last isdf_traj_check* kept (value < its margin), narrowed to value < below (a negative `below`: all of them;
 * NaN / inf: ISDF_ERR_INVALID_ARG), are merged into the ctx's obstacle-point set on the device.  The set is keyed by
 * voxel id as the reference's aabb_points is (PCSmap_manager.h:182-216; gathered at plan_manager.cpp:232-254): a row is a
 * duplicate when ANY point of the set lies in its voxel (getGridIndex of the point, Gridmap3D.cpp:135-175); a point of the set
 * outside the grid occupies no voxel (n_outside).  Existing points keep their index, their bytes and their lastTstar; the new
 * ones are APPENDED in ascending voxel index with the report's centre bytes and lastTstar = 0 (plan_manager.cpp:254) - a
 * tstar_inout array of isdf_eval stays aligned with its first M_before entries.  n_added == 0 changes nothing; otherwise the
 * set counts as new exactly as after isdf_set_points (the per-point scratch of the V1 step grows at its next step).  The kept
 * report stays: a second merge finds every row a duplicate.  No point crosses PCIe, two merges from the same state give the
 * same bytes.  ISDF_ERR_STATE: no kept report (never checked, or released), or the occupancy grid was replaced after the check
 * (isdf_set_grid / isdf_set_pointcloud: the voxel ids are stale); multi-device ctx: ISDF_ERR_UNSUPPORTED. */
typedef struct isdf_points_merge_info {
    int32_t M_before, M_after;   /* size of the ctx's point set before / after                                   */
    int32_t n_rows;              /* kept report rows considered (value < below)                                   */
    int32_t n_added;             /* rows appended                                                                 */
    int32_t n_duplicate;         /* rows whose voxel already holds a point of the set                             */
    int32_t n_outside;           /* points of the existing set that lie outside the grid (they occupy no voxel)   */
    int32_t reserved[2];
    double merge_ms;             /* device time (events on the ctx's stream)                                      */
} isdf_points_merge_info;
int isdf_points_merge_check(isdf_ctx *ctx, double below, isdf_points_merge_info *info_out);

/* ---- full objective callback ------------------------------------------------------------------------------ */
/* TrajOptimizer::costFunctionLmbm (back_end_optimizer.hpp:358-430): x = [tau(N) | inner waypoints 3(N-1)] ->
 * cost, g.  MINCO (minco.hpp:397-655: setParameters, energy and its partials, propogateGrad) and the sweeps: for
 * ISDF_V1_SWEPT the swept-volume sweep followed by the integral sweep without a collision term (the reference's live
 * configuration), otherwise the integral sweep of cfg.variant.  cost = energy + sweeps + rho * sum(T).
 * MINCO has two forms here.  On the DEVICE (csrc/minco_dev.hip, minco_pcr.hpp): the trajectory in its junction states - a
 * symmetric positive definite block-tridiagonal system with 2 x 2 blocks - solved by parallel cyclic reduction in
 * ceil(log2(N - 1)) rounds, as two small kernels either side of the sweeps; the callback then moves n doubles down and n + 5
 * up and nothing else crosses PCIe.  On the HOST (csrc/minco_host.hpp): the reference's banded LU, a chain of 6N dependent
 * pivots, pivot for pivot.  They agree to rounding (coefficients 1e-10 relative, tests/test_minco_pcr.py).
 * isdf_set_minco_mode: 0 = whichever is faster for the configuration (default: the device, except single-trajectory tile-sweep
 * steps of <= 64 pieces on one GPU, where the host's 10 us beat two more kernel launches), 1 = host, 2 = device (trajectories of
 * more than 400 pieces always take the host).  isdf_minco_path tells which one the last callback took (1 = device).
 * isdf_set_trajectory == minco.setConditions + the `rho` of setParam (head/tail: 3x3 column-major, columns =
 * position, velocity, acceleration).  isdf_pack_variables == backwardT/backwardP (back_end_optimizer.cpp:22-28),
 * isdf_unpack_variables == forwardT/forwardP + setParameters (T: N, coeffs: 6N x 3 column-major; either may be NULL). */
int isdf_set_trajectory(isdf_ctx *ctx, int N, const double head_pva[9], const double tail_pva[9], double rho);
int isdf_num_variables(const isdf_ctx *ctx);               /* N + 3(N-1), 0 before isdf_set_trajectory     */
int isdf_pack_variables(isdf_ctx *ctx, const double *T, const double *waypoints, double *x);
int isdf_unpack_variables(isdf_ctx *ctx, const double *x, double *T, double *coeffs);
int isdf_cost_function(isdf_ctx *ctx, const double *x, double *g, int n, double *cost_out);
int isdf_set_minco_mode(isdf_ctx *ctx, int mode);          /* 0 = auto (default), 1 = host band LU, 2 = device */
int isdf_minco_path(const isdf_ctx *ctx);                  /* of the last callback: 1 = device, 0 = host      */
/* the same with the lmbm_evaluate_t signature (src/utils/include/utils/lmbm.h:206-209); instance = isdf_ctx*,
 * returns +inf on error */
double isdf_cost_function_lmbm(void *instance, const double *x, double *g, const int n);
/* Multi-GPU form (one process per GPU after isdf_set_shard): _launch runs MINCO and queues this rank's share of the
 * sweeps on `stream` (hipStream_t as void*), returning the device buffer of partial sums (count doubles); the caller
 * sums it over the ranks in place on the same stream (ONE all-reduce per step: ncclAllReduce(sum, ncclDouble) /
 * torch.distributed.all_reduce); _finish downloads it and completes the callback - identical (cost, g) on every rank. */
int isdf_cost_function_launch(isdf_ctx *ctx, const double *x, int n, void *stream, double **d_partial_out, size_t *count_out);
int isdf_cost_function_finish(isdf_ctx *ctx, double *g, double *cost_out, void *stream);
/* energy | swept-volume sweep | integral sweep | rho*sum(T) of the last isdf_cost_function call */
int isdf_cost_parts(const isdf_ctx *ctx, double parts[4]);

/* ---- multi-GPU exchange over xGMI peer stores (one node) -------------------------------------------------------- */
/* The exchange INSIDE the step (csrc/tile_sweep.hip, fused launch): on = 1 makes every following isdf_eval_device a complete
 * multi-GPU step - the workgroup that owns a piece stores its 19 output rows and its cost straight into every peer's board
 * (IPC-mapped, uncached), the peers' workgroups for that piece poll them into their own output, so on return every rank's
 * output holds the FULL [cost | gradT | gradC] (bitwise identical on all ranks) and no isdf_xchg_allreduce / ncclAllReduce
 * follows.  A step that runs as one fused launch (analytic shape with identity body offset, one trajectory or a small batch)
 * carries the exchange in that launch; any other step of the integral sweep (larger shards, body offsets, mesh robots) in its
 * tail launch.  Requires isdf_set_shard(rank, world) equal to the exchange's, all ranks switching together and evaluating in
 * lock-step.  Waits are bounded (about one second): a missing peer sets the overflow flag and a NaN cost instead of hanging
 * the stream - after which the exchange should be switched off (the boards may be out of step).
 * Replaces: the reference has no multi-GPU path; SURVEY 8(e) "prefer one-shot P2P reduce over xGMI". */
int isdf_xchg_fuse(isdf_ctx *ctx, int on);
/* The sum of the ranks' packed vectors is the ONE exchange step of the sharded path.  Any all-reduce works (RCCL through
 * torch.distributed: INTEGRATION.md); for vectors this small (6-50 KB) its latency rivals the whole optimizer step, so the
 * library also provides a one-shot peer-to-peer form: every rank stores its vector into a mailbox slot on every peer
 * (IPC-mapped, uncached device memory), raises a flag, waits (bounded) for its own mailbox and adds the slots in rank order -
 * one kernel per step, bit-identical sums on all ranks.  Setup: every rank calls isdf_xchg_create (64-byte IPC handle out),
 * the host all-gathers the handles (any transport), every rank calls isdf_xchg_connect with the world x 64 bytes in rank
 * order.  isdf_xchg_allreduce is asynchronous on `stream` and sums d_buf[0..count) in place; isdf_xchg_status returns 1 if
 * a wait ever timed out (the result of that exchange is invalid: fall back to RCCL).  All ranks must be on one node with
 * peer access between their devices. */
int isdf_xchg_create(isdf_ctx *ctx, int rank, int world_size, size_t max_doubles, void *ipc_handle_out_64bytes);
int isdf_xchg_connect(isdf_ctx *ctx, const void *ipc_handles_world_x_64bytes);
int isdf_xchg_allreduce(isdf_ctx *ctx, double *d_buf, size_t count, void *stream);
int isdf_xchg_status(isdf_ctx *ctx);
int isdf_xchg_destroy(isdf_ctx *ctx);
/* The bound T of every wait of both exchange forms, in MILLISECONDS OF THE DEVICE'S WALL CLOCK (wall_clock64(), constant rate:
 * the same duration on every box; default 2 000 - generous: the ranks are separate processes -, settable 1 ... 10 000): how much later than this rank a peer may start a step
 * before this rank calls the exchange failed.  A failed isdf_xchg_allreduce kernel ends after T on the rank whose wait expired
 * and at once on the late rank (which reads the first one's verdict); a healthy one waits at most 2.25 T for the verdicts.
 * Replaces: nothing in the reference (no multi-GPU path); the counterpart of NCCL's watchdog time-out, SURVEY 8(e). */
double isdf_xchg_timeout_ms(isdf_ctx *ctx);
int isdf_xchg_set_timeout_ms(isdf_ctx *ctx, double milliseconds);

/* ---- optimizer driver ----------------------------------------------------------------------------------------- */
/* L-BFGS behind the callback: lbfgs::lbfgs_optimize of src/utils/include/utils/lbfgs.hpp:480-835 (the LBFGS-Lite fork
 * the reference ships; its mid end calls it at src/planner_algorithm/src/mid_end.cpp:48-62).  Field names and defaults
 * are lbfgs_parameter_t's (:15-129).  weak_wolfe = 0 is the fork's Armijo-only line search (:373-386), 1 the
 * Lewis-Overton test it comments out; reference_patches = 1 keeps the fork's steepest-descent fallbacks (:788-819).
 * status uses the reference's codes: 0 convergence, 1 stop (delta test), 2 cancelled, negative = LBFGSERR_* (:133-160). */
typedef struct isdf_lbfgs_params {
    int32_t mem_size, past, max_iterations, max_linesearch, weak_wolfe, reference_patches;
    double g_epsilon, delta, min_step, max_step, f_dec_coeff, s_curv_coeff, cautious_factor, machine_prec, dir_norm_cap;
} isdf_lbfgs_params;
typedef struct isdf_lbfgs_result {
    double f;                /* cost at the returned x                              */
    double wall_ms;          /* host wall time of the whole minimisation            */
    int32_t status, iterations, evaluations, reserved;
} isdf_lbfgs_result;
typedef double (*isdf_evaluate_fn)(void *instance, const double *x, double *g, const int n);   /* == lmbm_evaluate_t */
void isdf_lbfgs_params_default(isdf_lbfgs_params *p);
/* any callback (no device needed) */
int isdf_lbfgs_minimize(isdf_evaluate_fn evaluate, void *instance, double *x_inout, int n,
                        const isdf_lbfgs_params *p, isdf_lbfgs_result *out);
/* Progress / cancel hook of the drivers: lbfgs_progress_t (lbfgs.hpp:256-262) with plain pointers - called once per iteration
 * after the line search with the iterate x, its gradient g (n doubles each), the cost, the accepted step, the iteration count k
 * and the number of evaluations ls of this line search; a non-zero return cancels the minimisation (status 2 = LBFGS_CANCELED,
 * x_inout = the iterate the hook was shown).  The reference's callers pass one to stop or watch a run (earlyExit /
 * earlyexitLmbm, back_end_optimizer.hpp:888-960); LMBM's lmbm_progress_t (lmbm.h:211-213) is its (instance, x, k) subset. */
typedef int (*isdf_progress_fn)(void *instance, const double *x, const double *g, double fx, double step, int k, int ls);
/* isdf_lbfgs_minimize with the hook; `instance` goes to both callbacks, like the reference's callback_data_t */
int isdf_lbfgs_minimize_progress(isdf_evaluate_fn evaluate, isdf_progress_fn progress, void *instance, double *x_inout, int n,
                                 const isdf_lbfgs_params *p, isdf_lbfgs_result *out);
/* The hook of the ctx's own drivers (NULL: none).  isdf_optimize_lbfgs calls progress(instance, ...); in
 * isdf_optimize_lbfgs_batch trajectory t's hook gets (char *)instance + t * batch_instance_stride (stride 0: the same pointer)
 * and is called on that trajectory's host thread - concurrently with the other trajectories' - so that one trajectory can be
 * cancelled (its result: status 2) while the rest of the batch runs on. */
int isdf_set_progress(isdf_ctx *ctx, isdf_progress_fn progress, void *instance, size_t batch_instance_stride);
/* the ctx's own objective: isdf_cost_function */
int isdf_optimize_lbfgs(isdf_ctx *ctx, double *x_inout, int n, const isdf_lbfgs_params *p, isdf_lbfgs_result *out);

/* Lazy constraint generation around it: the V1 term sees only the ctx's obstacle points - in the reference those
 * gathered in boxes around the A* waypoints (plan_manager.cpp:232-254, PCSmap_manager.h:182-216) - while the optimised
 * trajectory is free to leave the boxes, which the reference notices and only reports (plan_manager.cpp:306-309).  Per round:
 * isdf_optimize_lbfgs from the current x (a negative L-BFGS status does not end the loop: the reference extracts the trajectory
 * even then, back_end_optimizer.cpp:61-95), isdf_unpack_variables, isdf_traj_check with `margin` and `mode`; nothing below the
 * margin: clear = 1, stop; else isdf_points_merge_check(below); nothing added: stalled = 1, stop.  At most max_rounds rounds.
 * The last check's rows stay kept in the ctx.  The point set may start empty (isdf_set_points(ctx, NULL, 0)): the check then
 * discovers the obstacle points that matter.  V1 ctx only (else ISDF_ERR_UNSUPPORTED); isdf_set_trajectory and an occupancy grid
 * are needed as the pieces need them. */
typedef struct isdf_refine_params {
    int32_t max_rounds;      /* optimise+check rounds, >= 1; default 4                                            */
    int32_t mode;            /* field mode of the check; default ISDF_SWEPT_FIELD_PLANNER                         */
    double margin;           /* the check's margin; negative (default) = cfg.safety_hor                           */
    double below;            /* passed to the merge; negative (default) = every kept row                          */
} isdf_refine_params;
typedef struct isdf_refine_result {
    int32_t rounds;          /* rounds run                                                                        */
    int32_t clear;           /* 1: the last check found nothing below the margin                                  */
    int32_t stalled;         /* 1: stopped because a merge added nothing (every offending voxel already a point)  */
    int32_t reserved;
    int32_t M_round[16];     /* size of the point set each round optimised with (first 16 rounds)                 */
    isdf_lbfgs_result last_opt;
    isdf_traj_check_info last_check;
} isdf_refine_result;
void isdf_refine_params_default(isdf_refine_params *p);
/* rp NULL = defaults */
int isdf_optimize_lbfgs_checked(isdf_ctx *ctx, double *x_inout, int n, const isdf_lbfgs_params *lp,
                                const isdf_refine_params *rp, isdf_refine_result *out);

/* A batch of trajectories optimised CONCURRENTLY on the shared map (BASELINE.json configs[2]): trajectory t has its own
 * boundary states heads_pva[9t..], tails_pva[9t..] (3x3 column-major each, like isdf_set_trajectory) and its own
 * variables x_inout[t*n .. (t+1)*n), n = N + 3(N-1); all share N, rho and the ctx's map / robot / weights.  Each runs
 * the same L-BFGS driver on its own callback (one host thread per trajectory); the callbacks of a round are evaluated as ONE
 * batched integral sweep on the device.  The trajectories are dealt into 4 fixed groups (ISDF_BATCH_GROUPS), a group's round
 * starts when all its live members wait - every round is full - and up to three rounds are in flight (ISDF_BATCH_SLOTS), so that
 * one group's sweep runs while the others' host threads do their L-BFGS updates: 128 x 40 pieces x 30 iterations in 75 ms = 4.9e8
 * point-evals/s end to end, 93 % of the batched sweep's own rate.  MINCO (minco.hpp:43-198,433-513,530-654) of a round runs on
 * the device, one workgroup per trajectory, either side of the sweep (csrc/minco_dev.hip); isdf_set_minco_mode(ctx, 1) keeps it on
 * the trajectories' host threads.  The iterates are bit for bit those of optimising every trajectory alone with
 * isdf_optimize_lbfgs UNDER THE SAME MINCO MODE (mode 0 picks the host form for a single trajectory of <= 64 pieces and the
 * device form for the batch: set the mode explicitly to compare).  results[t].reserved = number of device rounds of the whole
 * batch.  V2 / V3 contexts only; not on a sharded ctx (shard the batch across ranks instead). */
int isdf_optimize_lbfgs_batch(isdf_ctx *ctx, int n_traj, int N, const double *heads_pva, const double *tails_pva, double rho,
                              double *x_inout, const isdf_lbfgs_params *p, isdf_lbfgs_result *results, double *wall_ms_out);

/* ---- mid end: the MINCO fit to the front end's waypoints ------------------------------------------------------------ */
/* OriTraj (src/planner_algorithm/include/planner_algorithm/mid_end.hpp, src/planner_algorithm/src/mid_end.cpp): between the A*
 * and the back end the reference fits a MINCO trajectory to the path's waypoints and starts the back end from the result
 * (plan_manager.cpp:202-313, opt_x at :270,289).  Variables x = [tau(N) | inner waypoints 3(N-1), point-major] - the layout of
 * isdf_pack_variables, so the fit's x goes straight into isdf_optimize_lbfgs.  cost = MINCO jerk energy + weight_pr * sum(pose
 * penalty) + rho_mid_end * sum(T) (mid_end.hpp:262-304); constraint i (0 .. N-2) samples PIECE i+1 at T(i+1) / integral_intervs
 * (:228-247), cost_p = |pos - ref_i|^3 (:184-199), and the time gradient of the penalty carries the reference's extra factor cost_p
 * (:256).  The reference stores attitudes and accelerations (:41-43) and never reads them: there is no attitude term.
 * The boundary states are isdf_set_trajectory's (its rho is not used here); no grid, shape or points are needed, on a ctx of any
 * variant.  isdf_set_minco_mode picks the form as for the back end: 1 = host (csrc/midend_host.hpp: the reference's arithmetic on
 * the band LU), 2 = device (csrc/midend.hip: the whole callback in ONE launch, one workgroup per trajectory), 0 = host for a single
 * trajectory of <= 64 pieces, device otherwise and for every batch; more than 400 pieces always take the host.  isdf_minco_path
 * tells which form ran.  N < 2: ISDF_ERR_INVALID_ARG (the reference always has a waypoint, plan_manager.cpp:209-213); a
 * multi-device ctx: ISDF_ERR_UNSUPPORTED. */
typedef struct isdf_midend_params {
    double weight_pr;            /* weight_pr: 1000                                                                   */
    double rho_mid_end;          /* rho_mid_end: 200                                                                  */
    double rel_cost_tol;         /* relCostTolMidEnd -> the driver's delta (mid_end.cpp:54): 1e-6                     */
    double min_step, g_epsilon;  /* min_step 1e-32, g_epsilon 0 (mid_end.cpp:51-52)                                   */
    int32_t integral_intervs;    /* integralIntervs (mid_end.hpp:323); default: isdf_config_default's                 */
    int32_t mem_size, past;      /* mem_size 16, past 10 (mid_end.cpp:49-50)                                          */
    int32_t reserved;
} isdf_midend_params;
void isdf_midend_params_default(isdf_midend_params *p);
/* the same fields from a plan yaml of src/plan_manager/config (Config::loadParameters, config.hpp:96-154); what the file leaves
 * out keeps isdf_midend_params_default's value */
int isdf_load_yaml_midend(const char *yaml_path, isdf_midend_params *out);
/* OriTraj::costFunction (mid_end.hpp:262-304) at x: ref_points (N-1) x 3 point-major, g: n = N + 3(N-1), parts_out (nullable):
 * energy | weight_pr * sum(pose penalty) | rho_mid_end * sum(T). */
int isdf_midend_cost(isdf_ctx *ctx, const isdf_midend_params *params, const double *ref_points, const double *x, double *g, int n,
                     double *cost_out, double parts_out[3]);
/* ... of nb trajectories of isdf_set_trajectory's N pieces, each with its own boundary states (heads_pva / tails_pva: 9 doubles per
 * trajectory, like isdf_optimize_lbfgs_batch), ref_points [nb][(N-1) x 3], x and g [nb][n], cost_out [nb]: one launch, one workgroup
 * per trajectory; every row is bitwise what isdf_midend_cost returns for it alone in device mode. */
int isdf_midend_cost_batch(isdf_ctx *ctx, const isdf_midend_params *params, int nb, const double *heads_pva, const double *tails_pva,
                           const double *ref_points, const double *x, double *g, double *cost_out);
/* OriTraj::getOriTraj (mid_end.cpp:3-94): x seeded with tau = backwardT(T_init), xi = ref_points (:27-41), then the L-BFGS driver
 * with mem_size, past, min_step, g_epsilon, max_iterations = 100000 and delta = rel_cost_tol (:48-62) and the hook of
 * isdf_set_progress.  x_out (n) is the last iterate and is written whatever out->status says, as the reference extracts the
 * trajectory either way (:65-92); T_out (N) and coeffs_out (6N x 3 column-major), either nullable, are forwardT and setParameters
 * of it (:67-71). */
int isdf_midend_fit(isdf_ctx *ctx, const isdf_midend_params *params, const double *ref_points, const double *T_init, double *x_out,
                    double *T_out, double *coeffs_out, isdf_lbfgs_result *out);
/* nb fits of N pieces each (T_init [nb][N], x_out [nb][n]), one host thread per trajectory (ISDF_BATCH_THREADS caps the live ones); a
 * round starts when every live trajectory waits for its callback and is ONE launch with one workgroup per live trajectory.  The
 * iterates are bit for bit those of isdf_midend_fit on each trajectory alone in device mode.  The hook of isdf_set_progress is
 * called per trajectory as in isdf_optimize_lbfgs_batch; results[t].reserved = rounds of the whole batch.  Needs no
 * isdf_set_trajectory. */
int isdf_midend_fit_batch(isdf_ctx *ctx, const isdf_midend_params *params, int nb, int N, const double *heads_pva, const double *tails_pva,
                          const double *ref_points, const double *T_init, double *x_out, isdf_lbfgs_result *results, double *wall_ms_out);

/* ---- front end: pose feasibility by kernel convolution ------------------------------------- */
/* The A* front end decides whether the robot fits at a voxel by AND-ing a bit-packed voxelisation of the robot at a
 * (roll, pitch) attitude against the bit-packed occupancy map, trying attitudes breadth-first from the parent's
 * (SweptVolumeManager::checkKernelValue, sw_manager.hpp:911-942).  The tables are built on the device from the installed
 * shape and occupancy grid; queries are answered in batches.  All results are integer / byte work: bit-identical to the
 * reference's. */
typedef struct isdf_frontend_config {
    int32_t kernel_size;        /* Config::kernel_size: odd, side of the robot voxelisation in voxels (<= 31)            */
    int32_t reserved;
    double kernel_max_roll;     /* degrees: attitudes -max .. +max in steps of kernel_ang_res (Shape.hpp:297-298,          */
    double kernel_max_pitch;    /*          :416-421); the shipped configs use 45 / 45 / 9 -> 11 x 11 attitudes            */
    double kernel_ang_res;
    double front_end_safeh;     /* a voxel belongs to the robot when sdf <= max(front_end_safeh, resolution / 2) (:415)    */
} isdf_frontend_config;
/* Builds (a) the robot's attitude kernels - BasicShape::initShape<true,...> kernel part (Shape.hpp:400-459): for every
 * attitude, voxel (a, b, c) is set when getonlySDF(pos, Rx(roll) * Ry(pitch)) <= margin - and (b) the inflated, bit-packed
 * occupancy map of PCSmapManager::generateMapKernel (PCSmap_manager.h:46-78).  Needs isdf_set_shape and an occupancy grid
 * (isdf_set_grid ISDF_GRID_OCCUPANCY or isdf_set_pointcloud).  Call again after either changes. */
int isdf_frontend_build(isdf_ctx *ctx, const isdf_frontend_config *cfg);
/* Read-back in the REFERENCE's byte layouts (bit z of a row in byte z / 8 under mask 0x80 >> (z % 8)).
 * Shape kernels: ByteShapeKernel::map of every attitude, attitude-major ((i * ykernel + j) * k * k * ((k + 7) / 8) bytes;
 * what plan_manager.cpp:545 reads through getOccupied).  dims_out = {xkernel_size, ykernel_size, bytes per attitude}.
 * Map kernel: the array SweptVolumeManager::setMapKernel receives; dims_out = inflated {X, Y, bytes per z-row}.
 * `out` may be NULL to query the sizes. */
int isdf_frontend_get_shape_kernels(isdf_ctx *ctx, uint8_t *out, int dims_out[3]);
int isdf_frontend_get_map_kernel(isdf_ctx *ctx, uint8_t *out, int dims_out[3]);
/* n queries of the per-neighbour test of AstarPathSearcher::AstarGetSucc (front_end_Astar.hpp:214-217):
 *   ok[q] = isIndexValid(ind) && !isIndexOccupiedFlate(ind, 0) && checkKernelValue(father_roll, father_pitch, cr, cp, ind)
 * with ind = index[3q..3q+2] (voxel of the ORIGINAL map), and child_roll / child_pitch (degrees) of the first collision-free
 * attitude in the reference's breadth-first order (visit_kernels_by_distance, :850-909: level attitude first, then outward
 * from the parent's attitude, neighbours pushed in the order (0,+1) (0,-1) (+1,0) (-1,0)).  child_* are written only where
 * ok[q] = 1.  kernel_index_out (optional) receives i * ykernel + j of that attitude, -1 where ok = 0. */
int isdf_frontend_check(isdf_ctx *ctx, int n, const int32_t *index, const double *father_roll, const double *father_pitch,
                        uint8_t *ok, double *child_roll, double *child_pitch, int32_t *kernel_index_out);

/* The whole configuration space in one pass: for EVERY voxel of the map, which attitudes are collision-free
 * (kernelConv<true>(i, j, voxel), sw_manager.hpp:813-847, for all i, j).  free_mask_out (may be NULL: the table then only
 * stays on the device): 4 * ceil(attitudes / 128) dwords per voxel in the grid's own order (z fastest; 4 for the shipped 11 x 11),
 * bit (i * ykernel + j) set = that attitude fits; occupied voxels get 0.  An A* that holds this table answers checkKernelValue with a few
 * bit tests in the breadth-first order instead of k^2 byte-ANDs per attitude.  kernel_ms_out (optional): device time. */
int isdf_frontend_cspace(isdf_ctx *ctx, uint32_t *free_mask_out, double *kernel_ms_out);
/* The table as it stands, WITHOUT computing it again (same layout): which = 0 the device's table (ISDF_ERR_STATE before the first
 * isdf_frontend_cspace / search / field build), which = 1 the copy the A* keeps on the host (ISDF_ERR_STATE while it holds none that
 * is valid).  What isdf_update_pointcloud / isdf_update_voxels left behind is read with this. */
int isdf_frontend_cspace_get(isdf_ctx *ctx, int which, uint32_t *table_out);

/* The SE(3) A* of the front end (AstarPathSearcher, planner_algorithm/front_end_Astar.hpp:172-403) over the table above, called
 * like PlannerManager::generatePath calls the reference's (plan_manager.cpp:181-198):
 *   isdf_frontend_astar_search  = AstarPathSearch(start, end); result->success = success_flag;
 *   isdf_frontend_astar_path    = getPath() + getastarSE3Path() of that search (valid until the next search, which is also the
 *                                 reference's reset()).
 * The first search after isdf_frontend_build computes the whole configuration space on the device (isdf_frontend_cspace) and
 * keeps it in pinned host memory; a search then runs on the calling thread and answers every neighbour test
 * (isIndexValid && !isIndexOccupiedFlate && checkKernelValue, :214-216) with bit tests on a voxel's word of the table (128 bits per 128 attitudes) in the
 * reference's breadth-first attitude order.  Same open-set order (that of a multimap keyed by the fScore at insertion, first inserted
 * first among equals), same 26+1 neighbour order, same re-opening of closed nodes, same (roll, pitch) bookkeeping (a node's
 * attitude is overwritten by every expansion that finds it feasible, :227-228) => the same path and attitudes, node for node.
 * start / goal: world coordinates; outside the map => success = 0 (the reference logs an error and returns, :244-249). */
typedef struct isdf_astar_result {
    int32_t success;            /* AstarPathSearcher::success_flag                                                         */
    int32_t n_path;             /* nodes on the path, start and goal cells included (0 when the search failed)             */
    int64_t expansions;         /* nodes taken off the open set                                                            */
    int64_t checks;             /* neighbour tests = the reference's total_kernel (:218)                                   */
    double cspace_ms;           /* device time of the configuration-space pass when THIS call ran it, else 0               */
    double table_ms;            /* wall time of that pass + bringing the table to the host, else 0                         */
    double search_ms;           /* wall time of the search itself                                                          */
} isdf_astar_result;
int isdf_frontend_astar_search(isdf_ctx *ctx, const double start[3], const double goal[3], isdf_astar_result *result);
/* Path of the last successful search, start -> goal: xyz = cube centres (3 doubles per node), roll_pitch = degrees (2 per
 * node), rot = SE3State::rot = AngleAxis(roll, X) * AngleAxis(pitch, Y) as a row-major 3x3 (9 per node); any may be NULL.
 * Writes at most `capacity` nodes; returns the number of nodes of the path (0 = no path), or a negative isdf_status. */
int isdf_frontend_astar_path(isdf_ctx *ctx, int capacity, double *xyz, double *roll_pitch, double *rot);

/* ---- front end: the cost-to-go field of one goal, and paths read off it ------------------------------------------------- */
/* The search above is one chain of heap pops per start.  For MANY starts towards one goal (or one robot replanning towards a
 * fixed goal) the same graph is solved once for every voxel, on the device, and any number of paths are read off in parallel.
 * Graph = that of AstarPathSearcher::AstarGetSucc (planner_algorithm/front_end_Astar.hpp:197-236): a voxel is FREE when any
 * attitude bit of its word of the isdf_frontend_cspace table is set; a step goes to any of the 26 neighbours that is free and
 * inside the map and costs edge[i*i + j*j + k*k] = sqrt(i*i + j*j + k*k) CELLS (:230).  "Any bit set" equals checkKernelValue
 * (sw_manager.hpp:911-942) when the parent's attitude lies on the attitude grid and the grid has at most 801 attitudes.
 *   d[goal] = 0;  d[v] = min over free neighbours u of fl(d[u] + w(u, v)) for free v - fp64, one addition per candidate, the least
 *   fixed point from +inf; +inf where v is not free or cannot reach the goal.
 * Every relaxation order reaches the same bytes, those of Dijkstra with the same fl(d[u] + w): the device form (active bricks of
 * 8 x 8 x 64 voxels relaxed in LDS, one launch per round) and isdf_frontend_field_host agree byte for byte. */
typedef struct isdf_frontend_field_params {
    int32_t max_rounds;         /* bound of the relaxation rounds; 0 = the proven bound, the number of free voxels            */
    int32_t reserved;
} isdf_frontend_field_params;
void isdf_frontend_field_params_default(isdf_frontend_field_params *out);
typedef struct isdf_frontend_field_info {
    int32_t reachable;          /* 1: the goal cell is inside the map and free; 0: the whole field is +inf (the A* would     */
                                /*    return success = 0, front_end_Astar.hpp:244-249)                                        */
    int32_t status;             /* 0 the fixed point; 1 no reachable goal; 2 max_rounds hit: the field as it stands, an upper */
                                /*    bound of d everywhere                                                                   */
    int32_t rounds;             /* launches of the relaxation                                                                 */
    int32_t bricks;             /* bricks relaxed at least once                                                               */
    int64_t brick_visits;       /* bricks relaxed, over all rounds                                                            */
    int64_t free_voxels;
    int64_t reached_voxels;     /* voxels with a finite d                                                                     */
    double device_ms;           /* device time from the first launch to the end of the last                                   */
} isdf_frontend_field_info;
/* Builds the field of the cell of goal_xyz (world coordinates, the cell as AstarPathSearch takes it, :250-252).  Runs the
 * configuration-space pass if the table is not on the device yet and does NOT bring the table to the host.  params may be NULL.
 * Needs isdf_frontend_build (else ISDF_ERR_STATE); a new isdf_frontend_build drops the field.  Not on a multi-device ctx. */
int isdf_frontend_field_build(isdf_ctx *ctx, const double goal_xyz[3], const isdf_frontend_field_params *params, isdf_frontend_field_info *info_out);
/* The whole field, X * Y * Z doubles in the grid's own order (z fastest). */
int isdf_frontend_field_get(isdf_ctx *ctx, double *d_out);
/* d at the cells of n world points (3 doubles each; the cell as getGridIndex gives it); +inf for a point outside the map. */
int isdf_frontend_field_value(isdf_ctx *ctx, const double *xyz, int n, double *out);
/* Paths for B starts in one launch, one lane per start.  From the start's cell the walk steps to the neighbour u that minimises
 * fl(d[u] + w), the first in AstarGetSucc's i, j, k loop order (:207-211) among equals, until the goal cell.  The start cell need
 * not be free (the A* never tests it, :260-278).  Per node: the cube centre (getGridCubeCenter) and the attitude checkKernelValue
 * would give walking that way - the start at roll = pitch = 0, then the first set bit of the node's word in the breadth-first
 * order of the previous node's attitude, roll = fr + (ri - fi) * ang_res (sw_manager.hpp:914-932), degrees.
 * n_out[b]: nodes of path b, start and goal cells included; 0 = no path (start outside the map, all neighbours +inf, or no
 * reachable goal); 1 = the start is in the goal cell.  A path longer than cap is reported by its true length and truncated, as
 * isdf_frontend_astar_path does.  xyz_out: B x cap x 3, roll_pitch_out: B x cap x 2; the host form zeroes what lies past a
 * path's end, the device form leaves it.  cap < 1 and null pointers are argument errors. */
int isdf_frontend_field_paths(isdf_ctx *ctx, const double *starts_xyz, int B, int cap, int32_t *n_out, double *xyz_out, double *roll_pitch_out);
/* The same with device arrays, asynchronous on `stream` (a hipStream_t); the field must not be rebuilt before it has run. */
int isdf_frontend_field_paths_device(isdf_ctx *ctx, const double *d_starts_xyz, int B, int cap, int32_t *d_n_out, double *d_xyz_out,
                                     double *d_roll_pitch_out, void *stream);
/* The host form, no device and no ctx: Dijkstra with a binary heap over a caller-supplied table in isdf_frontend_cspace's layout
 * (4 * ceil(n_att / 128) dwords per voxel, dims = {X, Y, Z}, z fastest; free = any bit set - the graph of AstarGetSucc,
 * front_end_Astar.hpp:197-236).  goal_index: the goal's voxel; outside the map or not free => every d is +inf.
 * Returns 1 (reachable), 0 (not), or a negative isdf_status. */
int isdf_frontend_field_host(const uint32_t *free_mask, const int32_t dims[3], int n_att, const int32_t goal_index[3], double *d_out);
/* Frees the field and its scratch (isdf_frontend_field_build allocates again). */
int isdf_frontend_field_release(isdf_ctx *ctx);

/* ---- the field repaired after a map update ------------------------------------------------------------------ */
/* isdf_update_pointcloud / isdf_update_voxels (below) only ever CLOSE voxels: occupancy grows, free bits of the configuration-space
 * table fall.  That is the premise of the rule:
 *   closed = the voxels that were free when the field was built (or last repaired) and whose word is 0 now;
 *   tau    = the smallest OLD d over the closed voxels, +inf when none of them had a finite d.
 *   Every d < tau is kept, every finite d >= tau (the closed voxels included) becomes +inf, and the build's relaxation runs on from
 *   there, starting at the bricks that hold a reset voxel.
 * Why the bytes are those of a build on the new map: the new graph is a subgraph of the old, so no d can fall; every step costs
 * w > 0 and fl is monotone, so along the chain of minimising neighbours from a voxel to the goal d does not rise - from a voxel
 * with d < tau the chain passes only voxels with d < tau, none of them closed, so the old value is still reached.  From the kept
 * values every intermediate value is again the length of a real path summed from the goal outward, and the fixed point is the
 * least one.  tau = 0 when the goal cell closes (everything is reset, reachable = 0); tau = +inf when nothing reached closes
 * (zero rounds, the bytes unchanged).  If a bit OPENED - impossible while occupancy only grows - the rule is not trusted and the
 * field is dropped.
 * isdf_frontend_field_set_repair: mode 0 (default) - an update that occupies a voxel drops the field, field_dropped = 1: what the
 * sentence about the field under isdf_update_pointcloud describes; mode 1 - such an update repairs a valid field in place, on both
 * of its paths and in both of its forms, on the ctx's stream after the configuration-space refresh; afterwards field_dropped = 0 and
 * isdf_frontend_field_get / _value / _paths[_device] answer as after isdf_frontend_field_build on the new map.  A field without a
 * reachable goal stays valid and all +inf.  A repair that hits its round bound (the free voxels, or the max_rounds of the build)
 * leaves a valid status-2 field, as the build does.  Also with mode 1 the field is dropped, field_dropped = 1, when it had status 2
 * (an upper bound, not a fixed point), when refresh_frontend = 0, when a bit opened, or when a step of the repair fails (the
 * update then fails as a whole and drops every derived product).  The mode outlives isdf_frontend_build.
 * Other modes: ISDF_ERR_INVALID_ARG; a multi-device ctx: ISDF_ERR_UNSUPPORTED. */
int isdf_frontend_field_set_repair(isdf_ctx *ctx, int mode);
typedef struct isdf_field_repair_info {
    int64_t closed_voxels;      /* voxels whose free bit fell                                                                 */
    int64_t closed_reached;     /* ... that had a finite d                                                                    */
    double tau;                 /* the smallest old d of a closed voxel; +inf: nothing reached closed                         */
    int64_t reset_voxels;       /* finite values set to +inf: the shell d >= tau, the closed voxels included                  */
    int64_t brick_visits;       /* bricks relaxed, over all rounds                                                            */
    int64_t free_voxels;        /* of the new map                                                                             */
    int64_t reached_voxels;     /* voxels with a finite d after the repair                                                    */
    int32_t seeded_bricks;      /* bricks that held a reset voxel other than a closed one: the first active list              */
    int32_t rounds;             /* launches of the relaxation                                                                 */
    int32_t reachable, status;  /* as isdf_frontend_field_info                                                                */
    double device_ms;           /* device time from the mark kernel to the end of the count                                   */
} isdf_field_repair_info;
/* The last repair's report; ISDF_ERR_STATE when there was none since the last isdf_frontend_field_build. */
int isdf_frontend_field_repair_info(isdf_ctx *ctx, isdf_field_repair_info *out);
void isdf_frontend_field_repair_sizes(int sizes_out[1]);      /* sizeof of the struct above, for mirrors of this header        */
/* The same rule in plain host code, no ctx and no device.  d_inout: on entry the field of goal_index on a table of which
 * free_mask_new (isdf_frontend_field_host's layout) is a subset - every voxel free in it was free before -, on return the field on
 * free_mask_new, the bytes of isdf_frontend_field_host.  tau is taken over the voxels with a finite d and a zero new word; after
 * the reset Dijkstra runs on from the kept finite voxels.  info_out may be NULL; of it closed_voxels = closed_reached (no old table
 * is given), seeded_bricks, rounds, brick_visits and device_ms stay 0.  Returns 1 (the goal cell is in the map and free), 0 (not),
 * or a negative isdf_status. */
int isdf_frontend_field_repair_host(const uint32_t *free_mask_new, const int32_t dims[3], int n_att, const int32_t goal_index[3],
                                    double *d_inout, isdf_field_repair_info *info_out);

/* ---- the field lowered in place after a clear --------------------------------------------------------------- */
/* isdf_clear_pointcloud / isdf_clear_voxels (below) only ever OPEN voxels: occupancy shrinks, free bits of the configuration-space
 * table rise.  That is the premise of the rule:
 *   opened = the voxels that were not free when the field was built (or last repaired / reopened) and whose word is non-zero now;
 *            their old d is +inf.
 *   Every old value is kept; when the goal cell is among the opened voxels (the field was all +inf) it takes d = 0; the build's
 *   relaxation runs on from there, starting at the bricks that hold an opened voxel.
 * Why the bytes are those of a build on the new map: the old graph is a subgraph of the new, so every old finite d is the length of
 * a path that still exists, an upper bound of the new least fixed point d*; relaxation only forms further such sums, so nothing
 * falls below d*; and a fixed point that is >= d* with d[goal] = 0 IS d* (walk the voxels in Dijkstra order of d*: the predecessor
 * u of v already holds d*[u], so d[v] <= fl(d*[u] + w) = d*[v]).  A brick without an opened voxel and without a lowered halo voxel
 * satisfies its equations as before, so starting at the opened voxels' bricks loses nothing.  An opened voxel whose neighbours are
 * all +inf stays +inf; a field without a reachable goal whose goal cell did not open stays all +inf, with zero rounds.  If a bit
 * CLOSED - impossible while occupancy only shrinks - the rule is not trusted and the field is dropped.
 * isdf_frontend_field_set_reopen: mode 0 (default) - a clear that frees a voxel drops a valid field, field_dropped = 1; mode 1 -
 * such a clear lowers a valid field in place, on both of its paths and in both of its forms, on the ctx's stream after the
 * configuration-space refresh; afterwards field_dropped = 0 and isdf_frontend_field_get / _value / _paths[_device] answer as after
 * isdf_frontend_field_build on the new map.  A reopen that hits its round bound (the free voxels of the new map, or the max_rounds
 * of the build) leaves a valid status-2 field, as the build does.  Also with mode 1 the field is dropped, field_dropped = 1, when
 * it had status 2, when refresh_frontend = 0, when a bit closed, or when a step fails (the clear then fails as a whole and drops
 * every derived product).  The mode outlives isdf_frontend_build and is independent of isdf_frontend_field_set_repair, which
 * decides about updates only.  Other modes: ISDF_ERR_INVALID_ARG; a multi-device ctx: ISDF_ERR_UNSUPPORTED. */
int isdf_frontend_field_set_reopen(isdf_ctx *ctx, int mode);
typedef struct isdf_field_reopen_info {
    int64_t opened_voxels;      /* voxels whose free bit rose                                                                 */
    int64_t opened_reached;     /* ... that have a finite d afterwards                                                        */
    int64_t reached_before;     /* voxels with a finite d before the reopen                                                   */
    int64_t reached_voxels;     /* ... and after it                                                                           */
    int64_t free_voxels;        /* of the new map                                                                             */
    int64_t brick_visits;       /* bricks relaxed, over all rounds                                                            */
    int32_t seeded_bricks;      /* bricks that hold an opened voxel: the first active list                                    */
    int32_t rounds;             /* launches of the relaxation                                                                 */
    int32_t goal_opened;        /* 1: the goal cell was among the opened voxels                                               */
    int32_t reachable, status;  /* as isdf_frontend_field_info                                                                */
    int32_t reserved;
    double device_ms;           /* device time from the mark kernel to the end of the counts                                  */
} isdf_field_reopen_info;
/* The last reopen's report; ISDF_ERR_STATE when there was none since the last isdf_frontend_field_build.  A repair does not touch
 * it, and a reopen does not touch isdf_frontend_field_repair_info. */
int isdf_frontend_field_reopen_info(isdf_ctx *ctx, isdf_field_reopen_info *out);
void isdf_frontend_field_reopen_sizes(int sizes_out[1]);      /* sizeof of the struct above, for mirrors of this header        */
/* The same rule in plain host code, no ctx and no device.  d_inout: on entry the field of goal_index on a table of which
 * free_mask_new (isdf_frontend_field_host's layout) is a superset - every voxel free before is free in it -, on return the field on
 * free_mask_new, the bytes of isdf_frontend_field_host.  Dijkstra continues from the kept finite voxels: the heap is seeded from the
 * finite neighbours of the voxels with a non-zero word and d = +inf, and from the goal when it is free and +inf.  info_out may be
 * NULL.  No old table is given, so an opened voxel that stays +inf cannot be told from one that was free and unreached:
 * opened_voxels = opened_reached = the voxels that were +inf and are finite now; seeded_bricks, rounds, brick_visits and device_ms
 * stay 0.  Returns 1 (the goal cell is in the map and free), 0 (not), or a negative isdf_status. */
int isdf_frontend_field_reopen_host(const uint32_t *free_mask_new, const int32_t dims[3], int n_att, const int32_t goal_index[3],
                                    double *d_inout, isdf_field_reopen_info *info_out);

/* ---- the field carried through a shift of the map window ------------------------------------------------------ */
/* isdf_shift_map / isdf_map_follow (below) move bits BOTH ways: with s the shift, new voxel v holds old voxel v + s; the voxels of
 * the leaving slabs vanish, the entering slabs appear free, and the words of the bands at the faces change either way.  The goal
 * is a cell and moves with the content: goal' = goal - s.  After the shift's configuration-space refresh, in two phases:
 *   1. translate and close: d1[v] = d_old[v + s] where the source exists and v's new word is non-zero, else +inf;
 *      fm1[v] = fm_old[v + s] & free_new[v] (0 for an entering voxel).  closed = every leaving voxel and every overlap voxel that
 *      was free and is not; tau = the least finite old d over them; then 4.6.2's reset (every finite d1 >= tau becomes +inf) and
 *      relaxation on the graph fm1, from the bricks that hold a reset voxel.
 *   2. open: 4.6.3 unchanged, fm1 against the new words - the entering slabs are among the opened voxels; d[goal'] = 0 when the
 *      goal cell opened.
 * Why the bytes are those of isdf_frontend_field_build towards goal' on a fresh ctx: in old indices G1 = fm_old & free_new is a
 * subgraph of the old graph, and the closed set is exactly what the old graph has and G1 lacks, so 4.6.2's argument gives the least
 * fixed point on G1; G1 is a subgraph of the new graph and every kept value is the sum along a path that still exists, so 4.6.3's
 * argument gives the least fixed point on the new map.  fm1 is a subset of the new free set by construction: phase 2 never sees a
 * bit against its direction (if it does, the call fails with ISDF_ERR_STATE - a defect, not a drop).
 * isdf_frontend_field_set_shift: mode 0 (default) - a shift drops a valid field, field_dropped = 1; mode 1 - a shift carries a
 * valid field, on both of its paths, with and without the A*'s host table, on the ctx's stream after the front-end refresh;
 * afterwards field_dropped = 0 and isdf_frontend_field_get / _value / _paths[_device] answer as after isdf_frontend_field_build
 * towards the centre of cell goal' on the new map.  A field without a reachable goal (all +inf) is carried too and becomes reachable
 * when its goal cell opens.  A phase that hits its round bound (the free voxels of its graph, or the max_rounds of the build) leaves a
 * valid status-2 field, as the build does.  Also with mode 1 the field is dropped, field_dropped = 1, when it had status 2, when
 * there is no configuration-space table, when goal' lies outside the grid, when |s_a| >= dims_a on some axis (everything left), or
 * when a step fails (the shift then fails as a whole and drops every derived product).  s = 0 touches nothing.  One more copy of d
 * and of the free bits stays allocated (8 B + 1 bit per voxel); nothing is allocated after the first carried shift of a size.
 * The mode outlives isdf_frontend_build and is independent of isdf_frontend_field_set_repair / _set_reopen.  Other modes:
 * ISDF_ERR_INVALID_ARG; a multi-device ctx: ISDF_ERR_UNSUPPORTED. */
int isdf_frontend_field_set_shift(isdf_ctx *ctx, int mode);
#define ISDF_FIELD_SHIFT_GOAL_LEFT 3   /* isdf_frontend_field_shift_host: status and return value when goal' lies outside the grid */
typedef struct isdf_field_shift_info {
    int32_t shift[3];           /* s                                                                                          */
    int32_t goal_new[3];        /* goal' = goal - s, the field's goal cell after the call                                     */
    int64_t left_reached;       /* leaving voxels (no destination) that held a finite d                                       */
    int64_t closed_voxels;      /* overlap voxels whose free bit fell                                                         */
    int64_t closed_reached;     /* ... that held a finite d                                                                   */
    double tau;                 /* the least d among left_reached and closed_reached; +inf when there is none                 */
    int64_t reset_voxels;       /* overlap voxels whose d became +inf in phase 1: closed_reached + the kept voxels with d >= tau */
    int64_t opened_voxels;      /* voxels free in the new map and not in fm1: the entering free voxels and the opened overlap */
    int64_t opened_reached;     /* ... that have a finite d afterwards                                                        */
    int64_t brick_visits;       /* bricks relaxed, over all rounds of both phases                                             */
    int64_t free_voxels;        /* of the new map                                                                             */
    int64_t reached_voxels;     /* voxels with a finite d afterwards                                                          */
    int32_t seeded_bricks_close, rounds_close;      /* phase 1: bricks that reset a voxel, launches of the relaxation         */
    int32_t seeded_bricks_open, rounds_open;        /* phase 2: bricks that hold an opened voxel, launches of the relaxation  */
    int32_t goal_opened;        /* 1: the goal cell was among the opened voxels                                               */
    int32_t reachable, status;  /* as isdf_frontend_field_info; host form: ISDF_FIELD_SHIFT_GOAL_LEFT when goal' is outside   */
    int32_t reserved;
    double device_ms;           /* device time of both phases, from the translation to the end of the counts                  */
} isdf_field_shift_info;
/* The last carry's report; ISDF_ERR_STATE when there was none since the last isdf_frontend_field_build.  It does not touch
 * isdf_frontend_field_repair_info / _reopen_info, and a repair or a reopen does not touch it. */
int isdf_frontend_field_shift_info(isdf_ctx *ctx, isdf_field_shift_info *out);
void isdf_frontend_field_shift_sizes(int sizes_out[1]);       /* sizeof of the struct above, for mirrors of this header        */
/* The same rule in plain host code, no ctx and no device.  d_inout: on entry the field of goal_index_old on the OLD table, on
 * return the field of goal_index_old - shift on free_mask_new (isdf_frontend_field_host's layout, the table after the shift), the
 * bytes of isdf_frontend_field_host.  d is translated by isdf_shift_grid_host's index rule with +inf where there is no source; tau
 * is taken over the leaving finite values and over the finite values whose new word is 0; phase 1 is
 * isdf_frontend_field_repair_host's rule on the table free_mask_new restricted to the voxels with a finite translated d (a voxel
 * that was free and unreached stays unreached on a subgraph, so no old table is needed), phase 2 isdf_frontend_field_reopen_host's
 * on free_mask_new.  info_out may be NULL.  No old table is given: closed_voxels = closed_reached, opened_voxels = opened_reached =
 * the voxels that were +inf after phase 1 and are finite now; the brick and round counts and device_ms stay 0.  Returns 1 (the goal
 * cell is in the map and free), 0 (in the map, not free: all +inf), ISDF_FIELD_SHIFT_GOAL_LEFT (goal' lies outside the grid: all
 * +inf, status likewise), or a negative isdf_status. */
int isdf_frontend_field_shift_host(const uint32_t *free_mask_new, const int32_t dims[3], int n_att, const int32_t shift[3],
                                   const int32_t goal_index_old[3], double *d_inout, isdf_field_shift_info *info_out);

/* ---- the map updated in place from new sensor points ---------------------------------------------------------- */
/* isdf_set_pointcloud rebuilds everything from the full cloud.  isdf_update_pointcloud takes only the NEW points (n_points x 3
 * floats, binned as isdf_set_pointcloud bins them: a point outside the box counts for voxel (0,0,0)), adds them to the per-voxel
 * counts that isdf_set_pointcloud keeps, and refreshes every derived product only where it can change: the occupancy, the ESDF
 * (new = min(old, distance to the nearest newly occupied voxel); occupancy only grows, as in the reference, whose
 * PCSmap_manager.cpp:87-200 only counts points up - voxels are taken OUT again by isdf_clear_pointcloud / isdf_clear_voxels, the
 * section after this one), the front end's inflated bit map over the box of the new voxels and its
 * configuration-space table - and, when the A* holds the table on the host, that copy - over the box grown by (kernel_size - 1) / 2.
 * Afterwards every product is byte for byte what a fresh ctx holds after isdf_set_pointcloud(old ++ new) with the same explicit
 * boundaries, resolution and threshold, then isdf_generate_esdf if an ESDF was installed (it is taken to be the exact distance
 * transform of the occupancy), isdf_frontend_build and isdf_frontend_cspace if they had been run.
 * The grid's geometry and the voxel indices handed out before (clearance reports, isdf_points_merge_check) stay valid; the
 * occupancy bit grid and the ESDF bricks are rebuilt lazily as after any map change.  The V1 obstacle-point set and lastTstar are
 * NOT touched: new obstacles reach the optimizer the usual way, through isdf_traj_check and isdf_points_merge_check.  With mode 1
 * of isdf_traj_check_set_watch an update that occupies a voxel also folds the new voxels into the kept clearance report, which then
 * reads as after isdf_traj_check on the updated map.  The
 * cost-to-go field cannot be repaired by a decrease-only relaxation when voxels close: it is dropped whenever a voxel became
 * occupied (isdf_frontend_field_* then answer as before a build) - mode 0 of isdf_frontend_field_set_repair, the default; mode 1
 * resets the part of the field that the closed voxels can have fed and relaxes it again.  When no voxel became occupied nothing but
 * the counts changes.
 * isdf_update_voxels is the same for a map that came from isdf_set_grid, or for a caller with its own voxel list: ijk = n_voxels x 3
 * indices to set occupied (duplicates and occupied voxels are fine; an index outside the grid: ISDF_ERR_INVALID_ARG, nothing
 * changed).  It invalidates kept counts when it occupies a voxel.
 * A failure (ISDF_ERR_HIP) after the counts and the occupancy have advanced leaves those two consistent and drops what was derived
 * from the old map - the ESDF and the front end, as isdf_set_pointcloud drops them - so that nothing stale can be read.
 * isdf_update_pointcloud: ISDF_ERR_STATE without kept counts (no isdf_set_pointcloud, or isdf_set_grid / isdf_update_voxels since).
 * Both: a multi-device ctx ISDF_ERR_UNSUPPORTED.  params may be NULL (defaults), info_out may be NULL. */
typedef struct isdf_map_update_params {
    int64_t max_new_voxels;     /* more newly occupied voxels than this: rebuild everything (default 65536)                    */
    double full_fraction;       /* the grown dirty box holds more than this share of the map's voxels: rebuild everything      */
                                /* (default 0.5).  Both defaults are placeholders: the incremental path won at every size that */
                                /* tools/map_update_bench.py measured, none near these caps                      */
    int32_t refresh_esdf;       /* 1 (default): refresh the ESDF if one is installed; 0: drop it, as isdf_set_pointcloud does  */
    int32_t refresh_frontend;   /* 1 (default): refresh the front end if built; 0: release it                                  */
} isdf_map_update_params;
typedef struct isdf_map_update_info {
    int64_t n_points, n_new_voxels;     /* points (or voxel entries) counted; voxels that became occupied                      */
    int32_t dirty_lo[3], dirty_hi[3];   /* index box of the new voxels (inclusive; lo > hi when none)                          */
    int32_t path;                       /* 0 nothing changed, 1 incremental, 2 full rebuild (a cap of params exceeded, or an   */
                                        /*   ESDF of a map that had no occupied voxel)                                         */
    int32_t esdf_refreshed, frontend_refreshed, cspace_refreshed, host_table_patched;
    int32_t field_dropped;              /* 1: a VALID cost-to-go field was dropped by this call (0 also when there was none to drop) */
    int64_t esdf_voxels_lowered;        /* incremental path: ESDF values that fell                                             */
    int64_t cspace_voxels_recomputed;   /* voxels of the grown box (the whole map on the full path)                            */
    double count_ms, esdf_ms, frontend_ms;      /* device time, events on the ctx's stream                                     */
} isdf_map_update_info;
void isdf_map_update_params_default(isdf_map_update_params *p);
void isdf_map_update_sizes(int sizes_out[2]);      /* sizeof of the two structs above, for mirrors of this header            */
int isdf_update_pointcloud(isdf_ctx *ctx, const float *xyz, long long n_points, const isdf_map_update_params *params,
                           isdf_map_update_info *info_out);
int isdf_update_voxels(isdf_ctx *ctx, const int32_t *ijk, long long n_voxels, const isdf_map_update_params *params,
                       isdf_map_update_info *info_out);
/* The kept per-voxel point counts, X * Y * Z values in the grid's own order; ISDF_ERR_STATE when there are none. */
int isdf_map_counts_get(isdf_ctx *ctx, uint32_t *counts_out);

/* ---- voxels cleared from the map in place --------------------------------------------------------------------- */
/* The inverse of the update above: occupancy that shrinks (a door opens, a moving obstacle has passed, a false return is corrected).
 * isdf_clear_pointcloud takes points OUT of the kept per-voxel counts (n_points x 3 floats, binned exactly as isdf_update_pointcloud
 * bins them: a point outside the box counts for voxel (0,0,0)).  A count never goes below 0: a point that finds its voxel's count at
 * 0 changes nothing and is counted in n_points_ignored.  A voxel whose count falls from >= sta_threshold to below it becomes free.
 * isdf_clear_voxels sets the listed voxels free (ijk = n_voxels x 3 indices; duplicates and free voxels are fine; an index outside
 * the grid: ISDF_ERR_INVALID_ARG, nothing changed); it invalidates kept counts when it frees a voxel.
 * Every derived product is refreshed only where it can change.  The ESDF can only rise, and only at a voxel whose old nearest
 * occupied voxel was cleared: those voxels are found from the old values (a conservative superset, the TOUCHED voxels) and their
 * bounding box is recomputed exactly - the integer squared distance to the nearest voxel still occupied, converted as
 * isdf_generate_esdf converts it.  The front end's inflated bit map is recomputed over the box of the cleared voxels and its
 * configuration-space table - and the A*'s host copy - over that box grown by (kernel_size - 1) / 2.
 * Afterwards every product is byte for byte what a fresh ctx holds after the from-scratch sequence: isdf_set_pointcloud(the old
 * cloud minus the removed points, as multisets) with the same explicit boundaries, resolution and threshold - for isdf_clear_voxels
 * isdf_set_grid of the new occupancy -, then isdf_generate_esdf, isdf_frontend_build and isdf_frontend_cspace where they had been
 * run.  As after an update the geometry, grid_epoch and the voxel indices handed out before stay, the occupancy bit grid and the ESDF
 * bricks are rebuilt lazily, and nothing is allocated after the first call of a size on the incremental path.
 * A clear OPENS bits of the configuration space, which the repair rule of isdf_frontend_field_set_repair is not proved for: that
 * switch does not bear on a clear.  A valid cost-to-go field is dropped (field_dropped = 1) in mode 0 of
 * isdf_frontend_field_set_reopen, the default, and lowered in place by a relaxation seeded at the opened voxels in mode 1
 * (field_dropped = 0).  Removed voxels cannot be subtracted from the piece minima of
 * a kept clearance report: with mode 1 of isdf_traj_check_set_watch an armed watch is re-checked against the whole new map
 * (watch_rechecked = 1; isdf_traj_watch_info: path 2, one more update folded, the new_* fields empty) and then reads as after
 * isdf_traj_check on the new map.  The V1 obstacle-point set and lastTstar are NOT touched: a caller who merged voxels that are now
 * cleared (isdf_points_merge_check) must rebuild the set, or the optimizer keeps avoiding them.  When no voxel became free nothing
 * but the counts changes.
 * A failure (ISDF_ERR_HIP) after the counts and the occupancy have moved drops the ESDF and the front end, as the update does.
 * isdf_clear_pointcloud: ISDF_ERR_STATE without kept counts.  Both: a multi-device ctx ISDF_ERR_UNSUPPORTED.  params may be NULL
 * (defaults), info_out may be NULL. */
typedef struct isdf_map_clear_params {
    int64_t max_cleared_voxels; /* more cleared voxels than this: rebuild everything (default 65536)                           */
    double full_fraction;       /* the grown dirty box, or the touched box of the ESDF, holds more than this share of the map's */
                                /* voxels: rebuild everything (default 0.5).  Placeholders, as the update's       */
    int32_t refresh_esdf;       /* 1 (default): refresh the ESDF if one is installed; 0: drop it                               */
    int32_t refresh_frontend;   /* 1 (default): refresh the front end if built; 0: release it                                  */
} isdf_map_clear_params;
typedef struct isdf_map_clear_info {
    int64_t n_points;                   /* points (or voxel entries) given                                                     */
    int64_t n_points_ignored;           /* points whose voxel's count was 0 already (0 in the voxel form)                      */
    int64_t n_cleared_voxels;           /* voxels that became free                                                             */
    int32_t dirty_lo[3], dirty_hi[3];   /* index box of the cleared voxels (inclusive; lo > hi when none)                      */
    int32_t touched_lo[3], touched_hi[3];       /* index box of the ESDF voxels recomputed on the incremental path (lo > hi: none) */
    int32_t path;                       /* 0 nothing changed, 1 incremental, 2 full rebuild (a cap of params exceeded, or - with */
                                        /*   an ESDF to refresh - no occupied voxel left)                                      */
    int32_t esdf_refreshed, frontend_refreshed, cspace_refreshed, host_table_patched;
    int32_t field_dropped;              /* 1: a VALID cost-to-go field was dropped by this call                                */
    int32_t watch_rechecked;            /* 1: an armed clearance watch was re-checked against the whole new map                */
    int32_t reserved;
    int64_t esdf_voxels_recomputed;     /* voxels of the touched box (the whole map on the full path)                          */
    int64_t esdf_voxels_raised;         /* incremental path: ESDF values that rose                                             */
    int64_t cspace_voxels_recomputed;   /* voxels of the grown box (the whole map on the full path)                            */
    double count_ms, esdf_ms, frontend_ms;      /* device time, events on the ctx's stream                                     */
} isdf_map_clear_info;
void isdf_map_clear_params_default(isdf_map_clear_params *p);
void isdf_map_clear_sizes(int sizes_out[2]);       /* sizeof of the two structs above, for mirrors of this header            */
int isdf_clear_pointcloud(isdf_ctx *ctx, const float *xyz, long long n_points, const isdf_map_clear_params *params,
                          isdf_map_clear_info *info_out);
int isdf_clear_voxels(isdf_ctx *ctx, const int32_t *ijk, long long n_voxels, const isdf_map_clear_params *params,
                      isdf_map_clear_info *info_out);
/* The ESDF raise in plain host code, no ctx and no device.  occ_new: the occupancy AFTER the clear (X * Y * Z bytes, 1 = occupied,
 * z fastest; dims = {X, Y, Z}, each in [1, 4096]); esdf_inout: on entry the exact transform of the map before the clear (what
 * isdf_generate_esdf gives for occ_new plus the cleared voxels), on return that of occ_new, the bytes of isdf_generate_esdf;
 * cleared_ijk: the n voxels that were occupied and are free in occ_new.  info_out (nullable): n_points = n_cleared_voxels = n, the
 * dirty and the touched box, esdf_voxels_recomputed / _raised, path 1 - or 2 when no occupied voxel is left -, the rest 0.
 * Returns ISDF_OK or ISDF_ERR_INVALID_ARG (a null array, a bad dimension or resolution, an index outside the grid). */
int isdf_clear_esdf_host(const uint8_t *occ_new, float *esdf_inout, const int32_t dims[3], double resolution, const int32_t *cleared_ijk,
                         long long n_cleared, isdf_map_clear_info *info_out);
/* The touched test alone, on the transform BEFORE the clear: touched_out (nullable) gets one byte per voxel, 1 = the voxel is
 * recomputed.  Returns the number of touched voxels, or a negative isdf_status. */
long long isdf_clear_touched_host(const float *esdf_old, const int32_t dims[3], double resolution, const int32_t *cleared_ijk, long long n_cleared,
                                  uint8_t *touched_out);

/* ---- a range scan integrated into the map: free space ray-cast on the device ----------------------------------- */
/* The producer of the two sections above: WHICH voxels to clear is what a range scan says - a ray that passes through a voxel proves
 * it empty.  isdf_integrate_scan takes the sensor's origin (3 doubles), the scan's end points (xyz = n_rays x 3 floats) and hit
 * (nullable, n_rays bytes: NULL = every ray ends on a surface, 0 = this ray ends in free space, e.g. a max-range reading the caller has
 * cut to length), traces the rays on the device and takes the kept per-voxel counts down along the rays and up at the hits.
 * The ray is defined in integers, so that the device and isdf_scan_ray_host visit the same voxels bit for bit.  A point is inside by
 * the binning's own test (no coordinate < the lower or > the upper boundary) and when it is finite; u = (p - bmin) / resolution in
 * fp64, q = floor(u * 1024) clamped to dim * 1024 - 1, voxel q >> 10 (the binning's voxel).  The ray runs between the tick centres
 * P = 2 q + 1; on axis a it takes |ve_a - vo_a| steps; the next step is on the axis, among those with steps left, whose next voxel
 * boundary comes first - m_a / D_a smallest, m_a = 2048 (v_a + 1) - Po_a or Po_a - 2048 v_a by direction, D_a = |Pe_a - Po_a|, compared
 * as m_a D_b < m_b D_a in 64-bit integers, a tie to the lowest axis.  The visited voxels are vo and every voxel entered: 1 + the sum
 * of the steps, the last one ve.
 * A ray whose end point is outside the map is skipped whole (n_rays_skipped; it does NOT count for voxel (0,0,0): a ray is no map
 * point); an origin outside: ISDF_ERR_INVALID_ARG, nothing changed.  H = the multiset of the end voxels of the hit rays.  F = the SET
 * of voxels visited by any ray - a hit ray's end voxel left out, a no-hit ray's included - minus every voxel of H: a voxel hit in this
 * scan is never counted down by it.  counts'[v] = max(counts[v] - miss_weight, 0) on F, counts[v] + multiplicity on H; occupancy is
 * counts' >= sta_threshold.  F is a set per scan, not a sum per ray: the voxel next to the sensor that every ray crosses loses
 * miss_weight once, and the result depends neither on the order of the rays nor on the order of the device's atomics.
 * The call IS this sequence, and every product - counts, occupancy, ESDF, inflated bit map, configuration-space table, the A*'s host
 * copy, the cost-to-go field in every repair / reopen mode, a kept clearance report - is byte for byte what a second ctx holds after
 * it: isdf_clear_pointcloud of miss_weight copies of the centre of every voxel of F (params.clear), then isdf_update_pointcloud of
 * the end points of the hit rays that were not skipped (params.update).  The frees are applied and refreshed first, then the hits;
 * info.clear and info.update are what those two calls report (the *_ms apart).  A failure after counts or occupancy moved drops the
 * ESDF and the front end, as those calls do.  Nothing is allocated after the first call of a size beyond what the two stages allocate.
 * ISDF_ERR_STATE without kept counts; a multi-device ctx ISDF_ERR_UNSUPPORTED; n_rays = 0 is legal (path 0 twice).  params may be
 * NULL (defaults), info_out may be NULL.  Not offered: a voxel form for maps from isdf_set_grid; one merged refresh of both directions. */
typedef struct isdf_map_scan_params {
    int32_t miss_weight;        /* taken off the count of every voxel of F, default 1; < 0: ISDF_ERR_INVALID_ARG; 0: only the hits count */
    int32_t reserved;
    isdf_map_clear_params clear;    /* handed to the clear stage  */
    isdf_map_update_params update;  /* handed to the update stage */
} isdf_map_scan_params;
typedef struct isdf_map_scan_info {
    int64_t n_rays, n_rays_skipped, n_hits;     /* given; end point outside the map; hit rays that were not skipped */
    int64_t n_free_voxels, n_hit_voxels;        /* |F|; distinct voxels of H                                        */
    int32_t ray_lo[3], ray_hi[3];               /* index box of every visited voxel (lo > hi: no ray traced)        */
    double trace_ms;                            /* device time of the ray stage, events on the ctx's stream         */
    isdf_map_clear_info clear;                  /* as isdf_clear_pointcloud of the two-call sequence reports        */
    isdf_map_update_info update;                /* as isdf_update_pointcloud of it reports                          */
} isdf_map_scan_info;
void isdf_map_scan_params_default(isdf_map_scan_params *p);     /* null-safe */
void isdf_map_scan_sizes(int sizes_out[2]);                     /* null-safe; sizeof of the two structs above */
int isdf_integrate_scan(isdf_ctx *ctx, const double origin[3], const float *xyz, const uint8_t *hit, long long n_rays,
                        const isdf_map_scan_params *params, isdf_map_scan_info *info_out);
/* plain host code, no ctx, no device: the sets of one scan.  bmin / bmax / resolution / dims: the map's geometry (each dim in
 * [1, 4096]).  free_out (nullable): one byte per voxel, 1 = in F; hits_out (nullable): uint32 per voxel, the multiplicity in H;
 * n_skipped_out (nullable).  Returns |F| or a negative isdf_status (ISDF_ERR_INVALID_ARG: a null array, a bad geometry, an origin
 * outside the map). */
long long isdf_scan_sets_host(const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], const double origin[3],
                              const float *xyz, const uint8_t *hit, long long n_rays, uint8_t *free_out, uint32_t *hits_out, long long *n_skipped_out);
/* one ray's visited voxels, for tests and callers who want the list: ijk_out = capacity x 3; returns their number (also when it
 * exceeds capacity), 0 when the end point lies outside the map or is not finite, or a negative isdf_status */
long long isdf_scan_ray_host(const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], const double origin[3],
                             const float end[3], int32_t *ijk_out, long long capacity);

/* ---- rays cast through the map: the first occupied voxel per ray, on the device --------------------------------- */
/* The read-only counterpart of the scan: the same ray, quantised and walked exactly as the section above defines it, testing the
 * occupancy and stopping at the first occupied voxel.  A cast visits the voxels isdf_integrate_scan would write for the same ray.
 * Ray i runs from origin o_i (fp64; origins = 3 doubles shared by all rays, or n x 3 with params.per_ray_origin) to end point e_i
 * (ends = n x 3 floats, widened to fp64 as the scan widens them) and writes one row of eight int32 (32 bytes):
 *   {status, steps, i, j, k, axis, num, den}
 * status 3: o_i is outside the map or not finite (per-ray origins only).  status 2: e_i is outside or not finite (the scan's
 * "skipped").  Otherwise the walk from o_i's voxel - voxel 0, tested only when params.test_origin_voxel != 0 - towards e_i's;
 * status 1: the first tested voxel whose occupancy byte is not 0 ends the walk; status 0: the walk reaches e_i's voxel without one.
 * steps: the 0-based index in the walk of the voxel (i, j, k) where it ended - the hit voxel, or e_i's voxel with steps = the sum of
 * the steps on the three axes.  axis, num, den: where the ray entered that voxel - the axis of the last step taken, that axis's m
 * before the step and its D, so that Po + (Pe - Po) * num / den (P = 2 q + 1, the tick centres in half ticks) is the crossing point,
 * which lies on the voxel's face across `axis`; both are below 2^24.  A walk that ended at voxel 0: axis -1, num 0, den 1.  Status 2
 * and 3 rows: {status, -1, -1, -1, -1, -1, 0, 1}.  Everything in a row is an integer: isdf_raycast_host and the device agree byte
 * for byte; ranges and points in metres are the caller's arithmetic on the row.
 * A shared origin outside the map: ISDF_ERR_INVALID_ARG, nothing written.  ISDF_ERR_STATE without an occupancy grid (a map from
 * isdf_set_grid with ISDF_GRID_OCCUPANCY is served: no kept counts are needed); a multi-device ctx ISDF_ERR_UNSUPPORTED; n = 0 is
 * legal (every array but a shared origin may then be NULL); params may be NULL (defaults), info_out may be NULL.  The call is
 * read-only: no map product, epoch, dirty flag, kept field, watch or report changes.  Rays are not clipped to the map: the caller
 * clips.
 * isdf_map_raycast stages through grow-only buffers of its own: nothing is allocated after the first call of a size.
 * isdf_map_raycast_device: d_ends (n x 3 floats) and d_rows_out (n x 8 int32, 16-byte aligned) are device memory, the work is put on
 * `stream`; d_origins is device memory (n x 3 doubles) with per_ray_origin, and 3 doubles on the HOST without - a shared origin is an
 * argument of the call, as the scan's is, and is tested before anything is launched.  With info_out == NULL it hands nothing over and
 * does not synchronise; with info_out it synchronises `stream` once. */
typedef struct isdf_map_raycast_params {
    int32_t test_origin_voxel;   /* default 0: a sensor sits in free space, a line of sight may start in an occupied voxel */
    int32_t per_ray_origin;      /* default 0: origins = 3 doubles for all rays; 1: n x 3                                   */
    int32_t reserved[2];
} isdf_map_raycast_params;
typedef struct isdf_map_raycast_info {
    int64_t n_rays, n_skipped, n_origin_outside, n_hits, n_clear;      /* given; rows of status 2, 3, 1, 0 */
    int64_t steps_total;         /* sum of steps over status 0 and 1 */
    double  cast_ms;             /* device time, events on the ctx's stream (the device form: on `stream`) */
} isdf_map_raycast_info;
void isdf_map_raycast_params_default(isdf_map_raycast_params *p);   /* null-safe */
void isdf_map_raycast_sizes(int sizes_out[2]);                      /* null-safe; sizeof of the two structs above */
int isdf_map_raycast(isdf_ctx *ctx, const double *origins, const float *ends, long long n, const isdf_map_raycast_params *params,
                     int32_t *rows_out, isdf_map_raycast_info *info_out);
int isdf_map_raycast_device(isdf_ctx *ctx, const double *d_origins, const float *d_ends, long long n, const isdf_map_raycast_params *params,
                            int32_t *d_rows_out, isdf_map_raycast_info *info_out, void *stream);
/* plain host code, no ctx, no device: the same rows from occupancy bytes (X * Y * Z, z fastest) and the map's geometry (each dim in
 * [1, 4096]).  Returns n_hits or a negative isdf_status (ISDF_ERR_INVALID_ARG: a null array, a bad geometry, a shared origin outside
 * the map - nothing written). */
long long isdf_raycast_host(const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                            const double *origins, const float *ends, long long n, const isdf_map_raycast_params *params, int32_t *rows_out);

/* ---- the depth camera: a depth image rendered on the device, and one integrated into the map -------------------- */
/* The sensor of the reference is a simulated depth camera (src/uav_simulator/local_sensing/src/depth_render.cu:2-56, driven by
 * pcl_render_node.cpp:271-296, unprojected again in render_pcl_world, :224-269; intrinsics in local_sensing/params/camera.yaml).
 * The camera: width, height in [1, 4096], fx, fy > 0, cx, cy, all finite.  The pose is cam2world: 12 doubles, the rows (R | t) of
 * the rigid 4x4, row-major, z the optical axis, all finite.  Anything else: ISDF_ERR_INVALID_ARG.
 *
 * RENDER.  image = height x width int32 millimetres, row-major, 999999 where nothing reached the pixel (depth_initial).
 * world2cam = (R^T, -R^T t), formed in fp64 - the translation's row i is -(R_0i t_0 + R_1i t_1 + R_2i t_2), summed left to right -
 * and rounded to float32 once; fx_f = (float)fx, fy_f = (float)fy as the reference's Parameter holds them; cx, cy stay fp64.  Per point
 * (x, y, z), float32, nothing contracted into an FMA (depth_render.cu:12-32):
 *   X = x * w00 + y * w01 + z * w02 + w03, Y and Z likewise from rows 1 and 2, each summed left to right
 *   not (Z > 0): dropped, n_behind (the reference's Z <= 0; a NaN too).  Z < (float)min_depth_m: dropped, n_near.
 *   px = (int)((double)(X / Z * fx_f) + cx + 0.5), py = (int)((double)(Y / Z * fy_f) + cy + 0.5): the conversion truncates towards
 *   zero, so a value in (-1, 0) lands in column (row) 0, as in the reference.  Stated without the conversion's overflow: the point is
 *   kept when the fp64 value v satisfies -1 < v < width (height), otherwise dropped, n_outside (the centre pixel must be in the image,
 *   depth_render.cu:23).
 *   dist_mm = (int)(Z * 1000.0f + 0.5f) in float32 (2^31 or more: INT32_MAX, which changes no pixel)
 *   r = (int)(splat_m * (double)fx_f / (double)Z + (double)0.5f) - the reference's `0.0573 * para.fx / dist + 0.5f`: double * float /
 *   float + float, all promoted to double -, 4096 when that is 4096 or more (it then covers any image), then at most max_splat_px
 *   when that is > 0.
 *   every pixel (px + j, py + i), -r <= i, j <= r, inside the image takes min(its value, dist_mm).
 * A minimum over integers does not depend on the order of the atomics: isdf_depth_render_host gives the device's image byte for byte.
 * ISDF_DEPTH_SOURCE_CLOUD renders xyz (n x 3 floats; n = 0 is legal: every pixel 999999).  ISDF_DEPTH_SOURCE_MAP renders the centres
 * of the ctx's occupied voxels, bmin + (v + 0.5) * resolution in fp64 rounded to float32, in one pass over the occupancy bytes that
 * uploads nothing (xyz and n are ignored); ISDF_ERR_STATE without an occupancy grid.
 * info: n_points (given, or the occupied voxels), n_behind, n_near, n_outside, n_splat_pixels = the sum of the clipped windows' sizes,
 * n_pixels_set = pixels that are not 999999 at the end, render_ms.  All counts are sums: the host form repeats them (render_ms 0).
 * The call is read-only, like the ray cast; a multi-device ctx: ISDF_ERR_UNSUPPORTED.  isdf_depth_render stages through grow-only
 * buffers of its own: nothing is allocated after the first call of a size.  isdf_depth_render_device: d_xyz and d_image_out are device
 * memory, the work (the clear of the image included) is put on `stream`; with info_out == NULL nothing is counted, handed over or
 * synchronised, with it `stream` is synchronised once.  params may be NULL (defaults). */
#define ISDF_DEPTH_SOURCE_CLOUD 0
#define ISDF_DEPTH_SOURCE_MAP 1
#define ISDF_DEPTH_EMPTY_MM 999999
typedef struct isdf_depth_camera {
    int32_t width, height;
    double fx, fy, cx, cy;
} isdf_depth_camera;
typedef struct isdf_depth_render_params {
    double splat_m;             /* default 0.0573, the reference's live constant; >= 0                                         */
    double min_depth_m;         /* default 0; a point nearer than this is dropped; >= 0                                        */
    int32_t max_splat_px;       /* default 0 = unlimited, as in the reference (at Z = 0.1 m its r is 222: 198 025 pixels from   */
                                /* one point); otherwise r is clamped to it; < 0: ISDF_ERR_INVALID_ARG                         */
    int32_t source;             /* ISDF_DEPTH_SOURCE_*                                                                         */
    int32_t reserved[4];
} isdf_depth_render_params;
typedef struct isdf_depth_render_info {
    int64_t n_points, n_behind, n_outside, n_near, n_splat_pixels, n_pixels_set;
    double render_ms;           /* device time, events on the ctx's stream (the device form: on `stream`), the clear included   */
} isdf_depth_render_info;
void isdf_depth_render_params_default(isdf_depth_render_params *p);     /* null-safe */
void isdf_depth_render_sizes(int sizes_out[3]);                         /* null-safe; sizeof of the three structs above */
int isdf_depth_render(isdf_ctx *ctx, const isdf_depth_camera *camera, const double cam2world[12], const float *xyz, long long n,
                      const isdf_depth_render_params *params, int32_t *image_out, isdf_depth_render_info *info_out);
int isdf_depth_render_device(isdf_ctx *ctx, const isdf_depth_camera *camera, const double cam2world[12], const float *d_xyz, long long n,
                             const isdf_depth_render_params *params, int32_t *d_image_out, isdf_depth_render_info *info_out, void *stream);
/* plain host code, no ctx, no device.  The map source reads occ (X * Y * Z bytes, z fastest), bmin, resolution and dims (each in
 * [1, 4096]); the cloud source ignores them (they may be NULL).  Returns an isdf_status. */
int isdf_depth_render_host(const isdf_depth_camera *camera, const double cam2world[12], const float *xyz, long long n, const uint8_t *occ,
                           const double bmin[3], double resolution, const int32_t dims[3], const isdf_depth_render_params *params,
                           int32_t *image_out, isdf_depth_render_info *info_out);

/* RAYS.  A depth image turned into the (xyz, hit) arrays isdf_integrate_scan takes, cut to range and clipped to the map, which the
 * scan asks of its caller.  Formats: ISDF_DEPTH_I32_MM, the render's own output: a value >= 500000 is no return
 * (pcl_render_node.cpp:293), and so is a value <= 0, which no surface in front of the camera gives; ISDF_DEPTH_U16_MM: 0 is no
 * return; ISDF_DEPTH_F32_M: 0, a negative or a non-finite value is no return.
 * The output always has n = ceil(width / stride_u) * ceil(height / stride_v) rows (isdf_depth_rays_rows), ray k = iv * nu + iu for
 * pixel (u, v) = (iu * stride_u, iv * stride_v): v is the outer index.  A dropped pixel's row is three times the one float32 NaN
 * 0x7FC00000 with hit 0: the scan skips a non-finite end point, so nothing is compacted and the order is fixed.
 * Per kept pixel, in fp64, nothing contracted (render_pcl_world, pcl_render_node.cpp:241-246):
 *   d = mm / 1000.0, or the float widened
 *   p = ((u - cx) * d / fx, (v - cy) * d / fy, d);  e_a = R_a0 p_0 + R_a1 p_1 + R_a2 p_2 + t_a, summed left to right;  o = t
 *   range = sqrt(dx * dx + dy * dy + dz * dz) of e - o, summed left to right
 *   range < min_range_m: dropped (n_below_min).  range > max_range_m: e = o + (e - o) * (max_range_m / range), hit 0 (n_truncated).
 *   no return (n_no_return): dropped - or, with no_return_is_free, the same with d = 1 and e = o + (e - o) * (max_range_m / range),
 *   hit 0: a ray of length max_range_m along the pixel's direction, neither the minimum nor n_truncated applies.
 *   clip: box = [bmin + resolution / 2, bmax - resolution / 2] per axis.  On every axis a where e_a lies outside it
 *   s_a = (bound_a - o_a) / (e_a - o_a) (0 when e_a == o_a); s = the smallest of them held to [0, 1]; e = o + (e - o) * s, hit 0
 *   (n_clipped).  e - o is the difference of the e just formed and o.
 *   the end point is rounded to float32 (a row that is not finite after that is dropped); hit = 1 counts in n_hits.
 * Only + - * / and sqrt appear, correctly rounded on both sides: isdf_depth_rays_host gives the device's rows byte for byte.
 * isdf_depth_rays needs the ctx's map geometry only (ISDF_ERR_STATE without a grid; a multi-device ctx: ISDF_ERR_UNSUPPORTED) and is
 * read-only; it stages through grow-only buffers of its own, as the render does.  A camera outside the map
 * (the scan's test of its origin): ISDF_ERR_INVALID_ARG, as are a stride < 1, min_range_m < 0, max_range_m <= 0 or NaN, an unknown
 * format, and no_return_is_free with an infinite max_range_m.  isdf_depth_rays_device: d_image, d_ends_out (n x 3 floats) and
 * d_hit_out (n bytes) are device memory, the work is put on `stream`; info_out as for the render. */
#define ISDF_DEPTH_I32_MM 0
#define ISDF_DEPTH_U16_MM 1
#define ISDF_DEPTH_F32_M 2
typedef struct isdf_depth_rays_params {
    int32_t stride_u, stride_v; /* default 1: every pixel; >= 1                                                                 */
    double min_range_m;         /* default 0                                                                                   */
    double max_range_m;         /* default +inf; > 0                                                                           */
    int32_t no_return_is_free;  /* default 0                                                                                   */
    int32_t reserved[3];
} isdf_depth_rays_params;
typedef struct isdf_depth_rays_info {
    int64_t n_pixels, n_no_return, n_below_min, n_truncated, n_clipped, n_hits;     /* n_pixels: the rows written */
    double rays_ms;             /* device time of the unprojection                                                             */
} isdf_depth_rays_info;
void isdf_depth_rays_params_default(isdf_depth_rays_params *p);         /* null-safe */
void isdf_depth_rays_sizes(int sizes_out[2]);                           /* null-safe; sizeof of the two structs above */
long long isdf_depth_rays_rows(const isdf_depth_camera *camera, const isdf_depth_rays_params *params);     /* n, or ISDF_ERR_INVALID_ARG; params NULL: strides 1 */
int isdf_depth_rays(isdf_ctx *ctx, const isdf_depth_camera *camera, const double cam2world[12], const void *image, int format,
                    const isdf_depth_rays_params *params, float *ends_out, uint8_t *hit_out, isdf_depth_rays_info *info_out);
int isdf_depth_rays_device(isdf_ctx *ctx, const isdf_depth_camera *camera, const double cam2world[12], const void *d_image, int format,
                           const isdf_depth_rays_params *params, float *d_ends_out, uint8_t *d_hit_out, isdf_depth_rays_info *info_out,
                           void *stream);
/* plain host code, no ctx, no device; the map's geometry as isdf_scan_sets_host takes it.  Returns n_hits or a negative isdf_status. */
long long isdf_depth_rays_host(const isdf_depth_camera *camera, const double cam2world[12], const void *image, int format,
                               const isdf_depth_rays_params *params, const double bmin[3], const double bmax[3], double resolution,
                               const int32_t dims[3], float *ends_out, uint8_t *hit_out, isdf_depth_rays_info *info_out);
/* INTEGRATE.  By definition isdf_integrate_scan(ctx, t, ends, hit, n, scan_params, scan_info_out) with the arrays
 * isdf_depth_rays_host gives for (camera, cam2world, image, format, rays_params) and the ctx's map: every product and every count of
 * isdf_map_scan_info but the *_ms is that call's.  Here the image alone is uploaded; the unprojection writes the end points and the hit
 * bytes on the device straight into the scan's staged input, and the scan's trace, apply and hit stages run as they are (trace_ms
 * includes the unprojection; depth_info_out->rays_ms is its own time).  The errors are the scan's and the camera's, all before
 * anything moves.  Both infos may be NULL.  Not offered: an image that is on the device already. */
int isdf_integrate_depth(isdf_ctx *ctx, const isdf_depth_camera *camera, const double cam2world[12], const void *image, int format,
                         const isdf_depth_rays_params *rays_params, const isdf_map_scan_params *scan_params,
                         isdf_depth_rays_info *depth_info_out, isdf_map_scan_info *scan_info_out);

/* ---- the map window shifted in place, so that the map can follow the robot -------------------------------------- */
/* Every call above keeps the box (bmin, bmax, dims) that isdf_set_pointcloud fixed.  isdf_shift_map moves the window by
 * s = shift_ijk voxels: new voxel v holds what old voxel v + s held, a voxel whose source lies outside the old grid has count 0, and
 * bmin' = bmin + s * resolution, bmax' = bmax + s * resolution per axis (one fp64 product, one sum, nothing contracted).  If
 * isdf_set_pointcloud's own ceil((bmax' - bmin') / resolution) does not give the same dims on every axis the call fails with
 * ISDF_ERR_INVALID_ARG and changes nothing (isdf_shift_geometry_host is this rule).
 * After the call every product that had been built - kept counts, occupancy, ESDF, inflated bit map, configuration-space table on
 * the device and in the A*'s host copy - is byte for byte what a fresh ctx holds after isdf_set_pointcloud on a cloud with the
 * translated counts in the box (bmin', bmax') followed by whichever of isdf_generate_esdf, isdf_frontend_build and
 * isdf_frontend_cspace had been run.  Counts, occupancy and the table are translated into second buffers that then change places with
 * the first (one more copy of each stays allocated); the ESDF is transformed whole; of the table only the bands a translation cannot
 * supply are recomputed (isdf_shift_bands_host) - path 1 - unless their volume exceeds full_fraction of the map, no voxel is
 * occupied any more, or |s| >= dims on some axis (everything left: the empty map) - path 2, the whole-map kernels, the host copy
 * marked stale.  s = 0: path 0, nothing is touched.
 * Voxel indices change their meaning: the grid epoch advances (a report of isdf_traj_check from before the shift is stale for
 * isdf_points_merge_check), a valid cost-to-go field is dropped (field_dropped) or, with isdf_frontend_field_set_shift(1), carried
 * towards the same cell at its new index (field_dropped = 0), an armed clearance watch (isdf_traj_check_set_watch) is checked again against the new map and stays armed (watch_rechecked).  The obstacle-point set, lastTstar and a kept swept mesh
 * are world-space and stay.  A failure after the counts moved drops the ESDF and the front end, as a failing update does.
 * ISDF_ERR_UNSUPPORTED on a multi-device ctx, ISDF_ERR_STATE without a map or without kept counts (a map from isdf_set_grid).
 * Nothing is allocated after the first call of a size beyond what isdf_generate_esdf and the watch's re-check allocate.
 * params may be NULL (defaults), info_out may be NULL.  Not offered: an incremental ESDF. */
#define ISDF_MAP_SHIFT_NONE 0
#define ISDF_MAP_SHIFT_INCREMENTAL 1
#define ISDF_MAP_SHIFT_FULL 2
typedef struct isdf_map_shift_params {
    double full_fraction;       /* bands above this share of the map: path 2; default 0.5; < 0 or NaN: ISDF_ERR_INVALID_ARG     */
    int32_t force_path;         /* 0: as decided; 1: path 1 unless everything left; 2: path 2; else ISDF_ERR_INVALID_ARG        */
    int32_t reserved[5];
} isdf_map_shift_params;
typedef struct isdf_map_shift_info {
    int32_t path;               /* ISDF_MAP_SHIFT_*                                                                              */
    int32_t shift[3];           /* the shift applied                                                                             */
    double bmin_new[3];         /* the map's origin after the call                                                               */
    int64_t voxels_entered;     /* voxels of the new window without a source                                                     */
    int64_t occupied_left;      /* occupied voxels of the old window without a destination                                       */
    int64_t counts_left;        /* the sum of their and every other leaving voxel's kept counts                                  */
    int32_t n_boxes;            /* bands of the configuration space recomputed (path 1 with a table; else 0)                      */
    int32_t host_table_patched; /* the A*'s host copy was translated and patched in place                                        */
    int32_t field_dropped, watch_rechecked;
    int64_t cspace_voxels;      /* configuration-space words recomputed (the bands' volumes; the map on path 2)                  */
    double translate_ms, esdf_ms, frontend_ms;      /* device time, events on the ctx's stream                                    */
    double wall_ms;             /* the whole call on the host's clock                                                            */
} isdf_map_shift_info;
void isdf_map_shift_params_default(isdf_map_shift_params *p);    /* null-safe */
void isdf_map_shift_sizes(int sizes_out[2]);                     /* null-safe; sizeof of the two structs above */
int isdf_shift_map(isdf_ctx *ctx, const int32_t shift_ijk[3], const isdf_map_shift_params *params, isdf_map_shift_info *info_out);
/* Host arithmetic around isdf_shift_map: s_a = the voxel of centre_xyz (the binning's floor((x - bmin) / resolution), not clamped:
 * a centre outside the map is fine) minus dims_a / 2.  max |s_a| < min_shift: nothing happens, shift_out = 0, path 0.  Otherwise
 * isdf_shift_map(s); shift_out (nullable) = s on success, 0 on failure.  A non-finite centre, a negative min_shift or a voxel index
 * beyond int32: ISDF_ERR_INVALID_ARG. */
int isdf_map_follow(isdf_ctx *ctx, const double centre_xyz[3], int min_shift, const isdf_map_shift_params *params, int32_t shift_out[3],
                    isdf_map_shift_info *info_out);
/* plain host code, no ctx, no device.  The shifted box and the dims guard: ISDF_OK and the new box, or ISDF_ERR_INVALID_ARG (a null
 * array, resolution <= 0, a dim outside [1, 4096], or the guard; the outputs are then unspecified). */
int isdf_shift_geometry_host(const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], const int32_t shift[3],
                             double bmin_out[3], double bmax_out[3]);
/* out[v] = in[v + shift] where v + shift lies in the grid, zero elsewhere: elements of elem_bytes bytes, z fastest.  in == out is
 * allowed (this is how the A*'s host table is shifted); the arrays must not overlap otherwise. */
int isdf_shift_grid_host(const void *in, int elem_bytes, const int32_t dims[3], const int32_t shift[3], void *out);
/* The bands of the configuration space a shift recomputes, side = (kernel_size - 1) / 2 >= 0: per shifted axis the entering slab
 * grown by side and the side-thick band at the opposite face, over the whole extent of the other axes, clamped, empty ones left out:
 * boxes_out[i] = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z}, inclusive, *n_boxes_out <= 6.  The boxes may overlap. */
int isdf_shift_bands_host(const int32_t dims[3], const int32_t shift[3], int side, int32_t boxes_out[6][6], int *n_boxes_out);

/* ---- observed space in the map: the known grid and the frontier ---------------------------------------------------- */
/* The map above has two states per voxel, occupied or not; a voxel no ray has ever crossed reads like one a thousand rays have proved
 * empty, and the slab that enters the window in isdf_shift_map is "free".  The known grid is the third state: ONE BIT per voxel, voxel
 * a = (x * ny + y) * nz + z is bit a & 31 of uint32 word a >> 5, ceil(nx ny nz / 32) words, the bits beyond the last voxel always 0.
 * 1 = some ray has visited the voxel or the caller declared it known; 0 = unknown.  The feature is opt-in: with the mode off every
 * call above runs the launches it ran before, in the same order.
 * isdf_map_known_enable(ctx, 1): the ctx keeps a known grid K for its map.  If a map with kept counts exists K is allocated now, all
 * unknown; otherwise when the next isdf_set_pointcloud makes one.  A second enable(1) changes nothing.  enable(0) releases the grid and
 * its scratch.  The mode outlives maps: isdf_set_pointcloud and isdf_set_grid reset K to all unknown at the new size (after
 * isdf_set_grid K serves fill, get and frontier; the scan and the shift need kept counts anyway).  A multi-device ctx:
 * ISDF_ERR_UNSUPPORTED.  The grid, its second buffer and the scratch of fill, get and frontier grow only: those calls, the merge and the
 * translation allocate nothing on a second call of a size (isdf_debug_live_bytes).  isdf_traj_known_horizon does, as isdf_traj_check does:
 * its events and candidate buffers are scoped to the call.
 * Merge: isdf_integrate_scan and isdf_integrate_depth, when K exists, end their ray stage with K' = K u V, V = every voxel visited by
 * any ray that was not skipped - in terms of isdf_scan_sets_host free_out[v] != 0 or hits_out[v] > 0.  One extra kernel on the ctx's
 * stream after the trace and before the scan's first hand-over, whose record brings the number of new bits back: no synchronisation of
 * its own, no second read-back.  miss_weight = 0 still merges; n_rays = 0 merges nothing (and is not counted in `merges`); a call
 * refused before anything moves leaves K alone.  Every other product of the scan is byte for byte what it is with the mode off.
 * isdf_update_* and isdf_clear_* leave K alone: a caller's assertion about occupancy is not an observation.
 * Shift: isdf_shift_map / isdf_map_follow translate K on both paths, K'[v] = K[v + s] where v + s lies in the old grid, else 0 - the
 * entering slab is unknown; |s_a| >= dims_a on some axis: all unknown; s = 0: untouched.  The translation goes into a second buffer
 * that changes places with the first, inside the translation stage and under its hand-over.
 * isdf_map_known_fill: box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z}, inclusive, or NULL for the whole map; value != 0 sets the bits of the
 * box, 0 clears them - this is how an a-priori map is declared known.  A box outside the grid or with lo > hi on some axis:
 * ISDF_ERR_INVALID_ARG, nothing changed.
 * isdf_map_known_get: bits_out (nullable) = the words of K; info_out (nullable) is computed from K on the device when asked for.
 * isdf_map_frontier: voxel v is a frontier voxel iff K[v] = 1, its occupancy byte is 0, and some 6-neighbour INSIDE the grid has
 * K = 0 - the window's faces are not frontiers by themselves.  Computed on demand from the current K and occupancy; nothing is kept.
 * bits_out (nullable): the frontier in K's layout; vox_out (nullable, capacity entries): the frontier voxels' indices in ASCENDING
 * order, the same bytes on every run (counts, an exclusive scan, an emit pass: no atomics); a non-null vox_out with capacity <
 * n_frontier: ISDF_ERR_OVERFLOW with info_out (and bits_out) filled and the list untouched.
 * Every call but enable: ISDF_ERR_STATE without a known grid; the frontier also without an occupancy grid.
 * Not offered: a device-pointer form of the frontier; frontiers of the robot's configuration space; unknown space treated as an obstacle. */
typedef struct isdf_map_known_info {
    int64_t n_known, n_unknown;     /* bits set; voxels of the grid minus them                                                      */
    int32_t lo[3], hi[3];           /* index box of the known voxels (lo > hi: none)                                                */
    int64_t newly_known;            /* voxels the last successful merge or fill turned from 0 to 1                                  */
    int64_t merges;                 /* scans merged since the grid was last reset                                                   */
} isdf_map_known_info;
typedef struct isdf_map_frontier_info {
    int64_t n_frontier;
    int32_t lo[3], hi[3];           /* index box of the frontier voxels (lo > hi: none)                                             */
    double kernel_ms;               /* device time of the frontier kernel, events on the ctx's stream (the host form: 0)            */
} isdf_map_frontier_info;
/* The known horizon of a trajectory: the earliest time at which the robot's body comes within the margin of an unseen voxel - how far
 * a plan may be executed before the map must be looked at again.  isdf_traj_check's three steps with another predicate and
 * another reduction.  select: the UNKNOWN voxels (K = 0, occupied or not) within far_r of a coarse sample, in ascending voxel index - the
 * check's row kernel with "known bit clear" in place of "occupancy byte set".  field: the swept-volume query in params.mode at their
 * centres.  reduce: integer-keyed minima and integer sums only, so two runs give the same bytes.  margin and mode: isdf_traj_check_params'
 * rules and defaults.  Own scratch: the kept report of isdf_traj_check, an armed watch, the V1 points and lastTstar are untouched; more
 * than 2^31 candidates ISDF_ERR_OVERFLOW.  No known grid: ISDF_ERR_STATE; every other error as isdf_traj_check's.  The _device form takes
 * the trajectory on the device, works on `stream` (after the ctx's own stream has drained) and synchronises it before it returns. */
typedef struct isdf_traj_known_params {
    double margin;               /* negative (default) = cfg.safety_hor; above 2 safety_hor + 0.1: ISDF_ERR_INVALID_ARG             */
    int32_t mode;                /* ISDF_SWEPT_FIELD_PLANNER (default) or ISDF_SWEPT_FIELD_CLOSED                                   */
    int32_t reserved;
} isdf_traj_known_params;
typedef struct isdf_traj_known_info {
    int64_t unknown_in_box;      /* unknown voxels of the selection box (all of the grid if !culled)                                */
    int64_t candidates;          /* of them, those put through the field query                                                      */
    int64_t qualified;           /* candidates with a qualifying interval (value != 10)                                             */
    int64_t n_below_margin;      /* qualified candidates with value < margin                                                        */
    int64_t n_penetrating;       /* ... with value < 0                                                                              */
    double horizon_t;            /* the smallest t* among the candidates with value < margin; -1: there are none                    */
    int64_t horizon_voxel;       /* the lexicographic minimum of (t*, voxel index) (-1: none)                                       */
    double horizon_value;        /* its value (10: none)                                                                            */
    double horizon_point[3];     /* its voxel centre                                                                                */
    int32_t horizon_piece;       /* the piece horizon_t lies in (Trajectory::locatePieceIdx; -1: none)                              */
    int32_t culled;              /* as isdf_traj_check_info's                                                                       */
    double min_clearance;        /* smallest value over the unknown candidates (10: nothing qualified), ties to the lowest voxel    */
    int64_t min_voxel;           /* its voxel index (-1: nothing qualified)                                                         */
    double duration;             /* the sum of T                                                                                    */
    double margin, far_r;        /* the margin in force; the selection radius (0 if !culled)                                        */
    double select_ms, field_ms, reduce_ms;       /* device time of the three steps (events on the stream)                           */
} isdf_traj_known_info;
void isdf_traj_known_params_default(isdf_traj_known_params *p);  /* null-safe */
int isdf_traj_known_horizon(isdf_ctx *ctx, int N, const double *T, const double *coeffs, const isdf_traj_known_params *params,
                            isdf_traj_known_info *info_out);
int isdf_traj_known_horizon_device(isdf_ctx *ctx, int N, const double *d_T, const double *d_coeffs, const isdf_traj_known_params *params,
                                   isdf_traj_known_info *info_out, void *stream);
void isdf_map_known_sizes(int sizes_out[4]);                     /* null-safe; sizeof of isdf_map_known_info, isdf_map_frontier_info, isdf_traj_known_params, isdf_traj_known_info */
int isdf_map_known_enable(isdf_ctx *ctx, int on);
int isdf_map_known_fill(isdf_ctx *ctx, const int32_t *box, int value);
/* instrument (tools/map_known_bench.py): enable != 0 puts a pair of events round the merge kernel of every later scan; ms_out (nullable)
 * receives the device time of the last merge so timed, -1 if there is none.  Off by default: no event is recorded then. */
int isdf_map_known_merge_ms(isdf_ctx *ctx, int enable, double *ms_out);
int isdf_map_known_get(isdf_ctx *ctx, uint32_t *bits_out, isdf_map_known_info *info_out);
int isdf_map_frontier(isdf_ctx *ctx, uint32_t *bits_out, int64_t *vox_out, long long capacity, isdf_map_frontier_info *info_out);
/* plain host code, no ctx, no device; dims = {nx, ny, nz}, each in [1, 4096]; the same arithmetic the kernels run (map_known_host.hpp).
 * merge: bits |= V from isdf_scan_sets_host's outputs (either nullable); returns the bits that went from 0 to 1.  shift: bits_out =
 * bits_in translated (the arrays must differ).  fill: as isdf_map_known_fill; returns the bits that went from 0 to 1.  frontier: occ =
 * nx ny nz occupancy bytes; outputs and ISDF_ERR_OVERFLOW as isdf_map_frontier.  Bad arguments: ISDF_ERR_INVALID_ARG (negative). */
long long isdf_known_merge_host(uint32_t *bits_inout, const int32_t dims[3], const uint8_t *free_bytes, const uint32_t *hits_u32);
int isdf_known_shift_host(const uint32_t *bits_in, const int32_t dims[3], const int32_t shift[3], uint32_t *bits_out);
long long isdf_known_fill_host(uint32_t *bits_inout, const int32_t dims[3], const int32_t *box, int value);
int isdf_known_frontier_host(const uint32_t *bits, const uint8_t *occ, const int32_t dims[3], uint32_t *bits_out, int64_t *vox_out, long long capacity,
                             isdf_map_frontier_info *info_out);

/* ---- the view gain: the unknown voxels a depth camera would see, per candidate pose ------------------------------- */
/* What a next-best-view loop maximises: for each of n_views candidate poses, the number of voxels that are unknown today (K = 0) and
 * that the camera would observe from there, given the map as it stands.  One launch over views x rays; one row per view comes back.
 * The definition is integers only from a ray's end point on, so isdf_view_gain_host and the device agree byte for byte.
 * poses: n_views x 12 doubles, each a cam2world as the depth camera takes it (rows (R | t), z the optical axis).  For view j:
 *   RAYS.  nu = ceil(width / stride_u), nv = ceil(height / stride_v); ray k = iv * nu + iu is pixel (u, v) = (iu stride_u, iv stride_v).
 *   Its end point and the row order are exactly what isdf_depth_rays_host gives for an image with no return at any pixel with
 *   no_return_is_free = 1, min_range_m = 0, these strides and max_range_m, and the ctx's map geometry.  In fp64, nothing contracted into
 *   an FMA: p = ((u - cx) * 1 / fx, (v - cy) * 1 / fy, 1); e = R p + t, each row summed left to right; d = e - t; range = sqrt(d_x^2 +
 *   d_y^2 + d_z^2); k = max_range_m / range; e_a = t_a + d_a * k, d_a = e_a - t_a.  The clip, with lo = bmin + resolution / 2, hi = bmax -
 *   resolution / 2: over the axes a with e_a < lo_a (bound = lo_a) or e_a > hi_a (bound = hi_a), s = the smallest of (bound - t_a) / d_a
 *   (0 where d_a = 0); if there is such an axis, s is held to [0, 1] and e_a = t_a + d_a * s.  Then e is rounded to float32 once.  The
 *   origin is t.  A ray whose e has a component that is not finite, or whose e (as doubles again) lies outside the map by the scan's test
 *   (a coordinate < bmin or > bmax), is SKIPPED (n_skipped).
 *   WALK.  Origin and end are quantised as the scan's rays are (isdf_integrate_scan above: q = floor((p - bmin) / resolution * 1024)
 *   clamped to dim * 1024 - 1) and walked as isdf_map_raycast walks them with test_origin_voxel = 0: voxel 0 is not tested; the walk ends
 *   at the first voxel after it whose occupancy byte is not 0, or at the end point's voxel.  V(ray) = every voxel of the walk from voxel 0
 *   up to and including the one where it ended.  Unknown voxels are transparent - the occupancy byte alone decides: the optimistic gain.
 *   GAIN.  S_j = the union of V(ray) over the rays that were not skipped: a set per view, not a sum per ray (the voxel at the camera,
 *   which every ray crosses, counts once).  gain_j = the number of v in S_j with K[v] = 0.
 * rows_out: n_views x 8 int64, {status, gain, n_rays, n_skipped, n_hits, steps_total, n_rays_unknown, 0}.  status 0: scored.  status 1:
 * the pose has an entry that is not finite, or its origin lies outside the map by the scan's test - every other word of the row is 0;
 * never an error of the call, candidates come from anywhere.  n_rays = nu nv; n_hits: walks ended by an occupied voxel; steps_total: the
 * sum of the walks' step counts as isdf_map_raycast_info counts them; n_rays_unknown: rays whose V holds at least one unknown voxel.
 * Every word is an integer sum or a set size: nothing depends on the order of the device's atomics.
 * The call is read-only: K, the occupancy, epochs, a kept field, an armed watch and a kept report are untouched.  The device keeps one
 * `seen` bit grid in K's layout per view of a chunk: views_per_chunk = scratch_bytes / (4 * words of K) held to [1, n_views]; the chunks
 * run in turn on the stream, the bytes of the rows do not depend on their size.  The scratch grows only: a second call of a size
 * allocates nothing.
 * Errors, all before anything is launched: ISDF_ERR_INVALID_ARG for a bad camera (the depth camera's rule), a stride < 1, a max_range_m
 * that is not finite or <= 0, scratch_bytes < 0, n_views < 0, a null poses or rows_out with n_views > 0; ISDF_ERR_UNSUPPORTED on a
 * multi-device ctx; ISDF_ERR_STATE without a known grid or without an occupancy grid.  n_views = 0 is legal; params and info_out may be
 * NULL.  isdf_view_gain_device: d_poses and d_rows_out are device memory, the work goes on `stream`; with info_out == NULL nothing is
 * handed over and nothing synchronised, with it `stream` is synchronised once - isdf_map_raycast_device's rule.
 * Not offered: a pessimistic gain in which unknown voxels block; a range- or angle-weighted gain; a gain kept incrementally across
 * scans.  Candidates: isdf_map_frontier_clusters below gives the frontier's clusters and a voxel of each to look at, isdf_view_candidates
 * the eyes round each, posed and scored. */
typedef struct isdf_view_gain_params {
    int32_t stride_u, stride_v;   /* default 4, 4; >= 1 */
    double  max_range_m;          /* required: finite, > 0 (default 5.0) */
    int64_t scratch_bytes;        /* default 64 MiB; >= 0; 0 = one view per chunk */
    int32_t reserved[4];
} isdf_view_gain_params;

typedef struct isdf_view_gain_info {
    int64_t n_views, n_scored, n_rays_per_view;
    int64_t best_view;            /* lowest index among the largest gains of status-0 rows; -1: none */
    int64_t best_gain;
    int64_t gain_total;
    int32_t chunks, reserved;
    double  gain_ms;              /* device time, events on the stream */
} isdf_view_gain_info;

void isdf_view_gain_params_default(isdf_view_gain_params *p);   /* null-safe */
void isdf_view_gain_sizes(int sizes_out[2]);                    /* null-safe */
int isdf_view_gain(isdf_ctx *ctx, const isdf_depth_camera *camera, const double *poses, long long n_views, const isdf_view_gain_params *params,
                   int64_t *rows_out, isdf_view_gain_info *info_out);
int isdf_view_gain_device(isdf_ctx *ctx, const isdf_depth_camera *camera, const double *d_poses, long long n_views, const isdf_view_gain_params *params,
                          int64_t *d_rows_out, isdf_view_gain_info *info_out, void *stream);
/* plain host code, no ctx, no device: bits = K's words, occ = nx ny nz occupancy bytes, the map's geometry as isdf_raycast_host takes it;
 * scratch_bytes is ignored.  Returns best_view, -1 when no view was scored, or a negative isdf_status (ISDF_ERR_INVALID_ARG: a null
 * array, a bad geometry, the bad arguments above; rows_out untouched).  info_out (nullable) is filled by a call that was not refused
 * (chunks 0, gain_ms 0) and left alone by one that was: that tells the two meanings of -1 apart. */
long long isdf_view_gain_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                              const isdf_depth_camera *camera, const double *poses, long long n_views, const isdf_view_gain_params *params, int64_t *rows_out,
                              isdf_view_gain_info *info_out);

/* ---- frontier clusters: connected components of the frontier, their centroids and goal voxels ---------------------- */
/* The frontier is tens of thousands of voxels; a goal is one of a handful.  isdf_map_frontier_clusters groups a voxel set into its
 * connected components on the device and returns one small row per component.  Everything but the three times is an integer, and
 * isdf_known_clusters_host gives the same bytes.
 *   INPUT SET.  bits_in == NULL: S = the frontier of the current K and occupancy, exactly isdf_map_frontier's.  bits_in != NULL: S = the
 *   caller's bit grid in K's layout (voxel a = (x * ny + y) * nz + z is bit a & 31 of word a >> 5, ceil(nx ny nz / 32) words); a bit set
 *   beyond the last voxel: ISDF_ERR_INVALID_ARG.  Any voxel set can be clustered so: the unknown voxels, an occupancy mask.
 *   NEIGHBOURS.  params.connectivity is 6, 18 or 26 (default 26; anything else ISDF_ERR_INVALID_ARG): voxels p and q are neighbours iff
 *   q - p lies in {-1, 0, 1}^3, is not 0 and has at most 1, 2 or 3 non-zero entries.  Both lie inside the grid: nothing wraps, and two
 *   voxels whose bits are adjacent in the stream (the last voxel of a column, the first of the next) are neighbours only by this rule.
 *   A frontier is a sheet one voxel thick, which 6-connectivity shreds; hence the default.
 *   CLUSTER.  A connected component of S under that relation.  Its label is its lowest voxel index; the clusters are numbered in
 *   ascending label order.  params.min_size (default 1; < 1 ISDF_ERR_INVALID_ARG) drops the clusters with fewer voxels from the rows; the
 *   survivors keep their order and are numbered 0 .. n_rows - 1.
 *   ROW.  16 int64 per kept cluster: {label, size, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, sum_x, sum_y, sum_z, rep_voxel, rep_d2, first_pos,
 *   0, 0}.  lo / hi: the inclusive index box of the members; sum_a: the sum of their indices on axis a; first_pos: the position of
 *   `label` in vox_out.  The centroid cell is c_a = sum_a / size (C integer division, every term >= 0), the centroid itself sum_a / size
 *   as a fraction.  rep_voxel is the member p that minimises d2 = |p - c|^2, ties to the lowest voxel index - the minimum over the members
 *   of the key (d2 << 36) | voxel (a voxel index is below 2^36 and d2 below 2^26 for dims <= 4096, so the key is below 2^62) -, and rep_d2
 *   its d2: a voxel of S itself (for the frontier: known and free), also where the centroid cell is not one (a ring).
 *   OUTPUTS.  vox_out (nullable, vox_capacity entries): the voxels of S ascending - for the frontier isdf_map_frontier's list.  labels_out
 *   (nullable, int32, vox_capacity entries): the row number of vox_out[i]'s cluster, -1 if min_size dropped it.  rows_out (nullable,
 *   row_capacity rows).  vox_capacity < n_voxels with vox_out or labels_out non-null, or row_capacity < n_rows with rows_out non-null:
 *   ISDF_ERR_OVERFLOW, info_out filled, every output untouched - a call with all three NULL is the sizing call.  Negative capacities:
 *   ISDF_ERR_INVALID_ARG.  info_out (nullable): n_voxels = |S|; n_clusters before the filter; n_rows after it; n_voxels_dropped = the
 *   voxels of the dropped clusters; largest_size and largest_label over ALL clusters, ties to the lowest label (0 and -1: S is empty);
 *   frontier_ms, label_ms, stats_ms: device time (events on the ctx's stream) of the set's kernel with the list's scan and emit pass,
 *   of the components (union and flatten), and of numbering, statistics, representatives and rows; 0 in the host form and for an empty S.
 * The errors are isdf_map_frontier's: no known grid ISDF_ERR_STATE (with bits_in too: the set has the grid's size and uses the known
 * grid's scratch); no occupancy grid while bits_in is NULL ISDF_ERR_STATE; a multi-device ctx ISDF_ERR_UNSUPPORTED; more than 2^31 words
 * or voxels of S ISDF_ERR_OVERFLOW.  The call is read-only: K, the occupancy, `merges`, epochs, a kept field, an armed watch and every
 * kept report are untouched.  Two hand-overs per call: the count of S, which sizes the scratch, and the results.  An empty S launches
 * nothing past the count and returns zero rows.  The scratch grows only: a second call of a size allocates nothing
 * (isdf_debug_live_bytes).  Two runs give the same bytes: the components' roots are their lowest positions whatever the order of the
 * device's atomics, and every statistic is an integer sum, minimum or maximum.
 * Not offered: a device-pointer form of the outputs; clusters kept incrementally across scans; splitting a large cluster (by its
 * principal axis, say); unknown space treated as an obstacle.  The eye positions of candidate views: isdf_view_candidates below. */
typedef struct isdf_frontier_cluster_params {
    int32_t connectivity;         /* 6, 18 or 26 (default 26) */
    int32_t reserved;
    int64_t min_size;             /* default 1; >= 1 */
} isdf_frontier_cluster_params;

typedef struct isdf_frontier_cluster_info {
    int64_t n_voxels, n_clusters, n_rows, n_voxels_dropped;
    int64_t largest_size, largest_label;
    double  frontier_ms, label_ms, stats_ms;
} isdf_frontier_cluster_info;

#define ISDF_FRONTIER_CLUSTER_ROW 16
void isdf_frontier_cluster_params_default(isdf_frontier_cluster_params *p);      /* null-safe */
void isdf_frontier_cluster_sizes(int sizes_out[2]);                              /* null-safe; sizeof of the params and of the info */
int isdf_map_frontier_clusters(isdf_ctx *ctx, const uint32_t *bits_in, const isdf_frontier_cluster_params *params, int64_t *vox_out, int32_t *labels_out,
                               long long vox_capacity, int64_t *rows_out, long long row_capacity, isdf_frontier_cluster_info *info_out);
/* plain host code, no ctx, no device: set_bits = S's words over dims = {nx, ny, nz}, each in [1, 4096]; outputs, ISDF_ERR_OVERFLOW and
 * ISDF_ERR_INVALID_ARG (a null set, bad dims, the bad arguments above) as isdf_map_frontier_clusters. */
int isdf_known_clusters_host(const uint32_t *set_bits, const int32_t dims[3], const isdf_frontier_cluster_params *params, int64_t *vox_out, int32_t *labels_out,
                             long long vox_capacity, int64_t *rows_out, long long row_capacity, isdf_frontier_cluster_info *info_out);

/* ---- candidate views: eyes round each target, tested, posed, scored and ranked -------------------------------------- */
/* The link between isdf_map_frontier_clusters (targets) and isdf_view_gain (scores): for each target a set of eye positions is tested on
 * the device for being a safe, seen place from which the target is visible, the survivors are posed looking at the target, the view
 * gain scores them without leaving the device and the best few per target come back.  Everything but the three times is an integer or
 * an fp64 value of a fixed order of IEEE operations, so isdf_view_candidates_host gives the device's bytes.
 *   INPUTS.  camera: the depth camera's rule.  targets: n_targets x 3 doubles, metres.  offsets: n_offsets x 3 doubles, metres.
 *   Candidate c = i * n_offsets + k has eye = target_i + offset_k, one fp64 addition per component.  The ABI does no trigonometry: the
 *   offsets are data (a ring is engine.view_ring_offsets' business), so no byte depends on a libm.
 *   STATUS of a candidate: the first test that fails, in this order.
 *     1 bad.  A component of the target or of the eye is not finite; or the scan's quantisation (isdf_integrate_scan above) refuses the
 *       target or the eye: a coordinate < bmin or > bmax; or, with d = target - eye, n2 = d_x^2 + d_y^2 + d_z^2 (summed left to right)
 *       is 0 or not finite.
 *     2 occupied.  The occupancy byte of the eye's voxel is not 0.
 *     3 unknown.  K is 0 at the eye's voxel.
 *     4 close.  Some voxel of the cube of Chebyshev radius clearance_voxels round the eye's voxel, clipped to the grid, is occupied or
 *       unknown: a safe eye stands in seen, free space.  Radius 0 adds nothing to tests 2 and 3.
 *     5 blocked.  The walk of isdf_map_raycast with test_origin_voxel = 0 from the eye's tick to the target's tick (both quantised as the
 *       scan's points are) ends at an occupied voxel that is not the target's own voxel.  A hit at the target's own voxel is visible: a
 *       target may be a surface voxel.
 *     0 kept.
 *   POSE of a kept candidate, fp64, nothing contracted into an FMA, sums left to right in the written order, sqrt and division the IEEE
 *   ones: n = sqrt(n2); z = d / n; x0 = (z_y, -z_x, 0), h = sqrt(x0_x^2 + x0_y^2); if h <= 1e-9: x0 = (0, z_z, -z_y), h = sqrt(x0_y^2 +
 *   x0_z^2); x = x0 / h; y = (z_y x_z - z_z x_y, z_z x_x - z_x x_z, z_x x_y - z_y x_x); the pose is rows (x_a, y_a, z_a, eye_a) - what
 *   engine.look_at(eye, target) with the default up gives, restated so that two implementations round alike.
 *   GAIN.  The isdf_view_gain row of that pose with params.gain, to the byte.
 *   SELECTION.  Per target, the kept candidates with gain >= min_gain, ordered by gain descending, ties to the lower k; the first k_best
 *   of them are the target's best.
 *   OUTPUTS, all nullable, host memory (the host-pointer form is the only device form).
 *     cand_out: n_candidates x 8 int64, {status, eye_voxel, los_steps, gain, n_hits, steps_total, n_rays_unknown, rank}.  eye_voxel =
 *       (x * ny + y) * nz + z, -1 for status 1; los_steps: the step count of test 5's walk, -1 where test 5 was not reached; words 3 - 6:
 *       the gain row's words 1, 4, 5 and 6, 0 unless the status is 0; rank: the place in the target's best list, -1: not in it.
 *     poses_out: n_candidates x 12 doubles, all zero unless the status is 0.
 *     target_out: n_targets x 8 int64, {n_kept, n_bad, n_occupied, n_unknown, n_close, n_blocked, best_candidate, best_gain}; the last two
 *       are -1 and 0 when no candidate qualified.
 *     best_out: n_targets x k_best int64 candidate indices, padded with -1.
 *     info_out: the counts over all candidates; n_scored, the candidates the gain scored (every kept one: a kept eye is finite and
 *       inside the map); the view gain's chunks (0: nothing kept); best_target, best_candidate and best_gain over all targets, ties to the
 *       lowest candidate index (-1, -1, 0: none qualified); filter_ms (tests, poses, compaction), gain_ms and select_ms: device time from
 *       events on the ctx's stream, 0 in the host form and where the stage did not run.
 *   ERRORS, all before anything is launched, in this order: the view gain's own argument errors for camera and params.gain;
 *   ISDF_ERR_INVALID_ARG for clearance_voxels outside [0, 8], k_best outside [1, 64], min_gain < 0, a negative n_targets or n_offsets,
 *   n_offsets > 2^20, n_targets * n_offsets > 2^31 - 1, a null targets or offsets with a positive count; ISDF_ERR_UNSUPPORTED on a
 *   multi-device ctx; ISDF_ERR_STATE without an occupancy grid, then without a known grid.  Zero targets or zero offsets is legal: nothing
 *   is launched and no output array is written (info_out is filled: zeros, the three best words -1, -1, 0).
 * The call is read-only: K, the occupancy, `merges`, epochs, a kept field, an armed watch and every kept report are untouched.  The
 * scratch (its own and the view gain's) grows only: a second call of a size allocates nothing (isdf_debug_live_bytes).  Two hand-overs
 * per call: the count of kept candidates, which sizes the gain's launches (the gain is never launched over a rejected candidate, each
 * view costs a cleared `seen` grid; with nothing kept nothing more is launched), and the results.  Two runs give the same bytes: the
 * counters are integer sums and the selection is a reduction without atomics.  min_gain is an integer, as every gain is.
 * Not offered: a device-pointer form; a yaw sweep at a fixed eye; ranking by travel cost (isdf_view_select_routed does that over the best
 * eyes); eyes tested against the robot's configuration space rather than a voxel cube; a pessimistic or weighted gain; candidates kept
 * across scans. */
typedef struct isdf_view_candidates_params {
    isdf_view_gain_params gain;   /* strides, max_range_m, scratch_bytes: isdf_view_gain's, with its defaults */
    int32_t clearance_voxels;     /* default 1; in [0, 8] */
    int32_t k_best;               /* default 3; in [1, 64] */
    int64_t min_gain;             /* default 1; >= 0 */
    int32_t reserved[4];
} isdf_view_candidates_params;

typedef struct isdf_view_candidates_info {
    int64_t n_targets, n_offsets, n_candidates;
    int64_t n_kept, n_bad, n_occupied, n_unknown, n_close, n_blocked;
    int64_t n_scored;
    int64_t best_target, best_candidate, best_gain;
    int32_t chunks, reserved;
    double  filter_ms, gain_ms, select_ms;
} isdf_view_candidates_info;

#define ISDF_VIEW_CANDIDATE_ROW 8
void isdf_view_candidates_params_default(isdf_view_candidates_params *p);       /* null-safe */
void isdf_view_candidates_sizes(int sizes_out[2]);                              /* null-safe; sizeof of the params and of the info */
int isdf_view_candidates(isdf_ctx *ctx, const isdf_depth_camera *camera, const double *targets, long long n_targets, const double *offsets, long long n_offsets,
                         const isdf_view_candidates_params *params, int64_t *cand_out, double *poses_out, int64_t *target_out, int64_t *best_out,
                         isdf_view_candidates_info *info_out);
/* plain host code, no ctx, no device: bits = K's words, occ = nx ny nz occupancy bytes, the map's geometry as isdf_raycast_host takes it;
 * gain.scratch_bytes is ignored.  ISDF_OK, or ISDF_ERR_INVALID_ARG (a null bits or occ, a bad geometry, the bad arguments above) with
 * nothing written. */
int isdf_view_candidates_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                              const isdf_depth_camera *camera, const double *targets, long long n_targets, const double *offsets, long long n_offsets,
                              const isdf_view_candidates_params *params, int64_t *cand_out, double *poses_out, int64_t *target_out, int64_t *best_out,
                              isdf_view_candidates_info *info_out);

/* ---- the view selection: k views of a pose list by their joint gain, greedy coverage -------------------------------- */
/* The gains of isdf_view_gain and isdf_view_candidates are each view's alone and do not add up: the best eyes of one target, and of
 * neighbouring clusters, look at the same pocket of unknown space.  isdf_view_select picks an ordered set of up to k_select views of a
 * pose list by the standard greedy coverage rule - the view that sees the most voxels which are unknown today and which no view picked
 * so far sees, then that view's voxels are claimed - with every round on the device, from sets the gain kernel has built; the rays are
 * walked once per view, not once per round.  Integers only, so isdf_view_select_host gives the device's bytes.
 *   SETS.  poses: n_views x 12 doubles, as isdf_view_gain takes them.  A view j whose isdf_view_gain row (with params.gain) has status
 *   0 is SCORED: S_j is that call's set and U_j = {v in S_j : K[v] = 0}, so |U_j| is the row's gain.  A view of status 1 has an empty U_j
 *   and is never picked.
 *   ROUNDS.  C_0 is empty.  In round r = 0 .. k_select - 1: m_j = |U_j \ C_r| for every scored view not picked so far; j* is the lowest
 *   index among the largest m_j - the largest key ((m_j + 1) << 24) | (2^24 - 1 - j); a marginal is below 2^36 and j below 2^24, so the
 *   key is below 2^61.  If no such view is left, or m_j* < min_gain, the selection ends with n_selected = r.  Otherwise round r picks j*
 *   and C_{r+1} = C_r | U_j*.  With min_gain = 0 a view whose marginal is 0 is picked like any other.
 *   OUTPUTS, all nullable, host memory.
 *     rows_out: n_views x 8 int64, the isdf_view_gain row of each pose, to the byte.
 *     select_out: k_select x 4 int64, per round {view, marginal, cumulative, overlap}: marginal = m_j*, cumulative = |C_{r+1}|, overlap =
 *       the view's own gain - marginal (what earlier picks had claimed of it).  Rounds that did not happen are {-1, 0, 0, 0}.
 *     round_out: n_views int64, the round in which the view was picked, or -1.
 *     claimed_out: ceil(nx ny nz / 32) words, K | C_final in K's layout: the known grid the map would have after those views, if nothing
 *       new turns out to be occupied.
 *     info_out: n_views; n_scored; n_selected; gain_selected = the last cumulative (0: none); gain_solo_sum = the sum of the picked
 *       views' own gains, so the double counting shows beside gain_selected; best_single_gain = the largest gain of a scored view;
 *       list_words = the non-zero words of all U_j (the device's list has one 8-byte entry for each); chunks = the view gain's;
 *       lists_ms = device time of building the lists (count, scan, fill), select_ms = of the rounds and of claimed_out's kernel, gain_ms
 *       = the bracket round the view gain's launches less lists_ms (it holds the chunks' hand-overs) - events on the ctx's stream, 0 in
 *       the host form and with n_views = 0.
 *   ERRORS, all before anything is launched, in this order: everything isdf_view_gain refuses for camera, params.gain, n_views and a
 *   null poses, in its order; ISDF_ERR_INVALID_ARG for k_select < 1 or min_gain < 0; ISDF_ERR_INVALID_ARG for n_views > 2^24 (the key's
 *   room); ISDF_ERR_UNSUPPORTED on a multi-device ctx; ISDF_ERR_STATE without an occupancy grid, then without a known grid.  n_views = 0
 *   is legal: nothing is launched, select_out is padded, claimed_out = K and the info is filled.
 * The device keeps no dense set: after each chunk of the view gain, while its `seen` grids are live, every view's non-zero words are
 * compacted into a segment of {word index, bits} entries of one list; a round streams the segments against the claimed grid.  One
 * hand-over per chunk (its entry total, which sizes the list), none between the rounds - a `done` flag on the device makes the kernels of
 * the rounds after the last return at once; at most min(k_select, n_views) rounds are launched -, one at the end.  The call is
 * read-only: K, the occupancy, `merges`, epochs, a kept field, an armed watch and every kept report are untouched.  The scratch (its own
 * and the view gain's) grows only and the list keeps its content when it grows: a second call of a size allocates nothing
 * (isdf_debug_live_bytes).  Two runs give the same bytes: the order of a segment's entries depends on atomics and nothing reads it.
 * Not offered: a device-pointer form; a weighted objective other than isdf_view_select_routed's gain per travel cost (below); lazy-greedy
 * pruning of the marginals; sets kept across calls. */
typedef struct isdf_view_select_params {
    isdf_view_gain_params gain;   /* strides, max_range_m, scratch_bytes: isdf_view_gain's, with its defaults */
    int32_t k_select;             /* default 4; >= 1 */
    int32_t reserved0;
    int64_t min_gain;             /* default 1; >= 0 */
    int32_t reserved[4];
} isdf_view_select_params;

typedef struct isdf_view_select_info {
    int64_t n_views, n_scored, n_selected;
    int64_t gain_selected, gain_solo_sum, best_single_gain;
    int64_t list_words;
    int32_t chunks, reserved;
    double  gain_ms, lists_ms, select_ms;
} isdf_view_select_info;

#define ISDF_VIEW_SELECT_ROW 4
void isdf_view_select_params_default(isdf_view_select_params *p);       /* null-safe */
void isdf_view_select_sizes(int sizes_out[2]);                          /* null-safe; sizeof of the params and of the info */
int isdf_view_select(isdf_ctx *ctx, const isdf_depth_camera *camera, const double *poses, long long n_views, const isdf_view_select_params *params,
                     int64_t *rows_out, int64_t *select_out, int64_t *round_out, uint32_t *claimed_out, isdf_view_select_info *info_out);
/* plain host code, no ctx, no device: bits = K's words, occ = nx ny nz occupancy bytes, the map's geometry as isdf_raycast_host takes it;
 * gain.scratch_bytes is ignored.  ISDF_OK, or ISDF_ERR_INVALID_ARG (a null bits or occ, a bad geometry, the bad arguments above) with
 * nothing written. */
int isdf_view_select_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                          const isdf_depth_camera *camera, const double *poses, long long n_views, const isdf_view_select_params *params, int64_t *rows_out,
                          int64_t *select_out, int64_t *round_out, uint32_t *claimed_out, isdf_view_select_info *info_out);

/* ---- the routed view selection: greedy coverage by marginal gain per travel cost ----------------------------------- */
/* isdf_view_select does not know where the robot is: a view across the map with a few more unknown voxels beats one two metres away,
 * and a view whose eye the robot cannot reach is picked like any other (isdf_view_candidates tests an eye against the occupancy and a
 * voxel cube, not against the configuration space, so a gated field's d can be +inf at an eye that passed).  isdf_view_select_routed
 * is that selection by UTILITY = marginal gain per travel cost, the cost read on the device from the ctx's valid cost-to-go field at
 * each view's eye, and the ways to the picked views read off the same field in the same stream.  The caller builds the field TOWARDS THE
 * ROBOT'S CELL first (isdf_frontend_field_build or _build_known): the graph is symmetric, so d[eye] is the cost of going there.
 *   The sets U_j, the rows, the claimed grid and its layout, and the meaning of select_out and round_out are isdf_view_select's.
 *   COST.  c_j is a non-negative double or +inf, in the field's unit, CELLS.  With cost == NULL, c_j is the ctx's field at the cell of
 *   the eye (poses[12 j + 3], [12 j + 7], [12 j + 11]) - to the byte what isdf_frontend_field_value answers for that point, +inf for an
 *   eye outside the map.  With cost != NULL, c_j = cost[j], a host array of n_views doubles; no field is needed then.
 *   ELIGIBLE.  A view is eligible when it is scored (row status 0), not picked so far, c_j is finite and c_j <= max_cost.
 *   ROUND r.  m_j = |U_j \ C_r| for every eligible view.  Among the eligible views with m_j >= min_gain, u_j = (double)m_j / (cost0 +
 *   c_j): one IEEE addition, then one IEEE division, in fp64 (m_j < 2^36: the conversion is exact).  j* is the lowest index among the
 *   largest u_j.  If there is no such view the selection ends with n_selected = r; otherwise round r picks j* and C_{r+1} = C_r | U_j*.
 *   OUTPUTS, all nullable, host memory.
 *     rows_out, select_out (the same four int64 per round), round_out, claimed_out: as isdf_view_select gives them.
 *     cost_out: n_views doubles, c_j of every view, scored or not.
 *     util_out: k_select x 2 doubles, {c_j*, u_j*} per round; {0, 0} for a round that did not happen.
 *     with path_cap >= 1 (cost == NULL only), for the picked views in pick order: path_n_out k_select int32, path_xyz_out k_select x
 *       path_cap x 3 doubles, path_rp_out k_select x path_cap x 2 doubles - exactly what isdf_frontend_field_paths gives with the picked
 *       eyes as starts and cap = path_cap.  The walk goes FROM THE EYE TO THE ROBOT'S CELL (the field's goal), and the attitudes are those
 *       of walking that way; a caller that drives robot -> eye reverses the rows.  Rounds that did not happen: n = 0 and zeros.
 *     info_out: select = isdf_view_select_info's words; n_eligible = the eligible views at round 0; n_unreachable = the scored views
 *       whose c is not finite; n_over_budget = the scored views with a finite c > max_cost; cost_selected = the sum of the picked c_j in
 *       pick order; cost_source = 0 (field) or 1 (array); cost_ms, paths_ms = device time of the cost kernel and of the path launches
 *       (events on the ctx's stream; 0 in the host form and where the stage did not run).
 *   ERRORS, all before anything is launched, in this order: everything isdf_view_select refuses, in its order; ISDF_ERR_INVALID_ARG for
 *   min_gain < 1 (with a utility 0 is "none", and a view that adds nothing is not worth a trip), cost0 <= 0 or not finite, a NaN or
 *   negative max_cost, path_cap < 0, path_cap >= 1 together with a cost array, a cost array holding a NaN or a negative value; with
 *   cost == NULL what the field's getters answer: ISDF_ERR_STATE without a front end or without a valid field (a dropped field is no
 *   field).  n_views = 0 is legal: nothing is launched, the outputs are padded, claimed_out = K.
 * On the device: one lane per view reads c_j through the field's own cell rule; the marginal kernel skips ineligible views; the pick is
 * two integer reductions without atomics (the bit pattern of u, which orders as u does for u >= 0, then the lowest index among the
 * equals); the picked eyes are gathered on the device as starts for the path kernel, which follows the rounds with no hand-over and
 * rides the final copy.  The call is read-only, as the selection is: the field, K, the epochs, a kept report and an armed watch are
 * untouched; a gated and an ungated field are both accepted.  The scratch grows only: a second call of a size allocates nothing
 * (isdf_debug_live_bytes).  isdf_view_select itself launches what it always launched.
 * isdf_view_select_routed_host: plain host code, the same bytes; cost is required (isdf_frontend_field_host gives a field to read it
 * from), there are no paths, cost_source = 1.
 * Not offered: a tour whose cost is counted from the previous pick (it needs a field per round); other utilities (linear, exponential);
 * a device-pointer form. */
typedef struct isdf_view_select_routed_params {
    isdf_view_select_params select;   /* isdf_view_select's, with its defaults; min_gain >= 1 here */
    double  cost0;                    /* default 1.0; finite, > 0: the cost of standing still, in cells */
    double  max_cost;                 /* default +inf: no budget; >= 0 */
    int32_t path_cap;                 /* default 0: no paths; else the rows per path */
    int32_t reserved[5];
} isdf_view_select_routed_params;

typedef struct isdf_view_select_routed_info {
    isdf_view_select_info select;
    int64_t n_eligible, n_unreachable, n_over_budget;
    double  cost_selected;
    int32_t cost_source, reserved;
    double  cost_ms, paths_ms;
} isdf_view_select_routed_info;

void isdf_view_select_routed_params_default(isdf_view_select_routed_params *p);     /* null-safe */
void isdf_view_select_routed_sizes(int sizes_out[2]);                               /* null-safe; sizeof of the params and of the info */
int isdf_view_select_routed(isdf_ctx *ctx, const isdf_depth_camera *camera, const double *poses, long long n_views, const double *cost,
                            const isdf_view_select_routed_params *params, int64_t *rows_out, int64_t *select_out, int64_t *round_out, uint32_t *claimed_out,
                            double *cost_out, double *util_out, int32_t *path_n_out, double *path_xyz_out, double *path_rp_out,
                            isdf_view_select_routed_info *info_out);
/* ISDF_OK, or ISDF_ERR_INVALID_ARG (a null bits, occ or cost, a bad geometry, the bad arguments above) with nothing written. */
int isdf_view_select_routed_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                                 const isdf_depth_camera *camera, const double *poses, long long n_views, const double *cost,
                                 const isdf_view_select_routed_params *params, int64_t *rows_out, int64_t *select_out, int64_t *round_out, uint32_t *claimed_out,
                                 double *cost_out, double *util_out, isdf_view_select_routed_info *info_out);

/* ---- planning through observed space only: the eroded known grid and the field gated by it ------------------------ */
/* The configuration-space table knows "occupied" and "not occupied": a voxel behind a wall no sensor has looked behind is free to it,
 * and isdf_frontend_field_build plans through it.  The eroded known grid says, for every voxel, whether the whole cube of voxels a robot
 * centred there can touch has been observed; the gated build closes every voxel for which it has not.  Integers only.
 *   DEFINITION.  K is the known grid above: voxel a = (x * ny + y) * nz + z is bit a & 31 of word a >> 5, ceil(nx ny nz / 32) words, the
 *   tail bits 0.  For a radius r >= 0 and border in {0, 1}
 *     E[v] = 1  iff  for every u with max(|ux - vx|, |uy - vy|, |uz - vz|) <= r:
 *                    (u inside the grid and K[u] = 1)  or  (u outside the grid and border = 1)
 *   in K's layout, tail bits 0.  r = 0: E = K.  border = 0: the grid's outside counts as unseen - right for a window that follows the
 *   robot; border = 1: it counts as seen - right for a fixed world box.  A radius of the largest dimension or more gives, with border = 0,
 *   all 0, and with border = 1 all 1 when K is all 1 and all 0 otherwise.
 *   radius = -1 (the default) means (kernel_size - 1) / 2 of the last isdf_frontend_build, the footprint the configuration-space pass
 *   reads; ISDF_ERR_STATE without a front end.  Otherwise 0 <= radius <= 64.
 * isdf_map_known_erode: E of the ctx's K on the device - three one-axis passes over the bit stream, 2 r + 1 reads per dword and pass, not
 * (2 r + 1)^3 per voxel.  bits_out (nullable): E's words; info_out (nullable): radius_used, border, known_voxels = |K|, eroded_voxels = |E|,
 * erode_ms = device time of the passes.  ERRORS, all before anything is launched, in this order: a null ctx (ISDF_ERR_INVALID_ARG); a
 * border other than 0 or 1, then a radius outside -1 .. 64 (ISDF_ERR_INVALID_ARG); a multi-device ctx (ISDF_ERR_UNSUPPORTED); no known
 * grid (ISDF_ERR_STATE); radius -1 without a front end (ISDF_ERR_STATE).  The call is read-only: K, the occupancy, a kept field, an armed
 * watch, every kept report and the epochs are untouched; its scratch (two bit grids) grows only, so a second call of a size allocates
 * nothing (isdf_debug_live_bytes), and two calls give the same bytes.
 * isdf_known_erode_host: plain host code, no ctx, no device, the same bytes.  bits_out must not be bits.  ISDF_ERR_INVALID_ARG, with
 * nothing written, in this order: null or aliased grids; bad dims (each 1 .. 4096); a border other than 0 or 1; a radius outside 0 .. 64.
 *   THE GATED FIELD.  isdf_frontend_field_build_known is isdf_frontend_field_build over
 *     free'[v] = (any attitude bit of table[v]) && E[v],
 *   E eroded in the same call from the K of that moment: d is the least fixed point above over free', its bytes those of
 *   isdf_frontend_field_host on table'[v] = E[v] ? table[v] : 0.  A goal cell with E = 0 gives reachable = 0 and status = 1, as an
 *   occupied goal does.  info_out->free_voxels counts free'; gate_out (nullable) is the erosion's info.  Afterwards
 *   isdf_frontend_field_get / _value / _paths[_device] work on the gated field as on any other: a path steps on voxels with E = 1 only,
 *   its start cell excepted, which need not be free.  ERRORS, all before anything is launched, in this order: a null ctx; a null goal or
 *   info; a negative max_rounds; a border other than 0 or 1, then a radius outside -1 .. 64 (all ISDF_ERR_INVALID_ARG); a multi-device ctx
 *   (ISDF_ERR_UNSUPPORTED); no front end (ISDF_ERR_STATE); no known grid (ISDF_ERR_STATE); more than 2^31 - 16 voxels
 *   (ISDF_ERR_UNSUPPORTED).  isdf_frontend_field_build itself launches what it always launched.
 *   isdf_frontend_field_known_info: out = {gated, radius_used, border, 0} of the live field; zeros for an ungated field or none.
 *   THE ROBOT'S OWN CELL is usually unseen - no ray starts inside the robot -, so E is 0 round it and no gated path could leave it.  A
 *   caller declares a box round the robot known first (isdf_map_known_fill), as it does for the frontier; the paths never need a free
 *   start cell.
 *   DROPPED, NOT CARRIED.  A gated field describes the K of its build.  Everything that can change K or the map drops it - field_valid
 *   goes false and the getters answer "isdf_frontend_field_build has not been called" -: isdf_update_pointcloud / _voxels,
 *   isdf_clear_pointcloud / _voxels, isdf_integrate_scan / _depth (also when no occupancy changed), isdf_shift_map, isdf_map_follow (also
 *   when it does not move), once the call's own state checks have passed; isdf_map_known_fill, isdf_map_known_enable and
 *   isdf_frontend_build.  The repair, reopen and shift modes do not apply to it: nothing of them runs and their _info calls report none.
 *   An ungated field behaves in all of these exactly as before.  This is mode 0 of isdf_frontend_field_set_known_follow, the default;
 *   with mode 1 a gated field follows updates, clears, scans and fills in place (below).
 * Not offered: the A* (isdf_frontend_astar_search) over the gated table; a gate for isdf_traj_check (isdf_traj_known_horizon reports the
 * first unknown voxel a trajectory comes near); a gated field carried through a shift of the map window. */
typedef struct isdf_known_erode_params {
    int32_t radius;               /* default -1: the front end's (kernel_size - 1) / 2; else 0 .. 64 */
    int32_t border;               /* default 0: the outside counts as unseen; 1: as seen */
} isdf_known_erode_params;

typedef struct isdf_known_erode_info {
    int32_t radius_used, border;
    int64_t known_voxels, eroded_voxels;
    double  erode_ms;
} isdf_known_erode_info;

void isdf_known_erode_params_default(isdf_known_erode_params *p);       /* null-safe */
void isdf_known_erode_sizes(int sizes_out[2]);                          /* null-safe; sizeof of the params and of the info */
int isdf_map_known_erode(isdf_ctx *ctx, const isdf_known_erode_params *params, uint32_t *bits_out, isdf_known_erode_info *info_out);
int isdf_known_erode_host(const uint32_t *bits, const int32_t dims[3], int radius, int border, uint32_t *bits_out);
int isdf_frontend_field_build_known(isdf_ctx *ctx, const double goal_xyz[3], const isdf_known_erode_params *erode, const isdf_frontend_field_params *params,
                                    isdf_frontend_field_info *info_out, isdf_known_erode_info *gate_out);
int isdf_frontend_field_known_info(isdf_ctx *ctx, int32_t out[4]);

/* ---- the gated field kept across scans, updates, clears and fills ------------------------------------------------- */
/* The gated field's free set is free'[v] = (any attitude bit of table[v]) && E[v].  Every in-place change moves it in ONE direction
 * per stage: an update closes table bits with K fixed (closing); a clear opens them with K fixed (opening); isdf_map_known_fill(box, 1)
 * grows K, so E grows (opening), and (box, 0) shrinks both (closing), with E changed only inside the box grown by the gate's radius; a
 * scan ORs bits into K and opens table bits (one opening stage), then closes table bits with E fixed (one closing stage).  Each stage
 * is the mark / seed / relax of isdf_frontend_field_set_repair / _set_reopen with the mark taken against ballot(table) & E_new, E_new
 * eroded from the K of that moment at the radius and border of the build; the result has the bytes of isdf_frontend_field_build_known
 * on the new map and K, by the proofs of those two rules.
 * isdf_frontend_field_set_known_follow: mode 0 (default) - a gated field is dropped as described under DROPPED, NOT CARRIED above, to
 * every byte and status code; mode 1 - a gated field that is valid, has status 0 or 1 and whose table is on the device FOLLOWS
 *   isdf_update_pointcloud / _voxels   the closing stage over the dirty box grown by the footprint;
 *   isdf_clear_pointcloud / _voxels    the opening stage over it;
 *   isdf_integrate_scan / _depth       one opening stage after the clear's table refresh, over the union of the clear's grown box (if a
 *                                      voxel was cleared) and the rays' box grown by the gate's radius - also when nothing was cleared
 *                                      but a voxel became known -, then the update's closing stage.  No ray, or nothing newly known,
 *                                      cleared or occupied: the field is untouched, field_dropped = 0 and no stage is reported;
 *   isdf_map_known_fill                value 1: opening, value 0: closing, over the box grown by the gate's radius; no stage when no
 *                                      bit of K changed,
 * whatever the repair, reopen and shift modes say; an ungated field is governed by those three exactly as before.  field_dropped of
 * each call's info is 0 where the field followed.  STILL DROPPED in mode 1: by isdf_shift_map and isdf_map_follow, isdf_map_known_enable
 * and isdf_frontend_build; by a change with refresh_frontend = 0; a field of status 2; a stage that finds a bit moved against its
 * direction; and whenever a step fails after the map has moved.  The mode outlives isdf_frontend_build.  Other modes:
 * ISDF_ERR_INVALID_ARG; a multi-device ctx: ISDF_ERR_UNSUPPORTED.
 * isdf_frontend_field_follow_info: the last followed call's report - its stages added up, the state after the last of them;
 * ISDF_ERR_STATE when no call was followed since the last build, or the field has been dropped since.  isdf_frontend_field_repair_info / _reopen_info report the closing /
 * the opening stage that ran, as for an ungated field; isdf_frontend_field_known_info keeps answering (1, radius, border). */
typedef struct isdf_field_follow_info {
    int32_t opening, closing;                 /* stages of that direction that ran in the call                                       */
    int32_t radius_used, border;              /* the gate's, as at the build                                                          */
    int64_t known_voxels, eroded_voxels;      /* |K| and |E| after the change                                                         */
    int64_t opened_voxels, closed_voxels;     /* bits of free' that rose / fell                                                       */
    int64_t free_voxels, reached_voxels;      /* |free'| and the voxels with a finite d after the change                              */
    int32_t reachable, status;                /* as isdf_frontend_field_info                                                          */
    double erode_ms, device_ms;               /* device time of the erosions / of the stages (mark to counts), summed                 */
} isdf_field_follow_info;
int isdf_frontend_field_set_known_follow(isdf_ctx *ctx, int mode);
int isdf_frontend_field_follow_info(isdf_ctx *ctx, isdf_field_follow_info *out);
void isdf_frontend_field_follow_sizes(int sizes_out[1]);      /* sizeof of the struct above, for mirrors of this header              */

/* ---- the reference's own input files (host side; no device needed) ---------------------------------------------------- */
/* ASCII .pcd global map as pcl::io::loadPCDFile<pcl::PointXYZ> reads it (src/map_manager/src/globalmap_gene.cpp:433-460;
 * the shipped src/plan_manager/map_pcds are "FIELDS x y z / DATA ascii"): xyz_out = up to `capacity` points x 3 floats (may be
 * NULL to count).  Returns the number of points in the file, or a negative isdf_status (ISDF_ERR_UNSUPPORTED: binary data).
 * The points go to isdf_set_pointcloud (= PCSmapManager::rcvGlobalMapHandler, PCSmap_manager.cpp:87-200). */
long long isdf_read_pcd(const char *path, float *xyz_out, long long capacity);
/* Wavefront .obj as igl::read_triangle_mesh reads it (src/utils/src/Shape.cpp:36): vertices V_out (capV x 3), triangles F_out
 * (capF x 3, zero based; polygons fanned from their first vertex).  nV_out / nF_out always receive the counts in the file. */
int isdf_read_obj(const char *path, double *V_out, int capV, int32_t *F_out, int capF, int *nV_out, int *nF_out);
/* Writes V (nV x 3) and F (nF x 3, zero based) as a Wavefront .obj ("v x y z" with 17 significant digits, "f a b c" one based):
 * isdf_read_obj reads the same doubles and indices back. */
int isdf_write_obj(const char *path, const double *V, int nV, const int32_t *F, int nF);
/* yaml poly_params [x, y, z, roll, pitch, yaw (degrees)] -> Rotate = yaw * pitch * roll with Eigen's AngleAxis matrices and
 * PI = 3.14159265358979323846 (Shape.cpp:23,38-43), row-major. */
int isdf_poly_rotation(const double poly_params[6], double rotate_out[9]);
/* Generalshape's constructor transform (Shape.cpp:37-49): V <- (V.homogeneous() * Trans^T).hnormalized() in place, with
 * Trans = [Rotate | trans]; trans_out / rotate_out (nullable) receive what isdf_shape.trans / .rotate take. */
int isdf_body_transform(const double poly_params[6], double *V_inout, int nV, double trans_out[3], double rotate_out[9]);
/* What a plan needs from the yaml files of src/plan_manager/config (rosparam -> Config::loadParameters,
 * src/utils/include/utils/config.hpp:13-203).  Fields a file leaves out keep Config's in-class defaults. */
typedef struct isdf_plan_config {
    isdf_config sweep;             /* the hot path's fields; variant = ISDF_V1_SWEPT (the live configuration)                  */
    isdf_frontend_config frontend; /* kernel_size, kernel_max_roll / _pitch, kernel_ang_res, front_end_safeh                   */
    double occupancy_resolution;   /* voxel edge of the occupancy grid                                                        */
    int32_t sta_threshold;         /* points per voxel for "occupied" (PCSmap_manager.cpp:160)                                */
    int32_t threads_num;           /* the reference's OpenMP team (baseline only)                                             */
    double rho, inittime, momentum;
    double traj_parlength;         /* 3.0: waypoint spacing in metres (plan_manager.cpp:153,206-213)                          */
    double poly_params[6];         /* body offset of the robot: x y z roll pitch yaw(deg)                                     */
    double offset_aabb[3];         /* offsetAABBbox                                                                           */
    double box[3];                 /* box_x / box_y / box_z                                                                   */
    double map_bound[6];           /* mapBound                                                                                */
    char inputdata[256];           /* e.g. "shapes/RoundedCone.obj" (relative to the plan_manager package)                    */
    char pcdmapname[128];
} isdf_plan_config;
void isdf_plan_config_default(isdf_plan_config *out);
int isdf_load_yaml_config(const char *yaml_path, isdf_plan_config *out);
/* SweptVolumeManager::initShape (sw_manager.hpp:239-275): the stem of inputdata is looked up in the analytic registry
 * (isdf_shape_from_name; trans / rotate from poly_params); any other stem is the mesh Generalshape - the obj is read from
 * package_dir/inputdata into the caller's buffers and put through isdf_body_transform.  ISDF_ERR_OVERFLOW: buffers too small. */
int isdf_shape_from_config(isdf_shape *shape, const isdf_plan_config *cfg, const char *package_dir, double *V_buf, int capV,
                           int32_t *F_buf, int capF);

/* ---- instrumentation --------------------------------------------------------------------------------------- */
/* on = N > 0: every N-th isdf_eval_device attaches HIP start/stop events to the dispatch of its dominant kernel on
 * `stream` (hipExtLaunchKernel: the kernel's own begin/end timestamps, the interval rocprofv3 reports);
 * isdf_profile_read synchronises and returns the number of launches recorded since the last read and their
 * mean duration in milliseconds.  on = 0 disables.  on = N | ISDF_PROFILE_SECONDARY also times the kernel that follows
 * the dominant one (two more events per instrumented launch; each timed dispatch costs the stream a few microseconds). */
#define ISDF_PROFILE_SECONDARY 0x10000
int isdf_profile_enable(isdf_ctx *ctx, int on);
int isdf_profile_read(isdf_ctx *ctx, int *n_launches, double *mean_ms);
/* Mean duration (ms) of the kernel that follows the dominant one in the same launches (tail_kernel / the V1 reduce),
 * valid after isdf_profile_read when ISDF_PROFILE_SECONDARY was set (0 otherwise). */
int isdf_profile_read_secondary(isdf_ctx *ctx, double *mean_ms);
/* Counters of the last evaluation (for tests / roofline bookkeeping). */
typedef struct isdf_stats {
    int64_t n_units;          /* constraint-point evaluations (poses for V2/V3, obstacle points for V1)  */
    int64_t n_units_culled;   /* V3 poses skipped by the whole-tile cull                                  */
    int64_t n_pairs;          /* (pose, qualifying voxel) robot-SDF evaluations                           */
    int64_t n_grad_pairs;     /* pairs whose penalty was active (gradient evaluated)                      */
    int32_t overflow;         /* nonzero: a bounded list overflowed                                       */
    int32_t reserved;
} isdf_stats;
int isdf_get_stats(isdf_ctx *ctx, isdf_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* ISDF_ACCEL_H */
