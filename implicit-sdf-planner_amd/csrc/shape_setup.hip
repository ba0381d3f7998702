// Robot-shape setup of the C ABI: the analytic-shape registry, isdf_set_shape (mesh robots: hierarchy, device tables, form of the
// sweep, distance lattice), the sampled-lattice kind, the program kind (a composition from the CSG class's op library).
#include "isdf_ctx.hpp"
#include "mesh_tables.hpp"
#include "shape_program_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace isdf;

static void shape_identity(isdf_shape *s, int kind) {
    std::memset(s, 0, sizeof(*s));
    s->kind = kind;
    s->grad_mode = ISDF_GRAD_DEFAULT;
    s->rotate[0] = s->rotate[4] = s->rotate[8] = 1.0;
}
static void setp(isdf_shape *s, std::initializer_list<double> v) {
    int i = 0;
    for (double x : v) s->params[i++] = x;
}

extern "C" int isdf_shape_default(isdf_shape *s, int kind) {
    if (!s || kind < 0 || kind >= ISDF_SHAPE_KIND_COUNT) return ISDF_ERR_INVALID_ARG;
    shape_identity(s, kind);
    switch (kind) {
    case ISDF_SHAPE_TORUS: setp(s, {2.5, 0.3}); break;
    case ISDF_SHAPE_CAPPEDTORUS: setp(s, {std::sin(40), std::cos(40), 3.5, 0.3}); break;
    case ISDF_SHAPE_CAPPEDCONE: setp(s, {2.0, 0.8, 0, 0, -1, 0, 0, 1}); break;
    case ISDF_SHAPE_ROUNDEDCONE: setp(s, {1.5, 0.6, 4.5}); break;
    case ISDF_SHAPE_WIREFRAMEBOX: setp(s, {1.8, 2.5, 3.5, 0.1}); break;
    case ISDF_SHAPE_BENDLINEAR: setp(s, {2.0, 0.25}); break;
    case ISDF_SHAPE_TWISTBOX: setp(s, {2.0, 2.0, 2.0, 3.14159265358979323846 / 6}); break;
    case ISDF_SHAPE_BENDBOX: setp(s, {2.0, 2.0, 2.0, 0.5}); break;
    case ISDF_SHAPE_TABLE: setp(s, {0.0, 0.0, 0.0, 3.5, 1.75, 0.7, 2.8, 1.05, 0.0, 3.5, 1.75, 2.8}); break;
    case ISDF_SHAPE_TREFOIL: setp(s, {3.5, 0.2, 0.2, 0.05, 0.4}); break;
    case ISDF_SHAPE_SMOOTHDIFFERENCE: setp(s, {3.0, 3.0, 0.5, 1.0, 0.25}); break;
    case ISDF_SHAPE_SMOOTHINTERSECTION: setp(s, {3.0, 3.0, 0.5, 1.0, 0.25}); break;
    case ISDF_SHAPE_CSG: setp(s, {3.0, 4.5, 1.5}); break;
    case ISDF_SHAPE_BOX: setp(s, {3.0, 0.3, 0.3}); break;
    case ISDF_SHAPE_BALL: setp(s, {1.0}); break;
    default: break;
    }
    return ISDF_OK;
}

extern "C" int isdf_shape_from_name(isdf_shape *s, const char *stem) {
    if (!s || !stem) return ISDF_ERR_INVALID_ARG;
    struct Ent { const char *name; int kind; };
    static const Ent reg[] = {   // sw_manager.hpp:74-123
        {"CSG", ISDF_SHAPE_CSG}, {"Torus", ISDF_SHAPE_TORUS}, {"Torus_big", ISDF_SHAPE_TORUS},
        {"Cappedtorus", ISDF_SHAPE_CAPPEDTORUS}, {"Trefoil", ISDF_SHAPE_TREFOIL}, {"Table", ISDF_SHAPE_TABLE},
        {"CappedCone", ISDF_SHAPE_CAPPEDCONE}, {"RoundedCone", ISDF_SHAPE_ROUNDEDCONE},
        {"WireframeBox", ISDF_SHAPE_WIREFRAMEBOX}, {"BendLinear", ISDF_SHAPE_BENDLINEAR},
        {"BendLinear_big", ISDF_SHAPE_BENDLINEAR}, {"TwistBox", ISDF_SHAPE_TWISTBOX}, {"BendBox", ISDF_SHAPE_BENDBOX},
        {"SmoothDifference", ISDF_SHAPE_SMOOTHDIFFERENCE}, {"SmoothIntersection", ISDF_SHAPE_SMOOTHINTERSECTION},
        {"SmoothIntersection_big", ISDF_SHAPE_SMOOTHINTERSECTION}};
    for (const Ent &e : reg) {
        if (std::strcmp(e.name, stem) == 0) {
            isdf_shape_default(s, e.kind);
            if (!std::strcmp(stem, "Torus_big")) setp(s, {3.5, 0.3});
            if (!std::strcmp(stem, "BendLinear_big")) setp(s, {3.2, 0.45});
            if (!std::strcmp(stem, "SmoothIntersection_big")) setp(s, {9.0, 9.0, 1.5, 3.0, 0.25});
            return ISDF_OK;
        }
    }
    return ISDF_ERR_UNSUPPORTED;   // not analytic: the reference falls back to the mesh Generalshape (:263-274)
}

static void free_mesh(isdf_ctx *c) {
    for (DevBuf<float> *b : {&c->d_mesh_trif, &c->d_fwn_box, &c->d_fwn_boxq, &c->d_mesh_dl}) b->release();
    for (DevBuf<double> *b : {&c->d_mesh_tri, &c->d_fwn_triq}) b->release();
    c->d_mesh.release(); c->d_fwn_child.release(); c->d_mesh_flat.release();
}

// rotate()/rotate_to() of the CSG class (Shape.hpp:2016-2053), evaluated once on the host
static void csg_rotate_to(const double a_in[3], const double b_in[3], double R[9]) {
    auto nrm = [](const double v[3], double o[3]) {
        const double z = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        const double s = z > 0 ? std::sqrt(z) : 1.0;
        for (int i = 0; i < 3; i++) o[i] = z > 0 ? v[i] / s : v[i];
    };
    double a[3], b[3];
    nrm(a_in, a); nrm(b_in, b);
    const double d = b[0] * a[0] + b[1] * a[1] + b[2] * a[2];
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (std::fabs(d - 1) < 1.1920929e-07f) return;
    const double angle = std::acos(d);
    const double v[3] = {b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]};
    double n[3];
    nrm(v, n);
    const double x = n[0], y = n[1], z = n[2], s = std::sin(angle), co = std::cos(angle), m = 1 - co;
    R[0] = m * x * x + co;    R[1] = m * x * y + z * s; R[2] = m * z * x - y * s;
    R[3] = m * x * y - z * s; R[4] = m * y * y + co;    R[5] = m * y * z + x * s;
    R[6] = m * z * x + y * s; R[7] = m * y * z - x * s; R[8] = m * z * z + co;
}

// The device's form of an isdf_shape: the parameters in both precisions, the box the row pruning lets voxels come from (bb_c / bb_h:
// the caller's, or that of a mesh's vertices), the switches.  The mesh kind's tables follow in install_mesh.
static void fill_dev_shape(const isdf_shape *s, DevShape &d, double bb_c[3], double bb_h[3]) {
    d.kind = s->kind;
    d.grad_mode = s->grad_mode;
    if (d.grad_mode == ISDF_GRAD_DEFAULT)
        d.grad_mode = s->kind == ISDF_SHAPE_BOX ? ISDF_GRAD_BOX_FORWARD : (s->kind == ISDF_SHAPE_BALL ? ISDF_GRAD_ANALYTIC_BALL : ISDF_GRAD_CENTRAL);
    std::memcpy(d.d.p, s->params, sizeof(d.d.p));
    std::memcpy(d.d.trans, s->trans, sizeof(d.d.trans));
    std::memcpy(d.d.rot, s->rotate, sizeof(d.d.rot));
    d.bound_radius = s->bound_radius;
    const double X[3] = {1, 0, 0}, Y[3] = {0, 1, 0}, Z[3] = {0, 0, 1};
    csg_rotate_to(X, Y, d.d.csg_r2);
    csg_rotate_to(X, Z, d.d.csg_r3);
    for (int i = 0; i < 16; i++) d.f.p[i] = (float)d.d.p[i];
    for (int i = 0; i < 3; i++) d.f.trans[i] = (float)d.d.trans[i];
    {
        bool ident = d.d.trans[0] == 0.0 && d.d.trans[1] == 0.0 && d.d.trans[2] == 0.0;
        for (int i = 0; i < 9; i++) ident = ident && d.d.rot[i] == ((i % 4 == 0) ? 1.0 : 0.0);
        d.d.ident = d.f.ident = ident ? 1 : 0;
    }
    for (int i = 0; i < 9; i++) { d.f.rot[i] = (float)d.d.rot[i]; d.f.csg_r2[i] = (float)d.d.csg_r2[i]; d.f.csg_r3[i] = (float)d.d.csg_r3[i]; }
    for (int a = 0; a < 3; a++) { bb_c[a] = s->bbox_center[a]; bb_h[a] = s->bbox_half[a]; }
    if (s->kind == ISDF_SHAPE_MESH && s->mesh_vertices && s->n_vertices > 0 && !(bb_h[0] > 0 && bb_h[1] > 0 && bb_h[2] > 0)) {
        // a mesh lies inside the box of its vertices: use it for row pruning when the caller gave none
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int v = 0; v < s->n_vertices; v++)
            for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], s->mesh_vertices[3 * v + a]); hi[a] = std::max(hi[a], s->mesh_vertices[3 * v + a]); }
        for (int a = 0; a < 3; a++) { bb_c[a] = 0.5 * (lo[a] + hi[a]); bb_h[a] = 0.5 * (hi[a] - lo[a]) + 1e-6 * (std::fabs(lo[a]) + std::fabs(hi[a]) + 1.0); }
    }
    d.prune_rows = (bb_h[0] > 0 && bb_h[1] > 0 && bb_h[2] > 0) && !env_is("ISDF_NO_ROW_PRUNE", '1');
    for (int i = 0; i < 3; i++) { d.bbox_lo[i] = (float)(bb_c[i] - bb_h[i]); d.bbox_hi[i] = (float)(bb_c[i] + bb_h[i]); }
    // the fp32 pre-filter of tile_kernel needs a continuous analytic SDF; ISDF_NO_F32_FILTER=1 disables it (A/B runs)
    d.filter_f32 = (s->kind != ISDF_SHAPE_MESH) && !env_is("ISDF_NO_F32_FILTER", '1');
    d.mesh = nullptr;
    d.mesh_wg = 0;
    d.mesh_flat = 0; d.mesh_flat_words = 0; d.mesh_flat_slots = 0;
    d.mesh_levels = isdf::MESH_Q_LEVELS;
}

// A mesh robot on the host: its faces' coordinates, the winding-number hierarchy and the device tables built from it
// (csrc/mesh_tables.hpp)
struct MeshHost {
    std::vector<double> tri;            // nine coordinates per face ...
    std::vector<float> trif;            // ... and their float copies
    isdf_host::FwnTree tree;
    int depth = 0;
    std::vector<float> boxq;            // child-major records
    std::vector<double> triq;
    std::vector<int> flat;              // small meshes: the WHOLE hierarchy as one table; empty: it does not qualify
};
static int mesh_host_build(isdf_ctx *c, const isdf_shape *s, MeshHost &m) {
    if (!s->mesh_vertices || !s->mesh_faces || s->n_faces < 1 || s->n_vertices < 3) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "mesh shape needs vertices and faces");
    m.tri.resize((size_t)9 * s->n_faces);
    m.trif.resize((size_t)9 * s->n_faces);
    for (int f = 0; f < s->n_faces; f++)
        for (int k = 0; k < 3; k++) {
            const int vi = s->mesh_faces[3 * f + k];
            if (vi < 0 || vi >= s->n_vertices) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "mesh face index out of range");
            for (int a = 0; a < 3; a++) {
                m.tri[(size_t)9 * f + 3 * k + a] = s->mesh_vertices[3 * vi + a];
                m.trif[(size_t)9 * f + 3 * k + a] = (float)s->mesh_vertices[3 * vi + a];
            }
        }
    // the reference's winding-number hierarchy (igl::fast_winding_number(V, F, 2, fwn_bvh), Shape.cpp:86)
    isdf_host::fwn_build(s->mesh_vertices, s->n_vertices, s->mesh_faces, s->n_faces, m.tree);
    m.depth = isdf_host::fwn_depth(m.tree);
    if (3 * m.depth + 1 > isdf::MESH_STACK) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "mesh hierarchy too deep for the device traversal stack");
    isdf_host::mesh_child_records(m.tree, m.tri, m.trif, isdf::MESH_Q_REC, isdf::MESH_Q_TRI, m.boxq, m.triq);
    m.flat = isdf_host::mesh_flat_blob(m.tree, m.boxq, m.triq, 0, isdf::MESH_FLAT_SLOTS, isdf::MESH_FLAT_LEVELS, isdf::MESH_Q_REC, isdf::MESH_Q_TRI);
    return ISDF_OK;
}

// the mesh's tables into device memory; hm: the DevMesh that names them (not uploaded yet: the caller still decides the form)
static int mesh_upload(isdf_ctx *c, const MeshHost &m, int n_faces, DevMesh &hm) {
    const isdf_host::FwnTree &tree = m.tree;
    free_mesh(c);
    HIPCHK(c, c->d_fwn_child.alloc(tree.child.size()));
    HIPCHK(c, c->d_fwn_box.alloc(tree.box.size()));
    HIPCHK(c, hipMemcpy(c->d_fwn_child, tree.child.data(), tree.child.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_fwn_box, tree.box.data(), tree.box.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, c->d_mesh_tri.alloc(m.tri.size()));
    HIPCHK(c, c->d_mesh_trif.alloc(m.trif.size()));
    HIPCHK(c, c->d_mesh.alloc(1));
    HIPCHK(c, hipMemcpy(c->d_mesh_tri, m.tri.data(), m.tri.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_mesh_trif, m.trif.data(), m.trif.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, c->d_fwn_boxq.alloc(m.boxq.size()));
    HIPCHK(c, hipMemcpy(c->d_fwn_boxq, m.boxq.data(), m.boxq.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, c->d_fwn_triq.alloc(m.triq.size()));
    HIPCHK(c, hipMemcpy(c->d_fwn_triq, m.triq.data(), m.triq.size() * sizeof(double), hipMemcpyHostToDevice));
    hm = DevMesh{c->d_mesh_tri, c->d_mesh_trif, n_faces, c->d_fwn_child, c->d_fwn_box, tree.n_nodes(), c->d_fwn_boxq, c->d_fwn_triq, m.depth, nullptr, {0, 0, 0}, {0.f, 0.f, 0.f}, 0.f, 0.f, 0.f, 0.f,
                 nullptr, 0, 0, 0, 0, 0, 0};
    const std::vector<int> &flat = m.flat;
    if (!flat.empty()) {
        HIPCHK(c, c->d_mesh_flat.alloc(flat.size()));
        HIPCHK(c, hipMemcpy(c->d_mesh_flat, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
        hm.flat_words = (int)flat.size(); hm.flat_rec = flat[22]; hm.flat_trec = flat[23];
        hm.flat = c->d_mesh_flat; hm.flat_slots = flat[19]; hm.flat_nodes = tree.n_nodes(); hm.flat_levels = flat[20];
    }
    return ISDF_OK;
}

// The tile sweep's pre-filter for the mesh kind: a lattice of distances over the box the row pruning lets voxels come from (the
// shape's box inflated by the penalty band), 96 cells along its longest side.  A voxel whose nearest node is farther from the
// surface than the widened band + the node spacing, on the outside, cannot carry a penalty (DevMesh::dl) - most of the listed
// voxels of a mesh robot, each of which would cost a hierarchy query.  ISDF_NO_F32_FILTER=1 leaves it out.
// (closed meshes only: next to an OPEN surface the winding number is a fraction, and (1 - 2 w) * distance says nothing
// about the distance)
struct MeshLattice { bool want = false; int solid = 0; float s_range[2] = {0.f, 0.f}, defect[2] = {0.f, 0.f}; };
static int mesh_lattice(isdf_ctx *c, int n_faces, const double bb_h[3], DevShape &d, DevMesh &hm, MeshLattice &lat) {
    // ... and the surface must bound a solid: exact winding number 0 / 1 on the two sides of every face (shape_eval.hip:
    // nested sheets, overlapping or inverted components and tears show up there whatever their thickness)
    lat.want = d.prune_rows && !env_is("ISDF_NO_F32_FILTER", '1');
    double llo[3] = {0, 0, 0}, lhi[3] = {0, 0, 0}, lat_ext = 0.0;
    int cells = 96;
    if (lat.want) {
        // (the lattice's box: wide enough for the swept-volume scans' band, 2 safety_hor + 0.1, as well: mesh_lattice_not_below)
        const double margin = 1.05 * std::max(c->cfg.safety_hor, 2.0 * c->cfg.safety_hor + 0.1) + 0.01;
        for (int a = 0; a < 3; a++) { llo[a] = (double)d.bbox_lo[a] - margin; lhi[a] = (double)d.bbox_hi[a] + margin; lat_ext = std::max(lat_ext, lhi[a] - llo[a]); }
        if (const char *e = getenv("ISDF_MESH_LATTICE_CELLS")) { const int v = atoi(e); if (v >= 16 && v <= 256) cells = v; }      // (developer switch)
        double ext3 = 0.0;
        for (int a = 0; a < 3; a++) ext3 = std::max(ext3, 2.0 * bb_h[a]);
        // a defect pocket may be a tenth of the lattice's reach (half a cell diagonal) thick; anything thicker is a region
        const double tau_limit = 0.1 * 0.5 * 1.7320508 * (lat_ext / cells);
        const int rcv = isdf_mesh_surface_valid(c, c->d_mesh_tri, n_faces, ext3, tau_limit, &lat.solid, lat.defect);
        if (rcv) return rcv;
    }
    if (lat.want && lat.solid) {
        ISDF_TRY(isdf_mesh_lattice_build(c, &hm, llo, lhi, cells, lat.s_range));
        if (hm.dl) {
            hm.dl_tau = lat.defect[0]; hm.dl_slack = 1.05f * lat.defect[1] * lat.defect[0];
            HIPCHK(c, hipMemcpy(c->d_mesh, &hm, sizeof(hm), hipMemcpyHostToDevice)); d.filter_f32 = 1;
        }
    }
    return ISDF_OK;
}

// the mesh kind: hierarchy and tables, upload, the form of the sweeps, the distance lattice, isdf_mesh_info
static int install_mesh(isdf_ctx *c, const isdf_shape *s, DevShape &d, const double bb_h[3]) {
    MeshHost m;
    ISDF_TRY(mesh_host_build(c, s, m));
    DevMesh hm;
    ISDF_TRY(mesh_upload(c, m, s->n_faces, hm));
    const int depth = m.depth;
    // Which form the swept-volume sweep takes: the FLAT evaluation for small meshes (<= 64 slots: the reference's 12- to 20-face
    // robots), else one task per workgroup with the quad-cooperative walks (round 6, C5 shape: drone.obj, 52 faces, 1.50 ms against
    // 1.69 with the wave-cooperative walks, kuang.obj, 60 faces, 1.96 / 2.26, box.obj, 96 faces, 3.6 / 4.7); the wave-cooperative
    // walks keep the hierarchies deeper than MESH_Q_LEVELS.  ISDF_MESH_WG=0/1, ISDF_MESH_FLAT=0 force.
    d.mesh_levels = std::max(2, std::min(depth, isdf::MESH_Q_LEVELS));
    c->mesh_depth = depth;
    d.mesh_wg = depth <= isdf::MESH_Q_LEVELS ? 1 : 0;
    if (const char *e = getenv("ISDF_MESH_WG")) d.mesh_wg = (e[0] == '1' && depth <= isdf::MESH_Q_LEVELS) ? 1 : 0;
    // small meshes: the flat evaluation (one task per workgroup as well); ISDF_MESH_FLAT=0 keeps the walks (A/B runs, tests)
    d.mesh_flat = hm.flat ? 1 : 0;
    d.mesh_flat_words = hm.flat_words; d.mesh_flat_slots = hm.flat_slots;
    if (env_is("ISDF_MESH_FLAT", '0')) d.mesh_flat = 0;
    HIPCHK(c, hipMemcpy(c->d_mesh, &hm, sizeof(hm), hipMemcpyHostToDevice));
    d.mesh = c->d_mesh;
    // (the edge pairing goes by vertex INDEX: a triangle soup - the reference's Lthick.obj, box.obj, kuang.obj, drone.obj keep
    // three vertices of their own per face - is "open" to it whatever its geometry.  The exact test of mesh_lattice is geometric and catches
    // open surfaces too (next to a boundary the winding number is a fraction), so it alone decides; `closed` is reported.)
    const bool closed = isdf_host::mesh_closed_by_index(s->mesh_faces, s->n_faces, s->n_vertices);
    MeshLattice lat;
    ISDF_TRY(mesh_lattice(c, s->n_faces, bb_h, d, hm, lat));
    {   // isdf_mesh_info
        int *mi = c->mesh_info;
        mi[0] = s->n_faces; mi[1] = m.tree.n_nodes(); mi[2] = depth; mi[3] = d.mesh_wg; mi[4] = closed ? 1 : 0; mi[5] = lat.want ? lat.solid : -1;
        mi[6] = hm.dl ? hm.dln[0] : 0; mi[7] = hm.dl ? hm.dln[1] : 0; mi[8] = hm.dl ? hm.dln[2] : 0;
        mi[9] = (int)std::lround(1.0e6 * lat.s_range[0]); mi[10] = (int)std::lround(1.0e6 * lat.s_range[1]); mi[11] = d.mesh_flat ? hm.flat_slots : 0;
        mi[12] = (int)std::lround(1.0e9 * lat.defect[0]); mi[13] = (int)std::lround(1.0e3 * lat.defect[1]); mi[14] = mi[15] = 0;
    }
    return ISDF_OK;
}

extern "C" int isdf_set_shape(isdf_ctx *c, const isdf_shape *s) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!s || s->kind < 0 || s->kind >= ISDF_SHAPE_KIND_COUNT) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad shape kind");
    if (s->grad_mode < ISDF_GRAD_DEFAULT || s->grad_mode > ISDF_GRAD_ANALYTIC_BALL) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad grad_mode");
    if (s->kind == ISDF_SHAPE_GRID) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "ISDF_SHAPE_GRID is installed with isdf_set_shape_grid / isdf_set_shape_sampled");
    if (s->kind == ISDF_SHAPE_PROGRAM) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "ISDF_SHAPE_PROGRAM is installed with isdf_set_shape_program");
    HIPCHK(c, hipSetDevice(c->device));
    DevShape d{};
    double bb_c[3], bb_h[3];
    fill_dev_shape(s, d, bb_c, bb_h);
    if (s->kind == ISDF_SHAPE_MESH) ISDF_TRY(install_mesh(c, s, d, bb_h));
    if (s->kind != ISDF_SHAPE_MESH) std::memset(c->mesh_info, 0, sizeof(c->mesh_info));
    isdf_frontend_release(c);       // the attitude kernels were voxelised from the previous shape
    c->d_shape_prog.release();
    c->shape = d;
    c->mesh_rmax = 0.0;
    if (s->kind == ISDF_SHAPE_MESH)
        for (int v = 0; v < s->n_vertices; v++) {
            const double *q = s->mesh_vertices + 3 * v;
            c->mesh_rmax = std::max(c->mesh_rmax, std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]));
        }
    c->shape_host = *s;
    c->shape_host.mesh_vertices = nullptr;
    c->shape_host.mesh_faces = nullptr;
    c->have_shape = true;
    traj_watch_disarm(c);               // a kept clearance report answers for the old shape
    ISDF_REPLICATE(c, isdf_set_shape(p_, s));
    return ISDF_OK;
}

// A shape the library has no formula for, as the lattice BasicShape::initShape tabulates (Shape.hpp:361-404); sampled on the
// device like getonlySDFNum / getonlyGrad1Num / getSDFwithGrad1Num (:481-600).
extern "C" int isdf_set_shape_grid(isdf_ctx *c, const double *cells, int nx, int ny, int nz, const double grid_min[3], double nres,
                                   double bound_radius, const double *bbox_center, const double *bbox_half) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!cells || !grid_min || nx < 2 || ny < 2 || nz < 2 || !(nres > 0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad lattice (at least 2 nodes per axis)");
    if ((double)nx * ny * nz > 2.0e8) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "lattice too large");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)nx * ny * nz;
    free_mesh(c);
    ISDF_TRY(c->d_shape_grid.renew(c, n * 4));
    HIPCHK(c, hipMemcpy(c->d_shape_grid, cells, n * 4 * sizeof(double), hipMemcpyHostToDevice));
    DevShape d{};
    d.kind = ISDF_SHAPE_GRID; d.grad_mode = ISDF_GRAD_GRID;
    d.d.ident = d.f.ident = 1;
    for (int i = 0; i < 9; i++) { d.d.rot[i] = (i % 4 == 0) ? 1.0 : 0.0; d.f.rot[i] = (float)d.d.rot[i]; }
    d.grid = c->d_shape_grid; d.gn[0] = nx; d.gn[1] = ny; d.gn[2] = nz; d.gres = nres;
    for (int a = 0; a < 3; a++) d.gmin[a] = grid_min[a];
    // outside the lattice the sampler returns 1e20: the lattice box bounds everything that can carry a penalty
    const int dims[3] = {nx, ny, nz};
    double bb_c[3], bb_h[3], r2 = 0.0;
    for (int a = 0; a < 3; a++) {
        const double lo = grid_min[a], hi = grid_min[a] + (dims[a] - 1) * nres;
        bb_c[a] = 0.5 * (lo + hi); bb_h[a] = 0.5 * (hi - lo) + 1e-9;
        const double far = std::max(std::fabs(lo), std::fabs(hi));
        r2 += far * far;
    }
    if (bbox_center && bbox_half && bbox_half[0] > 0 && bbox_half[1] > 0 && bbox_half[2] > 0)
        for (int a = 0; a < 3; a++) { bb_c[a] = bbox_center[a]; bb_h[a] = bbox_half[a]; }
    d.bound_radius = bound_radius > 0 ? bound_radius : std::sqrt(r2);
    d.prune_rows = !env_is("ISDF_NO_ROW_PRUNE", '1');
    for (int a = 0; a < 3; a++) { d.bbox_lo[a] = (float)(bb_c[a] - bb_h[a]); d.bbox_hi[a] = (float)(bb_c[a] + bb_h[a]); }
    d.filter_f32 = 0;                      // no fp32 formula to pre-filter with
    d.mesh = nullptr;
    isdf_frontend_release(c);
    c->d_shape_prog.release();
    c->shape = d;
    c->shape_host = isdf_shape{};
    c->shape_host.kind = ISDF_SHAPE_GRID; c->shape_host.grad_mode = ISDF_GRAD_GRID;
    c->shape_host.bound_radius = d.bound_radius;
    for (int a = 0; a < 3; a++) { c->shape_host.bbox_center[a] = bb_c[a]; c->shape_host.bbox_half[a] = bb_h[a]; }
    c->have_shape = true;
    traj_watch_disarm(c);               // a kept clearance report answers for the old shape
    ISDF_REPLICATE(c, isdf_set_shape_grid(p_, cells, nx, ny, nz, grid_min, nres, bound_radius, bbox_center, bbox_half));
    return ISDF_OK;
}
extern "C" int isdf_set_shape_sampled(isdf_ctx *c, isdf_sdf_with_grad_fn fn, void *user, double ndx, double ndy, double ndz, double nres,
                                      double bound_radius, const double *bbox_center, const double *bbox_half) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!fn || !(ndx > 0) || !(ndy > 0) || !(ndz > 0) || !(nres > 0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad sampling arguments");
    // initShape (Shape.hpp:368-376): sizes ceil(nd / nres), the lattice starts at -nd / 2
    const int X = (int)std::ceil(ndx / nres), Y = (int)std::ceil(ndy / nres), Z = (int)std::ceil(ndz / nres);
    if (X < 2 || Y < 2 || Z < 2 || (double)X * Y * Z > 2.0e8) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad lattice size");
    const double mn[3] = {-ndx / 2, -ndy / 2, -ndz / 2};
    std::vector<double> cells((size_t)X * Y * Z * 4);
    for (int i = 0; i < X; i++)
        for (int j = 0; j < Y; j++)
            for (int k = 0; k < Z; k++) {
                const double p[3] = {mn[0] + i * nres, mn[1] + j * nres, mn[2] + k * nres};       // :390
                double g[3] = {0, 0, 0};
                const double dis = fn(user, p, g);                                                   // getSDFwithGrad1(p_rel, grad) :391
                double *o = cells.data() + 4 * (((size_t)i * Y + j) * Z + k);
                o[0] = g[0]; o[1] = g[1]; o[2] = g[2]; o[3] = dis;
            }
    return isdf_set_shape_grid(c, cells.data(), X, Y, Z, mn, nres, bound_radius, bbox_center, bbox_half);
}

// ---- ISDF_SHAPE_PROGRAM: a composition from the op library of the reference's CSG class (Shape.hpp:1684-2317) as an instruction
// list the device interprets (dev_shape_program.hpp).  Validated and lowered on the host (shape_program_host.hpp) before the ctx
// is touched: a rejected program leaves the installed shape as it was.
extern "C" int isdf_set_shape_program(isdf_ctx *c, const isdf_shape_instr *instr, int n, const double *trans, const double *rotate,
                                      double bound_radius, const double *bbox_center, const double *bbox_half) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    std::vector<isdf_shape_instr> low;
    {
        std::string why;
        if (isdf_host::prog_lower(instr, n, low, why) != ISDF_OK) return isdf_fail(c, ISDF_ERR_INVALID_ARG, why.c_str());
    }
    bool finite = std::isfinite(bound_radius) && bound_radius >= 0;
    for (int i = 0; i < 3; i++) finite = finite && (!trans || std::isfinite(trans[i])) && (!bbox_center || std::isfinite(bbox_center[i])) && (!bbox_half || std::isfinite(bbox_half[i]));
    for (int i = 0; i < 9; i++) finite = finite && (!rotate || std::isfinite(rotate[i]));
    if (!finite) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "shape program: non-finite body offset or bound");
    HIPCHK(c, hipSetDevice(c->device));
    // the instructions first, into a buffer of their own: a failure up to here leaves the installed shape usable
    DevBuf<isdf_shape_instr> d_prog;
    HIPCHK(c, d_prog.alloc(std::max<size_t>(low.size(), 1)));
    if (!low.empty()) HIPCHK(c, hipMemcpy(d_prog, low.data(), low.size() * sizeof(isdf_shape_instr), hipMemcpyHostToDevice));
    isdf_shape s;
    shape_identity(&s, ISDF_SHAPE_PROGRAM);
    s.grad_mode = ISDF_GRAD_CENTRAL;
    if (trans) std::memcpy(s.trans, trans, sizeof(s.trans));
    if (rotate) std::memcpy(s.rotate, rotate, sizeof(s.rotate));
    s.bound_radius = bound_radius;
    if (bbox_center) std::memcpy(s.bbox_center, bbox_center, sizeof(s.bbox_center));
    if (bbox_half) std::memcpy(s.bbox_half, bbox_half, sizeof(s.bbox_half));
    DevShape d{};
    double bb_c[3], bb_h[3];
    fill_dev_shape(&s, d, bb_c, bb_h);
    d.filter_f32 = 0;               // no float instantiation of the interpreter (yet): every listed voxel goes to the exact pass
    std::memset(c->mesh_info, 0, sizeof(c->mesh_info));
    isdf_frontend_release(c);
    c->d_shape_prog = std::move(d_prog);
    d.prog = c->d_shape_prog; d.prog_n = (int)low.size();
    c->shape = d;
    c->mesh_rmax = 0.0;
    c->shape_host = s;
    c->have_shape = true;
    traj_watch_disarm(c);               // a kept clearance report answers for the old shape
    ISDF_REPLICATE(c, isdf_set_shape_program(p_, instr, n, trans, rotate, bound_radius, bbox_center, bbox_half));
    return ISDF_OK;
}
extern "C" int isdf_shape_program_validate(const isdf_shape_instr *instr, int n, char *err_out, int err_cap) {
    std::vector<isdf_shape_instr> low;
    std::string why;
    const int rc = isdf_host::prog_lower(instr, n, low, why);
    if (err_out && err_cap > 0) { std::strncpy(err_out, why.c_str(), (size_t)err_cap - 1); err_out[err_cap - 1] = 0; }
    return rc;
}
extern "C" int isdf_shape_program_eval_host(const isdf_shape_instr *instr, int n, const double *trans, const double *rotate,
                                            const double *xyz, long long n_points, double *sdf_out, double *grad_out) {
    if (n_points < 0 || (n_points > 0 && !xyz)) return ISDF_ERR_INVALID_ARG;
    std::vector<isdf_shape_instr> low;
    std::string why;
    if (isdf_host::prog_lower(instr, n, low, why) != ISDF_OK) return ISDF_ERR_INVALID_ARG;
    const isdf_host::ProgBody B = isdf_host::prog_body(trans, rotate);
    for (long long i = 0; i < n_points; i++) {
        if (sdf_out) sdf_out[i] = isdf_host::prog_sdf(low.data(), (int)low.size(), B, xyz + 3 * i);
        if (grad_out) isdf_host::prog_grad(low.data(), (int)low.size(), B, xyz + 3 * i, grad_out + 3 * i);
    }
    return ISDF_OK;
}

extern "C" int isdf_mesh_info(const isdf_ctx *c, int info_out[16]) {
    if (!c || !info_out) return ISDF_ERR_INVALID_ARG;
    for (int k = 0; k < 16; k++) info_out[k] = c->mesh_info[k];
    return ISDF_OK;
}
