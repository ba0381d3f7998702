// Test shim: exposes the PRODUCT's host-side mesh tables (implicit-sdf-planner_amd/csrc/mesh_tables.hpp: child-major records, flat
// slot blob, index-paired "closed" test) to the CPU-only tests.  Built by tests/test_mesh_tables.py with g++.  The record sizes are
// those of csrc/dev_shapes.hpp (MESH_Q_REC = 40, MESH_Q_TRI = 10); the blob's limits (MESH_FLAT_SLOTS = 64, MESH_FLAT_LEVELS = 8)
// come from the test.
#include "mesh_tables.hpp"
namespace {
constexpr int Q_REC = 40, Q_TRI = 10;
struct Tables {
    isdf_host::FwnTree tree;
    std::vector<double> tri, triq;
    std::vector<float> trif, boxq;
};
}  // namespace
extern "C" {
void *shim_mt_build(const double *V, int nV, const int *F, int nF) {
    auto *t = new Tables();
    isdf_host::fwn_build(V, nV, F, nF, t->tree);
    t->tri.resize((size_t)9 * nF); t->trif.resize((size_t)9 * nF);
    for (int f = 0; f < nF; f++)
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) { t->tri[9 * f + 3 * k + a] = V[3 * F[3 * f + k] + a]; t->trif[9 * f + 3 * k + a] = (float)V[3 * F[3 * f + k] + a]; }
    isdf_host::mesh_child_records(t->tree, t->tri, t->trif, Q_REC, Q_TRI, t->boxq, t->triq);
    return t;
}
void shim_mt_destroy(void *h) { delete (Tables *)h; }
int shim_mt_num_nodes(void *h) { return ((Tables *)h)->tree.n_nodes(); }
void shim_mt_dump(void *h, int *child, float *box, float *boxq, double *triq) {
    auto *t = (Tables *)h;
    std::memcpy(child, t->tree.child.data(), t->tree.child.size() * sizeof(int));
    std::memcpy(box, t->tree.box.data(), t->tree.box.size() * sizeof(float));
    std::memcpy(boxq, t->boxq.data(), t->boxq.size() * sizeof(float));
    std::memcpy(triq, t->triq.data(), t->triq.size() * sizeof(double));
}
// the blob's size in ints (0: the tree does not qualify); copied into out when it fits into cap
int shim_mt_blob(void *h, int root, int max_slots, int max_levels, int *out, int cap) {
    auto *t = (Tables *)h;
    const std::vector<int> flat = isdf_host::mesh_flat_blob(t->tree, t->boxq, t->triq, root, max_slots, max_levels, Q_REC, Q_TRI);
    if (out && (int)flat.size() <= cap) std::memcpy(out, flat.data(), flat.size() * sizeof(int));
    return (int)flat.size();
}
int shim_mt_closed(const int *F, int nF, int nV) { return isdf_host::mesh_closed_by_index(F, nF, nV) ? 1 : 0; }
}
