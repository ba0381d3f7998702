// Host side of the mesh kind's device tables (DevMesh, csrc/dev_shapes.hpp), built from the winding-number hierarchy of
// fwn_host.hpp: the child-major (node, child) records of the quad-cooperative walks, the flat slot blob of a small mesh, and the
// index-paired "closed" test.  Pure host arithmetic: shape_setup.hip uploads what these return, tests/native/mesh_tables_shim.cpp
// hands it to the CPU tests.  The record sizes and limits (MESH_Q_REC, MESH_Q_TRI, MESH_FLAT_SLOTS, MESH_FLAT_LEVELS) are arguments.
#pragma once
#include "fwn_host.hpp"
#include <array>
#include <functional>
#include <map>
#include <utility>

namespace isdf_host {

// child-major copies for the quad-cooperative walks (csrc/dev_mesh.hpp): lane l of a quad reads child l's record, child
// word and triangle in one round of loads.  tri / trif: nine doubles / floats per face; boxq: q_rec floats per (node, child)
// (0-22 the child's column of tree.box, 23 the child word, 24-32 a triangle child's vertices, 34-39 the child's box), triq: q_tri
// doubles per (node, child) (a triangle child's nine fp64 coordinates).
inline void mesh_child_records(const FwnTree &tree, const std::vector<double> &tri, const std::vector<float> &trif, const int q_rec, const int q_tri,
                               std::vector<float> &boxq, std::vector<double> &triq) {
    boxq.assign((size_t)4 * q_rec * tree.n_nodes(), 0.f);
    triq.assign((size_t)4 * q_tri * tree.n_nodes(), 0.0);
    // bounding box of every (node, child) from the fp64 vertices, rounded OUTWARDS to float (the closest-point walk's bound);
    // children have higher node numbers than their parents in this layout or not - a memoised recursion does not care
    std::vector<double> aabb((size_t)4 * 6 * tree.n_nodes());
    std::vector<char> aabb_done((size_t)tree.n_nodes(), 0);
    std::function<void(int)> node_boxes = [&](int nd) {
        if (aabb_done[nd]) return;
        aabb_done[nd] = 1;
        for (int ch = 0; ch < 4; ch++) {
            double *bb = aabb.data() + ((size_t)4 * nd + ch) * 6;
            for (int a = 0; a < 3; a++) { bb[a] = 1.0e300; bb[3 + a] = -1.0e300; }
            const int32_t ci = tree.child[(size_t)4 * nd + ch];
            if (ci == -1) continue;
            if (ci >= 0) {
                for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) { const double v = tri[(size_t)9 * ci + 3 * k + a]; bb[a] = std::min(bb[a], v); bb[3 + a] = std::max(bb[3 + a], v); }
            } else {
                const int sub = ci & 0x7fffffff;
                node_boxes(sub);
                for (int c2 = 0; c2 < 4; c2++) {
                    const double *sb = aabb.data() + ((size_t)4 * sub + c2) * 6;
                    for (int a = 0; a < 3; a++) { bb[a] = std::min(bb[a], sb[a]); bb[3 + a] = std::max(bb[3 + a], sb[3 + a]); }
                }
            }
        }
    };
    node_boxes(0);
    auto f_down = [](double v) { float f = (float)v; if ((double)f > v) f = std::nextafterf(f, -INFINITY); return f; };
    auto f_up = [](double v) { float f = (float)v; if ((double)f < v) f = std::nextafterf(f, INFINITY); return f; };
    for (int nd = 0; nd < tree.n_nodes(); nd++)
        for (int ch = 0; ch < 4; ch++) {
            float *rq = boxq.data() + ((size_t)4 * nd + ch) * q_rec;
            {
                const double *bb = aabb.data() + ((size_t)4 * nd + ch) * 6;
                const bool any = bb[0] <= bb[3];
                for (int a = 0; a < 3; a++) { rq[34 + a] = any ? f_down(bb[a]) : 3.0e38f; rq[37 + a] = any ? f_up(bb[3 + a]) : -3.0e38f; }
            }
            for (int k = 0; k < 23; k++) rq[k] = tree.box[(size_t)92 * nd + 4 * k + ch];
            const int32_t ci = tree.child[(size_t)4 * nd + ch];
            std::memcpy(&rq[23], &ci, 4);
            if (ci >= 0) {
                for (int k = 0; k < 9; k++) rq[24 + k] = trif[(size_t)9 * ci + k];
                for (int k = 0; k < 9; k++) triq[((size_t)4 * nd + ch) * q_tri + k] = tri[(size_t)9 * ci + k];
            }
        }
}

// The flat slot table of a (sub)tree rooted at `root` (DevMesh::flat / DevMesh::sub) - levels by breadth-first search from it.
// ONE self-describing blob, copied into LDS as it is: a header of 24 ints ([0..8] the slot index where level l begins, [9..17]
// the same for the combine steps over the nodes, deepest level first, [18] triangles, [19] slots, [20] levels, [21] the blob's
// size in 4-byte words, [22] / [23] where the records / the fp64 triangles begin), per slot 4 ints (record = 4 node + child,
// parent slot or -1, triangle index or -1, level), per triangle its slot, per node (deepest first) 5 ints (own slot or -1 for the
// root, its four child slots or -1), then per slot its fwn_boxq record (q_rec floats) and its fwn_triq triangle
// (q_tri doubles).  Empty: the subtree does not qualify (more than max_slots slots, or more than max_levels levels).
inline std::vector<int> mesh_flat_blob(const FwnTree &tree, const std::vector<float> &boxq, const std::vector<double> &triq, const int root, const int max_slots,
                                       const int max_levels, const int q_rec, const int q_tri) {
    const int nn_all = tree.n_nodes();
    std::vector<int> node_level((size_t)nn_all, -1), node_slot((size_t)nn_all, -1), order;
    node_level[root] = 0; order.push_back(root);
    int n_slots = 0;
    for (size_t h = 0; h < order.size(); h++) {
        const int nd = order[h];
        for (int ch = 0; ch < 4; ch++) {
            const int32_t ci = tree.child[(size_t)4 * nd + ch];
            if (ci == -1) continue;
            if (++n_slots > max_slots) return {};
            if (ci < 0) { const int sub = ci & 0x7fffffff; if (node_level[sub] < 0) { node_level[sub] = node_level[nd] + 1; order.push_back(sub); } }
        }
    }
    const int nn = (int)order.size();
    // slots in (level of their node, node in search order, child) order
    std::vector<int> slots, tris, nodes, lvl_begin(9, 0), step_begin(9, 0);
    int cur_level = -1;
    for (int nd : order) {
        if (node_level[nd] != cur_level) { cur_level = node_level[nd]; if (cur_level >= max_levels) return {}; lvl_begin[cur_level] = (int)slots.size() / 4; }
        for (int ch = 0; ch < 4; ch++) {
            const int32_t ci = tree.child[(size_t)4 * nd + ch];
            if (ci == -1) continue;
            const int sl = (int)slots.size() / 4;
            if (ci < 0) node_slot[ci & 0x7fffffff] = sl;
            else tris.push_back(sl);
            slots.push_back(4 * nd + ch); slots.push_back(node_slot[nd]); slots.push_back(ci >= 0 ? ci : -1); slots.push_back(node_level[nd]);
        }
    }
    const int n_levels = cur_level + 1;
    for (int l = n_levels; l < 9; l++) lvl_begin[l] = n_slots;
    // combine steps: the nodes of the deepest level first; per node its own slot and its four child slots
    std::map<int, std::array<int, 4>> child_slots;
    for (int nd : order) child_slots[nd] = {-1, -1, -1, -1};
    for (int sl = 0; sl < n_slots; sl++) { const int rec = slots[(size_t)4 * sl]; child_slots[rec >> 2][rec & 3] = sl; }
    int step = 0;
    for (int l = n_levels - 1; l >= 0; l--, step++) {
        step_begin[step] = (int)nodes.size() / 5;
        for (int nd : order) if (node_level[nd] == l) { nodes.push_back(node_slot[nd]); for (int ch = 0; ch < 4; ch++) nodes.push_back(child_slots[nd][ch]); }
    }
    for (int st = step; st < 9; st++) step_begin[st] = nn;
    std::vector<int> flat;
    flat.insert(flat.end(), lvl_begin.begin(), lvl_begin.end());
    flat.insert(flat.end(), step_begin.begin(), step_begin.end());
    flat.push_back((int)tris.size()); flat.push_back(n_slots); flat.push_back(n_levels); flat.push_back(0); flat.push_back(0); flat.push_back(0);
    flat.insert(flat.end(), slots.begin(), slots.end());
    flat.insert(flat.end(), tris.begin(), tris.end());
    flat.insert(flat.end(), nodes.begin(), nodes.end());
    while (flat.size() % 4) flat.push_back(0);
    const int rec_off = (int)flat.size();                 // (in 4-byte units)
    flat.resize(flat.size() + (size_t)n_slots * q_rec);
    for (int sl = 0; sl < n_slots; sl++)
        std::memcpy(flat.data() + rec_off + (size_t)sl * q_rec, boxq.data() + (size_t)slots[(size_t)4 * sl] * q_rec, q_rec * sizeof(float));
    const int trec_off = (int)flat.size();
    flat.resize(flat.size() + (size_t)n_slots * q_tri * 2);
    for (int sl = 0; sl < n_slots; sl++)
        std::memcpy(flat.data() + trec_off + (size_t)sl * q_tri * 2, triq.data() + (size_t)slots[(size_t)4 * sl] * q_tri, q_tri * sizeof(double));
    while (flat.size() % 4) flat.push_back(0);
    flat[21] = (int)flat.size(); flat[22] = rec_off; flat[23] = trec_off;
    return flat;
}

// "closed" by vertex INDEX: every edge twice, once in each direction.  A triangle soup (three vertices of its own per face) is
// open to this test whatever its geometry.
inline bool mesh_closed_by_index(const int32_t *faces, const int n_faces, const int n_vertices) {
    bool closed = true;
    std::vector<std::pair<long long, int>> edges;
    edges.reserve((size_t)3 * n_faces);
    for (int f = 0; f < n_faces; f++)
        for (int k = 0; k < 3; k++) {
            const long long a = faces[3 * f + k], b = faces[3 * f + (k + 1) % 3];
            edges.emplace_back(std::min(a, b) * (long long)n_vertices + std::max(a, b), a < b ? 1 : -1);
        }
    std::sort(edges.begin(), edges.end());
    for (size_t i = 0; i < edges.size() && closed; i += 2)       // every edge twice, once in each direction
        closed = i + 1 < edges.size() && edges[i].first == edges[i + 1].first && edges[i].second + edges[i + 1].second == 0 &&
                 (i + 2 >= edges.size() || edges[i + 2].first != edges[i].first);
    return closed;
}

}  // namespace isdf_host
