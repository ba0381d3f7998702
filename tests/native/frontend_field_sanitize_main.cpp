// frontend_field_host.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_frontend_field_host.py): the
// maps of tests/field_reference.py, each result held to the definition - d[goal] = 0, every free voxel's d is the minimum of
// fl(d[u] + w) over its free neighbours, everything else is +inf.
#include "frontend_field_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Map {
    int X, Y, Z;
    std::vector<unsigned char> occ;
    Map(int x, int y, int z) : X(x), Y(y), Z(z), occ((size_t)x * y * z, 0) {}
    unsigned char &at(int x, int y, int z) { return occ[((size_t)x * Y + y) * Z + z]; }
};

constexpr int N_ATT = 121, NW = 4;

std::vector<uint32_t> table(Map &m) {
    std::vector<uint32_t> t((size_t)m.X * m.Y * m.Z * NW, 0u);
    for (int x = 0; x < m.X; x++)
        for (int y = 0; y < m.Y; y++)
            for (int z = 0; z < m.Z; z++)
                if (!m.at(x, y, z)) {
                    const int a = (x + 3 * y + 5 * z) % N_ATT;
                    t[(((size_t)x * m.Y + y) * m.Z + z) * NW + a / 32] = 1u << (a % 32);
                }
    return t;
}

int failures = 0;

// returns the number of finite voxels, -1 on a violation of the definition
long long hold(Map &m, const int goal[3], const std::vector<double> &d, bool reachable) {
    long long finite = 0;
    const bool goal_in = goal[0] >= 0 && goal[0] < m.X && goal[1] >= 0 && goal[1] < m.Y && goal[2] >= 0 && goal[2] < m.Z;
    for (int x = 0; x < m.X; x++)
        for (int y = 0; y < m.Y; y++)
            for (int z = 0; z < m.Z; z++) {
                const double dv = d[((size_t)x * m.Y + y) * m.Z + z];
                if (std::isfinite(dv)) finite++;
                if (!reachable || m.at(x, y, z)) { if (!std::isinf(dv)) return -1; continue; }
                if (goal_in && x == goal[0] && y == goal[1] && z == goal[2]) { if (dv != 0.0) return -1; continue; }
                double best = std::numeric_limits<double>::infinity();
                for (int i = -1; i < 2; i++)
                    for (int j = -1; j < 2; j++)
                        for (int k = -1; k < 2; k++) {
                            if (!(i | j | k)) continue;
                            const int vx = x + i, vy = y + j, vz = z + k;
                            if (vx < 0 || vx >= m.X || vy < 0 || vy >= m.Y || vz < 0 || vz >= m.Z || m.at(vx, vy, vz)) continue;
                            const double cand = d[((size_t)vx * m.Y + vy) * m.Z + vz] + std::sqrt((double)(i * i + j * j + k * k));
                            if (cand < best) best = cand;
                        }
                if (!(dv == best)) return -1;
            }
    return finite;
}

void run(const char *name, Map &m, int gx, int gy, int gz, bool want_reachable, long long want_finite) {
    const std::vector<uint32_t> t = table(m);
    std::vector<double> d((size_t)m.X * m.Y * m.Z, -1.0);
    const int goal[3] = {gx, gy, gz};
    const bool r = isdf_host::field_dijkstra(t.data(), m.X, m.Y, m.Z, N_ATT, goal, d.data());
    const long long finite = hold(m, goal, d, r);
    const bool ok = r == want_reachable && finite >= 0 && (want_finite < 0 || finite == want_finite);
    if (!ok) failures++;
    std::printf("%s %s: reachable %d, finite voxels %lld\n", name, ok ? "ok" : "FAILED", (int)r, finite);
}

}  // namespace

int main() {
    {
        Map m(9, 7, 5);
        run("open", m, 1, 5, 3, true, 9 * 7 * 5);
        run("goal outside the map", m, 9, 0, 0, false, 0);
    }
    {
        Map m(9, 7, 5);
        for (int y = 0; y < 7; y++) for (int z = 0; z < 5; z++) m.at(4, y, z) = 1;
        m.at(4, 3, 2) = 0;
        run("wall with a gap", m, 0, 0, 0, true, 9 * 7 * 5 - 34);
    }
    {
        Map m(9, 7, 5);
        for (int x = 3; x < 8; x++) for (int y = 1; y < 6; y++) for (int z = 0; z < 5; z++) m.at(x, y, z) = 1;
        for (int x = 4; x < 7; x++) for (int y = 2; y < 5; y++) for (int z = 1; z < 4; z++) m.at(x, y, z) = 0;
        run("sealed pocket", m, 0, 0, 0, true, 9 * 7 * 5 - 125);                 // the 27 cells inside stay +inf
        run("goal in the pocket", m, 5, 3, 2, true, 27);
        run("goal not free", m, 3, 1, 0, false, 0);
    }
    {
        Map m(20, 20, 3);
        for (int y = 1; y < 20; y += 2) {
            for (int x = 0; x < 20; x++) for (int z = 0; z < 3; z++) m.at(x, y, z) = 1;
            for (int z = 0; z < 3; z++) m.at((y / 2) % 2 == 0 ? 19 : 0, y, z) = 0;
        }
        run("serpentine", m, 0, 0, 1, true, 20 * 10 * 3 + 10 * 3);
    }
    std::printf(failures ? "FAILED\n" : "all ok\n");
    return failures ? 1 : 0;
}
