// Stand-alone program for the sanitizers (tests/test_shape_program_host.py builds it with -fsanitize=address,undefined and runs
// it): the validator and the evaluator of ISDF_SHAPE_PROGRAM on malformed programs and on 10 000 seeded random instruction
// arrays.  Host code only.
#include "shape_program_host.hpp"
#include <cstdio>
#include <cstdint>
#include <limits>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double rndu() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static isdf_shape_instr mk(int op, std::initializer_list<double> p = {}) {
    isdf_shape_instr I{};
    I.op = op;
    int k = 0;
    for (double v : p) I.p[k++] = v;
    return I;
}
// validator, then the evaluator on what it lowered AND on the raw array (which it must survive whatever it holds)
static int feed(const std::vector<isdf_shape_instr> &prog, int n, int &accepted) {
    std::vector<isdf_shape_instr> low;
    std::string why;
    const int rc = isdf_host::prog_lower(n >= 0 ? prog.data() : nullptr, n, low, why);
    const double pts[4][3] = {{0, 0, 0}, {0.3, -1.2, 2.5}, {-4.0, 0.0, 0.1}, {1e3, -1e3, 1e-3}};
    const isdf_host::ProgBody B = isdf_host::prog_body(nullptr, nullptr);
    volatile double sink = 0;
    for (const auto &p : pts) {
        if (rc == ISDF_OK) { double g[3]; sink = sink + isdf_host::prog_sdf(low.data(), (int)low.size(), B, p); isdf_host::prog_grad(low.data(), (int)low.size(), B, p, g); sink = sink + g[0]; }
        if (n > 0 && n <= (int)prog.size()) sink = sink + isdf_host::prog_eval(prog.data(), n, p);
    }
    if (rc == ISDF_OK) accepted++;
    else if (why.empty()) return 1;      // every rejection carries its reason
    return 0;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int bad = 0, accepted = 0;
    std::vector<std::vector<isdf_shape_instr>> malformed = {
        {mk(99)}, {mk(0)}, {mk(-5)},                                                   // unknown opcodes
        {mk(ISDF_OP_NEGATE)}, {mk(ISDF_OP_SPHERE, {1}), mk(ISDF_OP_UNION, {0})},        // underflow
        {mk(ISDF_OP_SPHERE, {1}), mk(ISDF_OP_SPHERE, {1})},                             // two values left
        {mk(ISDF_OP_TRANSLATE, {1, 2, 3})},                                             // none left
        {mk(ISDF_OP_SPHERE, {nan})}, {mk(ISDF_OP_BOX, {1, inf, 1})},                    // non-finite
        {mk(ISDF_OP_SCALE, {1, 0, 1}), mk(ISDF_OP_SPHERE, {1})},                        // zero scale
        {mk(ISDF_OP_CAPSULE, {1, 2, 3, 1, 2, 3, 0.5})}, {mk(ISDF_OP_CAPPED_CYLINDER, {0, 0, 0, 0, 0, 0, 1})},
        {mk(ISDF_OP_CAPPED_CONE, {1, 2, 0, 0, 1, 0, 0, 1})}, {mk(ISDF_OP_ROUNDED_CONE, {1, 0.5, 0})},
        {mk(ISDF_OP_SPHERE, {1}), mk(ISDF_OP_SPHERE, {2}), mk(ISDF_OP_UNION, {-0.1})},  // k < 0
        {mk(ISDF_OP_ROTATE_TO, {0, 0, 0, 0, 0, 0}), mk(ISDF_OP_ROTATE, {1, 0, 0, 0}), mk(ISDF_OP_ELLIPSOID, {0, 0, 0})},       // accepted; NaN values
    };
    {   // depth 9, 65 instructions
        std::vector<isdf_shape_instr> deep, longp;
        for (int i = 0; i < 9; i++) deep.push_back(mk(ISDF_OP_SPHERE, {1.0 + i}));
        for (int i = 0; i < 8; i++) deep.push_back(mk(ISDF_OP_UNION, {0.1}));
        longp.push_back(mk(ISDF_OP_SPHERE, {1}));
        for (int i = 0; i < 64; i++) longp.push_back(mk(ISDF_OP_NEGATE));
        malformed.push_back(deep); malformed.push_back(longp);
    }
    for (const auto &m : malformed) bad += feed(m, (int)m.size(), accepted);
    bad += feed({}, 0, accepted); bad += feed({}, -1, accepted); bad += feed({mk(ISDF_OP_SPHERE, {1})}, -3, accepted);
    std::printf("malformed ok: %d programs, %d accepted\n", (int)malformed.size() + 3, accepted);
    // random arrays: mostly known opcodes so that many get past the first instruction; parameters from a mix of magnitudes and specials
    const int ops[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 32, 33, 34, 35, 36, 37, 48, 49, 50, 51, 52, 64, 65, 66, 67, 0, 18, 31, 68, -1, 1000};
    const double specials[] = {0.0, -0.0, 1.0, -1.0, 0.5, 1e-300, 1e300, inf, -inf, nan};
    accepted = 0;
    for (int t = 0; t < 10000; t++) {
        const int n = 1 + (int)(rnd() % (t % 50 == 0 ? 70 : 12));
        std::vector<isdf_shape_instr> prog((size_t)n);
        for (auto &I : prog) {
            I.op = ops[rnd() % (sizeof(ops) / sizeof(ops[0]))];
            I.reserved = (int)rnd();
            for (double &v : I.p) v = (rnd() % 16 == 0) ? specials[rnd() % 10] : (rndu() - 0.5) * (rnd() % 4 == 0 ? 100.0 : 4.0);
        }
        if (t % 3 == 0) {       // bias towards valid shapes: a primitive first, reductions last
            prog[0].op = ops[rnd() % 17];
            for (int i = 1; i < n; i++) prog[i].op = (i % 2) ? ops[rnd() % 17] : ops[28 + rnd() % 4];
        }
        bad += feed(prog, n, accepted);
    }
    std::printf("random ok: 10000 arrays, %d accepted\n", accepted);
    return bad ? 1 : 0;
}
