// Stand-alone program for the sanitizers (tests/test_midend_host.py builds it with -fsanitize=address,undefined and runs it):
// the host mid end's cost and a short fit at N = 2, 5, 40.  Host code only.
#include "midend_host.hpp"
#include <cstdio>

int main() {
    const int shapes[3] = {2, 5, 40};
    for (int N : shapes) {
        double head[9] = {0}, tail[9] = {0};
        head[3] = 0.5;                                  // start velocity along x
        tail[0] = 3.0 * N; tail[1] = 1.0;
        std::vector<double> ref((size_t)3 * (N - 1)), T(N, 1.0 + 0.01 * N);
        for (int i = 0; i < N - 1; i++) { ref[3 * i] = 3.0 * (i + 1); ref[3 * i + 1] = 0.3 * std::sin(0.7 * i); ref[3 * i + 2] = 0.05 * i; }
        isdf_host::MidendParams p;
        isdf_host::Midend m;
        m.setup(head, tail, N, ref.data(), p);
        const int n = N + 3 * (N - 1);
        std::vector<double> x(n), g(n);
        m.seed(T.data(), x.data());
        const double c0 = m.cost(x.data(), g.data());
        isdf_host::Lbfgs opt;
        opt.param = isdf_host::midend_lbfgs_params(p);
        opt.param.max_iterations = 12;                  // a short fit
        opt.evaluate = isdf_host::Midend::evaluate; opt.instance = &m;
        const isdf_host::LbfgsResult r = opt.minimize(x.data(), n);
        if (!std::isfinite(c0) || !std::isfinite(r.f) || !(r.f <= c0)) { std::printf("N=%d: cost %g -> %g (status %d)\n", N, c0, r.f, r.status); return 1; }
        std::printf("N=%d ok: cost %.9g -> %.9g, status %d, %d evaluations\n", N, c0, r.f, r.status, r.evaluations);
    }
    return 0;
}
