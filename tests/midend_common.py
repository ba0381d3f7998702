"""Shared by tests/test_midend_host.py and tests/test_gpu_midend.py: the mid end's problems and its REFERENCE side - the reference's
own MINCO (pyoracle.ref_minco / ref_minco_propagate, compiled from its minco.hpp) with the pose penalty's dozen lines restated in
numpy (src/planner_algorithm/include/planner_algorithm/mid_end.hpp:184-199, 201-260, 262-304)."""
import numpy as np

PRM = dict(weight_pr=1000.0, rho_mid_end=200.0, rel_cost_tol=1e-6, min_step=1e-32, g_epsilon=0.0, integral_intervs=64, mem_size=16, past=10)


def forward_T(tau):          # forwardT (mid_end.hpp:116-128)
    tau = np.asarray(tau, dtype=np.float64)
    return np.where(tau > 0.0, (0.5 * tau + 1.0) * tau + 1.0, 1.0 / ((0.5 * tau - 1.0) * tau + 1.0))


def backward_T(T):           # backwardT (:131-143)
    T = np.asarray(T, dtype=np.float64)
    return np.where(T > 1.0, np.sqrt(np.maximum(2.0 * T - 1.0, 0.0)) - 1.0, 1.0 - np.sqrt(np.maximum(2.0 / T - 1.0, 0.0)))


def backward_grad_T(tau, gT):        # backwardGradT (:146-168)
    den = (0.5 * tau - 1.0) * tau + 1.0
    return np.where(tau > 0, gT * (tau + 1.0), gT * (1.0 - tau) / (den * den))


def sample_points(cm, T, N, intervs):
    """pos, vel of constraint i = piece i + 1 at s1 = T(i + 1) / intervs (:228-247); cm: 18N column-major coefficients."""
    c = cm.reshape(3, 6 * N)
    alpha = 1.0 / intervs
    pos = np.zeros((N - 1, 3)); vel = np.zeros((N - 1, 3)); beta0s = np.zeros((N - 1, 6))
    for i in range(N - 1):
        seg = i + 1
        s1 = alpha * T[seg]; s2 = s1 * s1; s3 = s2 * s1; s4 = s2 * s2; s5 = s4 * s1
        b0 = np.array([1.0, s1, s2, s3, s4, s5]); b1 = np.array([0.0, 1.0, 2.0 * s1, 3.0 * s2, 4.0 * s3, 5.0 * s4])
        blk = c[:, 6 * seg:6 * seg + 6]          # 3 x 6
        pos[i] = blk @ b0; vel[i] = blk @ b1; beta0s[i] = b0
    return pos, vel, beta0s


def ref_cost(orc, head, tail, ref, x, prm=PRM):
    """OriTraj::costFunction (:262-304) on the reference's own MINCO.  head / tail: 3 x 3 (columns pos, vel, acc), ref: (N-1) x 3.
    Returns (cost, g, parts [energy, pose, time], per-constraint cost_p, gradT of the objective before the tau chain rule)."""
    x = np.asarray(x, dtype=np.float64)
    N = (x.size + 3) // 4
    tau = x[:N]; way = x[N:].reshape(N - 1, 3)
    T = forward_T(tau)
    cm, e, gC, gT = orc.ref_minco(head, tail, way.T, T)
    gC = gC.copy(); gT = gT.copy()
    w = prm["weight_pr"]; alpha = 1.0 / prm["integral_intervs"]
    pos, vel, b0 = sample_points(cm, T, N, prm["integral_intervs"])
    cost = e; pen = 0.0; cps = np.zeros(N - 1)
    for i in range(N - 1):
        seg = i + 1
        d = pos[i] - ref[i]
        nrm = float(np.sqrt(d @ d))
        cost_p = nrm ** 3                                            # (:194)
        if not cost_p > 0:                                           # (:198, :249): skipped
            continue
        gradp = 3 * nrm ** 2 * (d / nrm)                             # (:195)
        for a in range(3):
            gC[a * 6 * N + 6 * seg:a * 6 * N + 6 * seg + 6] += w * (b0[i] * gradp[a])      # (:252,255)
        gT[seg] += w * (cost_p * (alpha * float(gradp @ vel[i])))    # (:253,256): the reference's extra factor cost_p
        cost += w * cost_p; pen += w * cost_p; cps[i] = cost_p       # (:257)
    gP, gTt = orc.ref_minco_propagate(head, tail, way.T, T, gC, gT)  # (:295)
    rho = prm["rho_mid_end"]
    cost += rho * T.sum()                                            # (:298)
    g = np.concatenate([backward_grad_T(tau, gTt + rho), gP.T.reshape(-1)])     # (:300-302)
    return float(cost), g, np.array([e, pen, rho * T.sum()]), cps, gTt


def ends(rng, span):
    head = np.zeros((3, 3)); tail = np.zeros((3, 3))
    head[:, 0] = rng.uniform(0, 2, 3); head[:, 1] = rng.normal(0, 1, 3); head[:, 2] = rng.normal(0, 0.5, 3)
    tail[:, 0] = head[:, 0] + span; tail[:, 1] = rng.normal(0, 1, 3)
    return head, tail


def cost_problem(N, seed, mix=False):
    """A callback's inputs: durations log-uniform in 0.05 .. 12 s (mix: alternating 0.1 / 10 s, 100:1), waypoints and reference
    points scattered about a line of 3 m per piece."""
    rng = np.random.default_rng(seed)
    head, tail = ends(rng, np.array([3.0 * N, 0.4 * N, 0.2 * N]))
    line = np.linspace(head[:, 0], tail[:, 0], N + 1)[1:-1]
    way = line + rng.normal(0, 0.6, (N - 1, 3))
    ref = line + rng.normal(0, 0.6, (N - 1, 3))
    T = np.exp(rng.uniform(np.log(0.05), np.log(12.0), N))
    if mix:
        T = np.where(np.arange(N) % 2 == 0, 0.1, 10.0)
    x = np.concatenate([backward_T(T), way.reshape(-1)])
    return head, tail, ref, x


def ref_sensitivity(orc, head, tail, ref, x, prm=PRM, trials=2):
    """How far the reference side itself moves (cost, g(tau), g(waypoints): each relative to its largest entry) when every input
    changes by one ulp: the floor under any comparison against it, whatever computes the other side."""
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    c0, g0 = ref_cost(orc, head, tail, ref, x, prm)[:2]
    N = (x.size + 3) // 4
    worst = 0.0
    for s in range(trials):
        xp = x * (1.0 + np.random.default_rng(s).choice([-1.0, 1.0], x.size) * 2.0 ** -52)
        c1, g1 = ref_cost(orc, head, tail, ref, xp, prm)[:2]
        worst = max(worst, abs(c1 - c0) / abs(c0), rel(g1[:N], g0[:N]), rel(g1[N:], g0[N:]))
    return worst


def posed_cost_problem(orc, N, seed, floor):
    """cost_problem(N, seed + 1000 k) for the first k at which the reference side's own one-ulp sensitivity is at most `floor`.
    Durations spread over 0.05 .. 12 s inside one long trajectory can condition the reference's unpivoted band LU so badly that
    its own result moves by more than the comparison's tolerance when its inputs move by an ulp (N = 320, seed 620: 4e-10); such
    an input measures the reference, not the code compared with it.  Returns (seed used, sensitivity, problem)."""
    for k in range(8):
        prob = cost_problem(N, seed + 1000 * k)
        sens = ref_sensitivity(orc, *prob)
        if sens <= floor:
            return seed + 1000 * k, sens, prob
    raise AssertionError(f"no well-posed problem found for N = {N} from seed {seed}")


def fit_problem(N, inittime=2.5):
    """Waypoints every 3 m along a gently bent line, at rest at both ends, T_init = inittime per piece (2.5 s in every shipped yaml; plan_manager.cpp:206-213)."""
    s = 3.0 * np.arange(N + 1)
    pts = np.stack([s, 0.15 * s * np.sin(0.05 * np.arange(N + 1)), 0.02 * s], axis=1)
    head = np.zeros((3, 3)); tail = np.zeros((3, 3))
    head[:, 0] = pts[0]; tail[:, 0] = pts[-1]
    return head, tail, pts[1:-1].copy(), np.full(N, float(inittime))


def colmajor9(M):
    return np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)


def prm_array(prm=PRM):
    return np.array([prm[k] for k in ("weight_pr", "rho_mid_end", "rel_cost_tol", "min_step", "g_epsilon", "integral_intervs", "mem_size", "past")],
                    dtype=np.float64)
