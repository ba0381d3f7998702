"""NumPy restatement of the routed view selection (include/isdf_accel.h, "the routed view selection"): the sets are
tests/view_select_reference.py's, the rounds a plain greedy loop over the utility np.float64(m) / (np.float64(cost0) + c) with argmax
(the first of the largest).  Nothing here calls isdf_view_select*."""
import numpy as np

import known_reference as kr
import view_gain_reference as vr
import view_select_reference as sr

ROUTE_WORDS = ("n_eligible", "n_unreachable", "n_over_budget")


def info_words(info):
    """the integer words of an IsdfViewSelectRoutedInfo, in the order of `select`'s "info\""""
    return tuple(getattr(info.select, w) for w in sr.INFO_WORDS) + tuple(getattr(info, w) for w in ROUTE_WORDS)


def select(vs, k, k_select, min_gain, cost, cost0=1.0, max_cost=np.inf):
    """{"rows", "select", "round", "claimed", "cost", "util" [k_select, 2], "cost_selected", "info": INFO_WORDS' + ROUTE_WORDS' values}"""
    k = np.asarray(k, dtype=bool)
    cost = np.asarray(cost, dtype=np.float64).reshape(-1)
    rows = vr.rows(vs, k)
    U = sr.sets(vs, k)
    n = len(vs)
    assert cost.shape == (n,) and min_gain >= 1
    scored = np.array([u is not None for u in U], dtype=bool)
    ok = scored & np.isfinite(cost) & (cost <= max_cost)
    claimed = np.zeros(k.size, dtype=bool)
    sel = np.zeros((k_select, 4), dtype=np.int64)
    sel[:, 0] = -1
    util = np.zeros((k_select, 2))
    rnd = np.full(n, -1, dtype=np.int64)
    n_selected = cumulative = solo = 0
    cost_selected = np.float64(0.0)
    for r in range(k_select):
        left = [j for j in range(n) if ok[j] and rnd[j] < 0]
        m = {j: int((U[j] & ~claimed).sum()) for j in left}
        left = [j for j in left if m[j] >= min_gain]
        if not left:
            break
        u = np.array([np.float64(m[j]) / (np.float64(cost0) + cost[j]) for j in left])
        j = left[int(np.argmax(u))]              # the first of the largest: the lowest index
        claimed |= U[j]
        cumulative += m[j]
        solo += int(rows[j, 1])
        sel[r] = [j, m[j], cumulative, rows[j, 1] - m[j]]
        util[r] = [cost[j], u.max()]
        cost_selected = cost_selected + cost[j]
        rnd[j] = r
        n_selected = r + 1
    list_words = sum(int((kr.pack(u.reshape(k.shape)) != 0).sum()) for u in U if u is not None)
    info = (n, int(scored.sum()), n_selected, cumulative, solo, int(rows[scored, 1].max()) if scored.any() else 0, list_words,
            int(ok.sum()), int((scored & ~np.isfinite(cost)).sum()), int((scored & np.isfinite(cost) & ~(cost <= max_cost)).sum()))
    return {"rows": rows, "select": sel, "round": rnd, "claimed": kr.pack((k.reshape(-1) | claimed).reshape(k.shape)), "cost": cost.copy(), "util": util,
            "cost_selected": float(cost_selected), "info": info}
