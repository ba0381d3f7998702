"""NumPy restatement of the view selection (include/isdf_accel.h, "the view selection") from code older than it: S_j is
tests/view_gain_reference.py's `views` / `seen` (built from the depth rays', the ray cast's and the scan's host forms), U_j its mask by
~K, the rounds a plain greedy loop with argmax (the first of the largest).  Nothing here calls isdf_view_select*."""
import numpy as np

import known_reference as kr
import view_gain_reference as vr

INFO_WORDS = ("n_views", "n_scored", "n_selected", "gain_selected", "gain_solo_sum", "best_single_gain", "list_words")


def sets(vs, k):
    """U_j as flat boolean arrays, None for a view that is not scored"""
    unknown = ~np.asarray(k, dtype=bool).reshape(-1)
    return [None if v is None else vr.seen(v, unknown.size) & unknown for v in vs]


def select(vs, k, k_select, min_gain):
    """{"rows", "select", "round", "claimed" (K | C_final as words), "claimed_mask" (C_final, bool), "sets" (the U_j), "info": INFO_WORDS' values}"""
    k = np.asarray(k, dtype=bool)
    rows = vr.rows(vs, k)
    U = sets(vs, k)
    n = len(vs)
    claimed = np.zeros(k.size, dtype=bool)
    sel = np.zeros((k_select, 4), dtype=np.int64)
    sel[:, 0] = -1
    rnd = np.full(n, -1, dtype=np.int64)
    n_selected = cumulative = solo = 0
    for r in range(k_select):
        left = [j for j in range(n) if U[j] is not None and rnd[j] < 0]
        if not left:
            break
        m = np.array([int((U[j] & ~claimed).sum()) for j in left])
        i = int(np.argmax(m))                   # the first of the largest: the lowest index
        if m[i] < min_gain:
            break
        j = left[i]
        claimed |= U[j]
        cumulative += int(m[i])
        solo += int(rows[j, 1])
        sel[r] = [j, m[i], cumulative, rows[j, 1] - m[i]]
        rnd[j] = r
        n_selected = r + 1
    assert cumulative == int(claimed.sum())
    scored = rows[:, 0] == 0
    list_words = sum(int((kr.pack(u.reshape(k.shape)) != 0).sum()) for u in U if u is not None)
    info = (n, int(scored.sum()), n_selected, cumulative, solo, int(rows[scored, 1].max()) if scored.any() else 0, list_words)
    return {"rows": rows, "select": sel, "round": rnd, "claimed": kr.pack((k.reshape(-1) | claimed).reshape(k.shape)), "claimed_mask": claimed, "sets": U, "info": info}


def top_k_by_solo_gain(rows, k):
    """what ranking by each view's own gain would pick: the scored views by gain descending, ties to the lower index"""
    scored = np.flatnonzero(rows[:, 0] == 0)
    return scored[np.argsort(-rows[scored, 1], kind="stable")][:k].tolist()
