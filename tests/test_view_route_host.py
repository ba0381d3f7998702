"""The routed view selection without a device (csrc/view_select_host.hpp through isdf_view_select_routed_host) against the NumPy
restatement (tests/view_route_reference.py), == on rows, select, round, claimed, cost, util (as bytes) and the integer words of the info.
The scene is the view selection's base case (tests/view_select_cases.py) on 24 x 20 x 70 voxels with the view gain's camera; the costs are
tests/view_route_cases.py's and this file's."""
import ctypes as C

import numpy as np
import pytest

import known_reference as kr
import view_gain_reference as vr
import view_route_cases as rc
import view_route_reference as rr
import view_select_cases as cs
import view_select_reference as sr
from test_view_gain_host import STRIDES, cam_of
from test_view_select_host import case_of, views_of

RES = cs.RES
DIMS = cs.BASE_DIMS
NAMES = ("rows", "select", "round", "claimed", "cost", "util")
# the base case's travel costs, in cells: the two big views far away, the smaller one (2, and 4, the same pose) and the small one (7) near
COSTS = np.array([40.0, 38.5, 3.0, 1.0, 3.0, 0.0, 12.25, 2.0 ** 0.5])


def _host(pkg, lib, k, cost, poses=None, **params):
    occ, _, base, rng_m = case_of(pkg, DIMS)
    params.setdefault("stride", 1)
    return pkg.engine.view_select_routed_host(kr.pack(k), occ, np.zeros(3), np.array(DIMS) * RES, RES, cam_of(pkg), base if poses is None else poses, cost, lib=lib,
                                              max_range_m=rng_m, **params)


def _same(got, ref, what=None):
    for a, name in zip(got[:6], NAMES):
        b = ref[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, a, b)
    assert rr.info_words(got[6]) == ref["info"], (what, rr.info_words(got[6]), ref["info"])
    assert np.float64(got[6].cost_selected).tobytes() == np.float64(ref["cost_selected"]).tobytes() and got[6].cost_source == 1
    assert (got[6].cost_ms, got[6].paths_ms, got[6].select.chunks) == (0.0, 0.0, 0)


def test_equal_costs_give_the_plain_selection(pkg, product_lib):
    """all costs 0 and cost0 = 1: u = m, and the outputs are isdf_view_select_host's to the byte"""
    occ, k, poses, rng_m = case_of(pkg, DIMS)
    n = len(poses)
    for stride in STRIDES:
        vs = views_of(pkg, product_lib, DIMS, stride)
        largest = int(vr.rows(vs, k)[:, 1].max())
        for k_select in (1, 3, n + 1):
            for min_gain in (1, largest, largest + 1):
                got = _host(pkg, product_lib, k, np.zeros(n), stride=stride, k_select=k_select, min_gain=min_gain, cost0=1.0)
                _same(got, rr.select(vs, k, k_select, min_gain, np.zeros(n)), (stride, k_select, min_gain))
                plain = pkg.engine.view_select_host(kr.pack(k), occ, np.zeros(3), np.array(DIMS) * RES, RES, cam_of(pkg), poses, lib=product_lib, stride=stride,
                                                    max_range_m=rng_m, k_select=k_select, min_gain=min_gain)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], plain[:4]))
                assert [getattr(got[6].select, w) for w in sr.INFO_WORDS] == [getattr(plain[4], w) for w in sr.INFO_WORDS]
                ns = plain[4].n_selected
                assert not got[4].any() and np.array_equal(got[5][:ns, 1], plain[1][:ns, 1].astype(np.float64)) and not got[5][ns:].any()


def test_the_cost_changes_the_order(pkg, product_lib):
    """by the restatement alone: plain greedy takes one of the two big views first, routed greedy the near one with the smaller gain"""
    _, k, poses, _ = case_of(pkg, DIMS)
    n = len(poses)
    for stride in STRIDES:
        vs = views_of(pkg, product_lib, DIMS, stride)
        plain, routed = sr.select(vs, k, n, 1), rr.select(vs, k, n, 1, COSTS)
        assert plain["select"][0, 0] in (0, 1) and routed["select"][0, 0] == 2 and plain["rows"][2, 1] < plain["rows"][0, 1]
        assert routed["info"][2] >= 3 and set(routed["select"][:routed["info"][2], 0]) != set(plain["select"][:plain["info"][2], 0]) or \
            routed["select"][:, 0].tolist() != plain["select"][:, 0].tolist()
        assert routed["util"][0, 1] == plain["rows"][2, 1] / 4.0 and routed["cost_selected"] == routed["util"][:, 0].sum()
        for k_select, cost0, max_cost in ((n, 1.0, np.inf), (2, 0.25, np.inf), (n, 1.0, 12.25), (n, 7.0, 3.0)):
            _same(_host(pkg, product_lib, k, COSTS, stride=stride, k_select=k_select, cost0=cost0, max_cost=max_cost),
                  rr.select(vs, k, k_select, 1, COSTS, cost0, max_cost), (stride, k_select, cost0, max_cost))


def test_utility_ties_go_to_the_lower_index(pkg, product_lib):
    """(m, cost0 + c) = (4, 2) and (2, 1): u = 2 both; the lower index wins, and swapped the other does"""
    _, _, poses, _ = case_of(pkg, DIMS)
    vs = views_of(pkg, product_lib, DIMS, (1, 1))
    n_vox = int(np.prod(DIMS))
    k = rc.tie_known(vr.seen(vs[0], n_vox), vr.seen(vs[2], n_vox), DIMS)
    for order, cost, first in (((0, 2), (1.0, 0.0), 4), ((2, 0), (0.0, 1.0), 2)):
        pair = [vs[j] for j in order]
        ref = rr.select(pair, k, 2, 1, cost)
        assert ref["rows"][:, 1].tolist() == [first, 6 - first] and ref["select"][:, :2].tolist() == [[0, first], [1, 6 - first]] and ref["util"][:, 1].tolist() == [2.0, 2.0]
        _same(_host(pkg, product_lib, k, cost, poses=poses[list(order)], k_select=2), ref, order)
    # one unit in the last place of cost0 + c more on the lower index and the other goes first (2 + 2^-51 is the next double above 2)
    hair = (1.0 + 2.0 ** -51, 0.0)
    ref = rr.select([vs[0], vs[2]], k, 2, 1, hair)
    assert ref["select"][:, 0].tolist() == [1, 0] and ref["util"][:, 1].tolist() == [2.0, 4.0 / (2.0 + 2.0 ** -51)] and ref["util"][1, 1] < 2.0
    _same(_host(pkg, product_lib, k, hair, poses=poses[[0, 2]], k_select=2), ref)


def test_reachability_and_budget(pkg, product_lib):
    _, k, poses, _ = case_of(pkg, DIMS)
    n = len(poses)
    vs = views_of(pkg, product_lib, DIMS, (1, 1))
    cost = COSTS.copy()
    cost[[0, 2]] = np.inf                       # the first picks of both orders are out of reach
    got = _host(pkg, product_lib, k, cost, k_select=n)
    _same(got, rr.select(vs, k, n, 1, cost), "inf")
    assert got[2][0] == got[2][2] == -1 and got[6].n_unreachable == 2 and got[6].select.n_selected >= 2 and np.isfinite(got[5]).all()
    # c == max_cost is eligible, the next double above is not
    for max_cost, in_budget in ((COSTS[4], True), (np.nextafter(COSTS[4], 0.0), False)):
        c2 = COSTS.copy()
        c2[2] = np.inf
        got = _host(pkg, product_lib, k, c2, k_select=n, max_cost=max_cost)
        _same(got, rr.select(vs, k, n, 1, c2, 1.0, max_cost), max_cost)
        assert (got[2][4] >= 0) == in_budget and got[6].n_over_budget == (3 if in_budget else 4) and got[6].n_unreachable == 1
    # more rounds than eligible views
    got = _host(pkg, product_lib, k, COSTS, k_select=n + 3, max_cost=3.0)
    ref = rr.select(vs, k, n + 3, 1, COSTS, 1.0, 3.0)
    _same(got, ref, "k_select > eligible")
    assert got[6].n_eligible == 4 and got[6].select.n_selected < got[6].n_eligible and (got[1][got[6].select.n_selected:] == [-1, 0, 0, 0]).all()
    # every view ineligible: nothing is picked and claimed is K
    for cost, max_cost in ((np.full(n, np.inf), np.inf), (COSTS + 1.0, 0.5)):
        got = _host(pkg, product_lib, k, cost, k_select=n, max_cost=max_cost)
        _same(got, rr.select(vs, k, n, 1, cost, 1.0, max_cost), max_cost)
        assert got[6].select.n_selected == 0 and got[6].n_eligible == 0 and np.array_equal(got[3], kr.pack(k)) and not got[5].any() and got[6].cost_selected == 0.0
    # no views
    got = _host(pkg, product_lib, k, np.zeros(0), poses=poses[:0], k_select=3)
    _same(got, rr.select([], k, 3, 1, np.zeros(0)), "no views")
    assert got[1].tolist() == [[-1, 0, 0, 0]] * 3 and np.array_equal(got[3], kr.pack(k))


def test_struct_sizes_and_defaults(pkg, product_lib):
    sz = (C.c_int * 2)()
    product_lib.isdf_view_select_routed_sizes(sz)
    assert list(sz) == [C.sizeof(pkg.capi.IsdfViewSelectRoutedParams), C.sizeof(pkg.capi.IsdfViewSelectRoutedInfo)] == [112, 144]
    p, s = pkg.capi.IsdfViewSelectRoutedParams(), pkg.capi.IsdfViewSelectParams()
    product_lib.isdf_view_select_routed_params_default(C.byref(p))
    product_lib.isdf_view_select_params_default(C.byref(s))
    assert (p.cost0, p.max_cost, p.path_cap, list(p.reserved)) == (1.0, np.inf, 0, [0] * 5) and bytes(p.select) == bytes(s)
    product_lib.isdf_view_select_routed_params_default(None)
    product_lib.isdf_view_select_routed_sizes(None)
    for n in ("isdf_view_select_routed_params_default", "isdf_view_select_routed_sizes", "isdf_view_select_routed", "isdf_view_select_routed_host"):
        assert n in pkg.capi.EXPORTED_SYMBOLS and hasattr(product_lib, n)


def test_bad_arguments_and_their_order(pkg, product_lib):
    occ, k, poses, _ = case_of(pkg, DIMS)
    w = kr.pack(k)
    b0, b1 = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(*(np.array(DIMS) * RES))
    d = (C.c_int32 * 3)(*DIMS)
    poses = np.ascontiguousarray(poses[:2])
    good = np.array([1.0, np.inf])
    outs = [np.full((2, 8), -7, dtype=np.int64), np.full((4, 4), -7, dtype=np.int64), np.full(2, -7, dtype=np.int64), np.full(len(w), 7, dtype=np.uint32),
            np.full(2, -7.0), np.full((4, 2), -7.0)]
    E = pkg.capi.ISDF_ERR_INVALID_ARG
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def call(cost=good, bits=w, n=2, out=outs, select=None, **kw):
        p = pkg.capi.IsdfViewSelectRoutedParams()
        product_lib.isdf_view_select_routed_params_default(C.byref(p))
        p.select.gain.max_range_m = 4.0
        for key, v in (select or {}).items():
            setattr(p.select, key, v)
        for key, v in kw.items():
            setattr(p, key, v)
        info = pkg.capi.IsdfViewSelectRoutedInfo()
        info.select.n_views = -1
        cc = None if cost is None else np.ascontiguousarray(cost, dtype=np.float64)
        rc_ = product_lib.isdf_view_select_routed_host(ptr(bits), ptr(occ), b0, b1, RES, d, C.byref(cam_of(pkg)), ptr(poses), n, ptr(cc), C.byref(p),
                                                       *[ptr(a) for a in out], C.byref(info))
        return rc_, info.select.n_views, (product_lib.isdf_last_error(None) or b"").decode()
    assert call(bits=None)[:2] == (E, -1)
    # the selection's own rules come first, in its order; then the routed ones
    rc_, nv, msg = call(select={"k_select": 0, "min_gain": 0}, cost0=0.0)
    assert (rc_, nv) == (E, -1) and "view select parameters" in msg, msg
    rc_, nv, msg = call(n=(1 << 24) + 1, select={"min_gain": 0})
    assert (rc_, nv) == (E, -1) and "2^24" in msg, msg
    rc_, nv, msg = call(select={"min_gain": 0}, cost0=0.0)
    assert (rc_, nv) == (E, -1) and "min_gain >= 1" in msg, msg
    for kw in ({"cost0": 0.0}, {"cost0": -1.0}, {"cost0": np.inf}, {"cost0": np.nan}, {"max_cost": np.nan}, {"max_cost": -0.5}, {"path_cap": -1}):
        rc_, nv, msg = call(cost=[np.nan, 1.0], **kw)
        assert (rc_, nv) == (E, -1) and "routed view select parameters" in msg, (kw, msg)
    assert call(path_cap=8)[:2] == (E, -1)                      # no paths without a field
    for bad in ([np.nan, 1.0], [1.0, -1e-300], [-np.inf, 0.0], None):
        rc_, nv, msg = call(cost=bad)
        assert (rc_, nv) == (E, -1) and "cost" in msg, (bad, msg)
    assert all((a == -7).all() for a in outs[:3] + outs[4:]) and (outs[3] == 7).all()
    with pytest.raises(pkg.engine.IsdfError) as e:
        pkg.engine.view_select_routed_host(w, occ, np.zeros(3), np.array(DIMS) * RES, RES, cam_of(pkg), poses, good, lib=product_lib, min_gain=0)
    assert e.value.code == E
    with pytest.raises(ValueError):
        pkg.engine.view_select_routed_host(w, occ, np.zeros(3), np.array(DIMS) * RES, RES, cam_of(pkg), poses, [1.0], lib=product_lib)
    assert call(max_cost=0.0)[:2] == (0, 2) and call(cost=[0.0, -0.0])[:2] == (0, 2)
    want = [a.copy() for a in outs] if call()[:2] == (0, 2) else None
    assert want is not None and want[4].tolist() == [1.0, np.inf]
    for skip in range(6):                                       # every output is nullable
        for a in outs:
            a[...] = 9
        assert call(out=[None if i == skip else a for i, a in enumerate(outs)])[:2] == (0, 2)
        assert all((a == 9).all() if i == skip else np.array_equal(a, b) for i, (a, b) in enumerate(zip(outs, want)))
