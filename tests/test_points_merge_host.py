"""Host side of the report merge and the checked optimiser (isdf_points_merge_check, isdf_refine_params_default,
isdf_optimize_lbfgs_checked): what needs no device - the parameter defaults, the argument checks that come before the ctx is looked
at, the struct layouts against the header, the exported symbols."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refine_params_defaults(pkg, product_lib):
    capi = pkg.capi
    p = capi.IsdfRefineParams()
    p.max_rounds = 99; p.mode = 7; p.margin = 3.0; p.below = 2.0
    product_lib.isdf_refine_params_default(C.byref(p))
    # negative margin = cfg.safety_hor of the ctx; negative below = every kept row; the collision term's own query
    assert (p.max_rounds, p.mode, p.margin, p.below) == (4, capi.SWEPT_FIELD_PLANNER, -1.0, -1.0)
    product_lib.isdf_refine_params_default(None)        # tolerated


def test_bad_arguments_are_refused_without_a_device(pkg, product_lib):
    capi, L = pkg.capi, product_lib
    dp = C.POINTER(C.c_double)
    info = capi.IsdfPointsMergeInfo()
    # ---- the merge: `below` is checked before the ctx, then the ctx
    assert L.isdf_points_merge_check(None, -1.0, C.byref(info)) == capi.ISDF_ERR_INVALID_ARG
    assert b"ctx" in L.isdf_last_error(None)
    assert L.isdf_points_merge_check(None, 0.25, None) == capi.ISDF_ERR_INVALID_ARG
    assert b"ctx" in L.isdf_last_error(None)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.isdf_points_merge_check(None, bad, C.byref(info)) == capi.ISDF_ERR_INVALID_ARG
        assert b"below" in L.isdf_last_error(None), L.isdf_last_error(None)
    # ---- the driver
    x = np.zeros(7)
    lp = capi.IsdfLbfgsParams()
    L.isdf_lbfgs_params_default(C.byref(lp))
    res = capi.IsdfRefineResult()

    def params(**kw):
        q = capi.IsdfRefineParams()
        L.isdf_refine_params_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    call = lambda q: L.isdf_optimize_lbfgs_checked(None, x.ctypes.data_as(dp), x.size, C.byref(lp), None if q is None else C.byref(q), C.byref(res))     # noqa: E731
    assert call(None) == capi.ISDF_ERR_INVALID_ARG and b"ctx" in L.isdf_last_error(None)
    assert call(params()) == capi.ISDF_ERR_INVALID_ARG and b"ctx" in L.isdf_last_error(None)
    for kw, word in ((dict(max_rounds=0), b"max_rounds"), (dict(max_rounds=-2), b"max_rounds"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(below=float("nan")), b"below"), (dict(below=float("inf")), b"below"), (dict(margin=float("nan")), b"margin")):
        assert call(params(**kw)) == capi.ISDF_ERR_INVALID_ARG, kw
        assert word in L.isdf_last_error(None), (kw, L.isdf_last_error(None))


def test_struct_layouts_match_header(pkg):
    capi = pkg.capi
    structs = {"isdf_points_merge_info": capi.IsdfPointsMergeInfo, "isdf_refine_params": capi.IsdfRefineParams,
               "isdf_refine_result": capi.IsdfRefineResult}
    lines = []
    for cname, S in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _ in S._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    others = ["isdf_config", "isdf_shape", "isdf_stats", "isdf_lbfgs_params", "isdf_lbfgs_result", "isdf_traj_check_params", "isdf_traj_check_info"]
    for cname in others:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
    lines.append('printf("%d\\n", ISDF_ABI_VERSION);')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"isdf_accel.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    want = []
    for S in structs.values():
        want.append(C.sizeof(S))
        want += [getattr(S, f).offset for f, _ in S._fields_]
    # the existing ABI is unchanged
    want += [C.sizeof(S) for S in (capi.IsdfConfig, capi.IsdfShape, capi.IsdfStats, capi.IsdfLbfgsParams, capi.IsdfLbfgsResult,
                                   capi.IsdfTrajCheckParams, capi.IsdfTrajCheckInfo)]
    want.append(1)
    assert out == want
    assert [f for f, _ in capi.IsdfPointsMergeInfo._fields_] == ["M_before", "M_after", "n_rows", "n_added", "n_duplicate", "n_outside",
                                                                 "reserved", "merge_ms"]
    assert [f for f, _ in capi.IsdfRefineParams._fields_] == ["max_rounds", "mode", "margin", "below"]
    assert [f for f, _ in capi.IsdfRefineResult._fields_] == ["rounds", "clear", "stalled", "reserved", "M_round", "last_opt", "last_check"]


def test_entry_points_are_exported(pkg, product_lib):
    for n in ("isdf_points_merge_check", "isdf_refine_params_default", "isdf_optimize_lbfgs_checked"):
        assert n in pkg.capi.EXPORTED_SYMBOLS and hasattr(product_lib, n)
    assert hasattr(pkg.Engine, "points_merge_check") and hasattr(pkg.Engine, "optimize_lbfgs_checked")
