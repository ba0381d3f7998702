"""What the trajectory tools (isdf_traj_limits*, isdf_traj_sample*, isdf_traj_retime*, isdf_traj_realloc*) say before they touch a
device, and in which order: arguments, durations held on the host and parameters first, the ctx after them.  Every call passes a
null ctx, so the message is read through isdf_last_error(NULL) and no test needs a GPU.  Return codes and messages are literals."""
import ctypes as C

import numpy as np
import pytest

INVALID = -1            # ISDF_ERR_INVALID_ARG
RETIME_MAX = 1 << 20    # ISDF_TRAJ_RETIME_MAX_PIECES
REALLOC_MAX_N = 400     # ISDF_TRAJ_REALLOC_MAX_N

LIM_NULL = b"trajectory limits: null trajectory"
LIM_DUR = b"trajectory limits: a duration is not positive and finite"
LIM_CTX = b"trajectory limits: null ctx"
SMP_ARG = b"trajectory sample: null argument"
SMP_CTX = b"trajectory sample: null ctx"
RT_NULL = b"trajectory retime: null trajectory"
RT_OUT = b"trajectory retime: null output"
RT_DUR = b"trajectory retime: a duration is not positive and finite"
RT_PAR = b"trajectory retime: s_lo must be positive and finite, s_hi finite and above it, ladder 2..64, rounds 1..4"
RT_BATCH = b"trajectory retime: no clearance check in the batch form"
RT_CAP = b"trajectory retime: B x ladder x N above ISDF_TRAJ_RETIME_MAX_PIECES"
RT_CTX = b"trajectory retime: null ctx"
RA_NULL = b"trajectory realloc: null argument, B < 1 or N < 1"
RA_DUR = b"trajectory realloc: a duration is not positive and finite"
RA_PAR = b"trajectory realloc: rounds 1..16, headroom finite and >= 0, f_max finite and above 1"
RA_BATCH = b"trajectory realloc: no clearance check in the batch form"
RA_CAP = b"trajectory realloc: N above ISDF_TRAJ_REALLOC_MAX_N on the device (the host form takes any N)"
RA_OVER = b"trajectory realloc: an output overlaps an input or the other output"
RA_CTX = b"trajectory realloc: null ctx"

BAD_DURATIONS = {"zero": 0.0, "negative": -1.0, "inf": float("inf"), "nan": float("nan")}
DP = C.POINTER(C.c_double)


def _p(a):
    return None if a is None else a.ctypes.data_as(DP)


class Arrays:
    """B trajectories of N pieces: durations of 1, zero coefficients, ends, waypoints and room for the results."""

    def __init__(self, B, N, bad=None):
        self.B, self.N = B, N
        self.T = np.ones(B * N)
        if bad is not None:
            self.T[-1] = bad                    # the last duration of the last trajectory: the scan has to reach it
        self.Cc = np.zeros(18 * B * N)
        self.head, self.tail = np.zeros(9 * B), np.zeros(9 * B)
        self.Q = np.zeros(3 * B * max(N - 1, 1))
        self.To, self.Co = np.zeros(B * N), np.zeros(18 * B * N)
        self.t, self.rows = np.zeros(2), np.zeros(2 * 20)


def _retime_params(capi, lib, **kw):
    p = capi.IsdfTrajRetimeParams()
    lib.isdf_traj_retime_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _realloc_params(capi, lib, **kw):
    p = capi.IsdfTrajReallocParams()
    lib.isdf_traj_realloc_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- the calls: every one with a null ctx.  form: "single", "batch" or "device" (B is 1 but for "batch")
def limits(lib, form, a, T="T", Cc="Cc", N=None):
    N = a.N if N is None else N
    T, Cc = _p(getattr(a, T, None)), _p(getattr(a, Cc, None))
    if form == "batch":
        return lib.isdf_traj_limits_batch(None, a.B, N, T, Cc, None, None, None)
    if form == "device":
        return lib.isdf_traj_limits_device(None, N, C.cast(T, C.c_void_p), C.cast(Cc, C.c_void_p), None, None, None, None)
    return lib.isdf_traj_limits(None, N, T, Cc, None, None, None)


def sample(lib, form, a, T="T", Cc="Cc", N=None, n=2):
    N = a.N if N is None else N
    T, Cc = _p(getattr(a, T, None)), _p(getattr(a, Cc, None))
    if form == "device":
        return lib.isdf_traj_sample_device(None, N, C.cast(T, C.c_void_p), C.cast(Cc, C.c_void_p), n, C.cast(_p(a.t), C.c_void_p),
                                           C.cast(_p(a.rows), C.c_void_p), None)
    return lib.isdf_traj_sample(None, N, T, Cc, n, _p(a.t), _p(a.rows))


def retime(lib, form, a, p=None, T="T", N=None, To="To"):
    N = a.N if N is None else N
    T, Cc, To, Co = _p(getattr(a, T, None)), _p(a.Cc), _p(getattr(a, To, None)), _p(a.Co)
    pp = None if p is None else C.byref(p)
    if form == "batch":
        return lib.isdf_traj_retime_batch(None, a.B, N, T, Cc, pp, To, Co, None)
    if form == "device":
        v = [C.cast(x, C.c_void_p) for x in (T, Cc, To, Co)]
        return lib.isdf_traj_retime_device(None, N, v[0], v[1], pp, v[2], v[3], None, None)
    return lib.isdf_traj_retime(None, N, T, Cc, pp, To, Co, None)


def realloc(lib, form, a, p=None, T="T", N=None, To="To"):
    N = a.N if N is None else N
    T, To = _p(getattr(a, T, None)), _p(getattr(a, To, None))
    h, t, q, Co = _p(a.head), _p(a.tail), _p(a.Q), _p(a.Co)
    pp = None if p is None else C.byref(p)
    if form == "batch":
        return lib.isdf_traj_realloc_batch(None, a.B, N, h, t, q, T, pp, To, Co, None)
    if form == "device":
        v = [C.cast(x, C.c_void_p) for x in (h, t, q, T, To, Co)]
        return lib.isdf_traj_realloc_device(None, N, v[0], v[1], v[2], v[3], pp, v[4], v[5], None, None)
    return lib.isdf_traj_realloc(None, N, h, t, q, T, pp, To, Co, None)


def _said(lib, rc, want_rc, want_msg):
    assert rc == want_rc
    assert lib.isdf_last_error(None) == want_msg


def _arrays(form, N=2, bad=None):
    return Arrays(3 if form == "batch" else 1, N, bad)


HOST_FORMS = ("single", "batch")
ALL_FORMS = ("single", "batch", "device")
# tool, call, forms that hold the durations on the host, (null trajectory, bad duration, null ctx)
TOOLS = {
    "limits": (limits, ALL_FORMS, (LIM_NULL, LIM_DUR, LIM_CTX)),
    "sample": (sample, ("single", "device"), (LIM_NULL, LIM_DUR, SMP_CTX)),      # the sampler shares the report's trajectory check
    "retime": (retime, ALL_FORMS, (RT_NULL, RT_DUR, RT_CTX)),
    "realloc": (realloc, ALL_FORMS, (RA_NULL, RA_DUR, RA_CTX)),
}
TOOL_FORMS = [(tool, form) for tool, (_, forms, _) in TOOLS.items() for form in forms]
TOOL_HOST_FORMS = [(tool, form) for tool, form in TOOL_FORMS if form != "device"]


@pytest.mark.parametrize("tool,form", TOOL_FORMS)
def test_null_trajectory(product_lib, tool, form):
    call, _, (null_msg, _, _) = TOOLS[tool]
    want = SMP_ARG if (tool, form) == ("sample", "device") else null_msg
    _said(product_lib, call(product_lib, form, _arrays(form), T="none"), INVALID, want)


@pytest.mark.parametrize("tool,form", TOOL_FORMS)
def test_no_pieces(product_lib, tool, form):
    call, _, (null_msg, _, _) = TOOLS[tool]
    want = SMP_ARG if (tool, form) == ("sample", "device") else null_msg
    _said(product_lib, call(product_lib, form, _arrays(form), N=0), INVALID, want)


@pytest.mark.parametrize("bad", sorted(BAD_DURATIONS))
@pytest.mark.parametrize("tool,form", TOOL_HOST_FORMS)
def test_bad_duration(product_lib, tool, form, bad):
    call, _, (_, dur_msg, _) = TOOLS[tool]
    _said(product_lib, call(product_lib, form, _arrays(form, bad=BAD_DURATIONS[bad])), INVALID, dur_msg)


@pytest.mark.parametrize("tool,form", TOOL_FORMS)
def test_null_ctx_comes_last(product_lib, tool, form):
    """Valid arguments: only now is the ctx looked at.  The device forms judge their durations on the device, so after the ctx."""
    call, _, (_, _, ctx_msg) = TOOLS[tool]
    _said(product_lib, call(product_lib, form, _arrays(form)), INVALID, ctx_msg)


def test_sample_own_arguments(product_lib):
    a = _arrays("single")
    _said(product_lib, sample(product_lib, "single", a, n=-1), INVALID, SMP_ARG)
    _said(product_lib, sample(product_lib, "single", a, T="none", n=-1), INVALID, SMP_ARG)      # its own arguments before the trajectory
    _said(product_lib, sample(product_lib, "single", a, n=0), INVALID, SMP_CTX)                 # no stamps: still no ctx


@pytest.mark.parametrize("form", ALL_FORMS)
@pytest.mark.parametrize("field,value", [("ladder", 1), ("rounds", 5)])
def test_retime_params(pkg, product_lib, form, field, value):
    p = _retime_params(pkg.capi, product_lib, **{field: value})
    _said(product_lib, retime(product_lib, form, _arrays(form), p), INVALID, RT_PAR)


def test_retime_batch_refuses_check(pkg, product_lib):
    p = _retime_params(pkg.capi, product_lib, check=1)
    _said(product_lib, retime(product_lib, "batch", _arrays("batch"), p), INVALID, RT_BATCH)
    for form in ("single", "device"):                   # the other forms take it and go on to the ctx
        _said(product_lib, retime(product_lib, form, _arrays(form), p), INVALID, RT_CTX)


def test_retime_candidate_cap(pkg, product_lib):
    p = _retime_params(pkg.capi, product_lib, ladder=64)
    _said(product_lib, retime(product_lib, "batch", Arrays(RETIME_MAX // 64 + 1, 1), p), INVALID, RT_CAP)
    _said(product_lib, retime(product_lib, "batch", Arrays(RETIME_MAX // 64, 1), p), INVALID, RT_CTX)       # at the cap: taken


@pytest.mark.parametrize("form", ALL_FORMS)
def test_retime_order(pkg, product_lib, form):
    p = _retime_params(pkg.capi, product_lib, ladder=1, rounds=5)
    _said(product_lib, retime(product_lib, form, _arrays(form), p, T="none"), INVALID, RT_NULL)     # the trajectory before the parameters
    _said(product_lib, retime(product_lib, form, _arrays(form), p, To="none"), INVALID, RT_OUT)     # and the outputs
    if form != "device":
        _said(product_lib, retime(product_lib, form, _arrays(form, bad=0.0), p), INVALID, RT_PAR)   # the parameters before the durations


@pytest.mark.parametrize("form", ALL_FORMS)
@pytest.mark.parametrize("field,value", [("rounds", 0), ("f_max", 1.0)])
def test_realloc_params(pkg, product_lib, form, field, value):
    p = _realloc_params(pkg.capi, product_lib, **{field: value})
    _said(product_lib, realloc(product_lib, form, _arrays(form), p), INVALID, RA_PAR)


def test_realloc_batch_refuses_check(pkg, product_lib):
    p = _realloc_params(pkg.capi, product_lib, check=1)
    _said(product_lib, realloc(product_lib, "batch", _arrays("batch"), p), INVALID, RA_BATCH)
    for form in ("single", "device"):
        _said(product_lib, realloc(product_lib, form, _arrays(form), p), INVALID, RA_CTX)


@pytest.mark.parametrize("form", ALL_FORMS)
def test_realloc_piece_cap(product_lib, form):
    _said(product_lib, realloc(product_lib, form, _arrays(form, N=REALLOC_MAX_N + 1)), INVALID, RA_CAP)
    _said(product_lib, realloc(product_lib, form, _arrays(form, N=REALLOC_MAX_N)), INVALID, RA_CTX)


@pytest.mark.parametrize("form", ALL_FORMS)
def test_realloc_output_aliases_input(product_lib, form):
    _said(product_lib, realloc(product_lib, form, _arrays(form), To="T"), INVALID, RA_OVER)


@pytest.mark.parametrize("form", ALL_FORMS)
def test_realloc_order(pkg, product_lib, form):
    p = _realloc_params(pkg.capi, product_lib, rounds=0, f_max=1.0)
    _said(product_lib, realloc(product_lib, form, _arrays(form), p, T="none"), INVALID, RA_NULL)    # the trajectory before the parameters
    if form != "device":
        _said(product_lib, realloc(product_lib, form, _arrays(form, bad=0.0), p), INVALID, RA_PAR)  # the parameters before the durations


def test_literals_are_the_package_constants(pkg):
    capi = pkg.capi
    assert (INVALID, RETIME_MAX, REALLOC_MAX_N) == (capi.ISDF_ERR_INVALID_ARG, capi.TRAJ_RETIME_MAX_PIECES, capi.TRAJ_REALLOC_MAX_N)
