"""Builder for ISDF_SHAPE_PROGRAM: the construction kit of the reference's CSG class (src/utils/include/utils/Shape.hpp:1684-2317)
under the reference's own names.  Every function returns an expression tree; compile(tree) turns it into the instruction array
isdf_set_shape_program / Engine.set_shape_program take (include/isdf_accel.h lists the opcodes and the lines they restate).

Push-down rule: the device evaluates a flat list with ONE working point, so a transform that wraps a whole subtree is written in
front of every primitive of that subtree, outermost first - the order in which the reference's nested closures apply them
(translate(rotate(f, ...), o)(p) = f(R (p - o))).  Transforms are not multiplied together.  scale() also leaves the unary
"x min(factor)" behind its subtree (Shape.hpp:2015)."""
import ctypes as C
import math

import numpy as np

from . import capi

_PRIM, _DOMAIN, _UNARY, _BINARY = range(4)


class Node:
    def __init__(self, cls, op, params=(), children=()):
        self.cls, self.op, self.params, self.children = cls, op, [float(v) for v in params], list(children)


def _v3(v):
    v = [float(x) for x in v]
    assert len(v) == 3, "a 3-vector is expected"
    return v


# ---- primitives (Shape.hpp:1724-1994)
def sphere(radius, center=(0.0, 0.0, 0.0)): return Node(_PRIM, capi.OP_SPHERE, [radius] + _v3(center))
def capsule(a, b, radius): return Node(_PRIM, capi.OP_CAPSULE, _v3(a) + _v3(b) + [radius])
def box(size, center=(0.0, 0.0, 0.0)): return Node(_PRIM, capi.OP_BOX, _v3(size) + _v3(center))
def rounded_box(size, radius): return Node(_PRIM, capi.OP_ROUNDED_BOX, _v3(size) + [radius])
def wireframe_box(size, thickness): return Node(_PRIM, capi.OP_WIREFRAME_BOX, _v3(size) + [thickness])
def torus(r1, r2): return Node(_PRIM, capi.OP_TORUS, [r1, r2])
def cylinder(radius): return Node(_PRIM, capi.OP_CYLINDER, [radius])
def capped_cylinder(a, b, radius): return Node(_PRIM, capi.OP_CAPPED_CYLINDER, _v3(a) + _v3(b) + [radius])
def rounded_cylinder(ra, rb, h): return Node(_PRIM, capi.OP_ROUNDED_CYLINDER, [ra, rb, h])
def capped_cone(a, b, ra, rb): return Node(_PRIM, capi.OP_CAPPED_CONE, [ra, rb] + _v3(a) + _v3(b))
def rounded_cone(r1, r2, h): return Node(_PRIM, capi.OP_ROUNDED_CONE, [r1, r2, h])
def ellipsoid(size): return Node(_PRIM, capi.OP_ELLIPSOID, _v3(size))
def pyramid(h): return Node(_PRIM, capi.OP_PYRAMID, [h])
def tetrahedron(r): return Node(_PRIM, capi.OP_TETRAHEDRON, [r])
def octahedron(r): return Node(_PRIM, capi.OP_OCTAHEDRON, [r])
def dodecahedron(r): return Node(_PRIM, capi.OP_DODECAHEDRON, [r])
def icosahedron(r): return Node(_PRIM, capi.OP_ICOSAHEDRON, [r])


# ---- transforms of the working point (:1996-2059, :2198-2230)
def translate(other, offset): return Node(_DOMAIN, capi.OP_TRANSLATE, _v3(offset), [other])
def scale(other, factor): return Node(_DOMAIN, capi.OP_SCALE, _v3(factor), [other])
def rotate(other, angle, vector=(0.0, 0.0, 1.0)): return Node(_DOMAIN, capi.OP_ROTATE, [angle] + _v3(vector), [other])
def rotate_to(other, a, b): return Node(_DOMAIN, capi.OP_ROTATE_TO, _v3(a) + _v3(b), [other])     # resolved by the library, on the host
def twistOp(other, k): return Node(_DOMAIN, capi.OP_TWIST, [k], [other])
def bendOp(other, k): return Node(_DOMAIN, capi.OP_BEND, [k], [other])


# ---- values (:2061-2284).  Of the vector overloads only unionOp's and blendOp's fold: the vector differenceOp / intersectionOp
# of the reference return after their first operand, i.e. they are the binary forms.
def _fold(op, a, bs, k):
    for b in (bs if isinstance(bs, (list, tuple)) else [bs]):
        a = Node(_BINARY, op, [k], [a, b])
    return a


def unionOp(a, b, k=0.0): return _fold(capi.OP_UNION, a, b, k)
def blendOp(a, bs, k=0.5): return _fold(capi.OP_BLEND, a, bs, k)
def differenceOp(a, b, k=0.0): return Node(_BINARY, capi.OP_DIFFERENCE, [k], [a, b])
def intersectionOp(a, b, k=0.0): return Node(_BINARY, capi.OP_INTERSECTION, [k], [a, b])
def negateOp(other): return Node(_UNARY, capi.OP_NEGATE, [], [other])
def dilateOp(other, r): return Node(_UNARY, capi.OP_DILATE, [r], [other])
def erodeOp(other, r): return Node(_UNARY, capi.OP_ERODE, [r], [other])
def shellOp(other, thickness): return Node(_UNARY, capi.OP_SHELL, [thickness], [other])


def instructions(rows):
    """[(op, params), ...] -> the ctypes instruction array (no checks: what the library's validator is tested with)"""
    arr = (capi.IsdfShapeInstr * max(len(rows), 1))()
    for i, (op, params) in enumerate(rows):
        arr[i].op = int(op)
        for k, v in enumerate(params):
            arr[i].p[k] = float(v)
    arr._n = len(rows)
    return arr


def compile(tree):
    """The instruction array of an expression tree.  ValueError when it needs more than 64 instructions or a value stack
    deeper than 8."""
    rows = []
    depth = [0, 0]      # current, deepest

    def emit(node, transforms):
        if node.cls == _PRIM:
            rows.extend((t.op, t.params) for t in transforms)
            rows.append((node.op, node.params))
            depth[0] += 1
            depth[1] = max(depth[1], depth[0])
        elif node.cls == _DOMAIN:
            emit(node.children[0], transforms + [node])
            if node.op == capi.OP_SCALE:
                rows.append((capi.OP_MUL, [min(node.params)]))
        elif node.cls == _UNARY:
            emit(node.children[0], transforms)
            rows.append((node.op, node.params))
        else:
            emit(node.children[0], transforms)
            emit(node.children[1], transforms)
            rows.append((node.op, node.params))
            depth[0] -= 1
    emit(tree, [])
    if len(rows) > capi.PROGRAM_MAX_INSTR:
        raise ValueError(f"shape program: {len(rows)} instructions (at most {capi.PROGRAM_MAX_INSTR})")
    if depth[1] > capi.PROGRAM_MAX_DEPTH:
        raise ValueError(f"shape program: value stack {depth[1]} deep (at most {capi.PROGRAM_MAX_DEPTH})")
    return instructions(rows)


def _n(instr):
    return getattr(instr, "_n", len(instr))


def validate(instr, n=None):
    """(status, message) of the library's validator for an instruction array"""
    lib = capi.load_library()
    buf = C.create_string_buffer(256)
    rc = lib.isdf_shape_program_validate(instr, _n(instr) if n is None else n, buf, 256)
    return rc, buf.value.decode()


def eval_host(program, points, trans=None, rotate=None, want_grad=True):
    """(sdf[n], grad[n, 3]) of a program at body-frame points through isdf_shape_program_eval_host: the device's arithmetic in
    plain C++, no context and no GPU"""
    lib = capi.load_library()
    instr = compile(program) if isinstance(program, Node) else program
    dp = C.POINTER(C.c_double)
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    sdf = np.zeros(len(P)); grad = np.zeros((len(P), 3)) if want_grad else None
    tr = None if trans is None else np.ascontiguousarray(trans, dtype=np.float64).reshape(3)
    ro = None if rotate is None else np.ascontiguousarray(rotate, dtype=np.float64).reshape(9)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    rc = lib.isdf_shape_program_eval_host(instr, _n(instr), ptr(tr), ptr(ro), ptr(P), len(P), ptr(sdf), ptr(grad))
    if rc != 0:
        raise ValueError(f"isdf_shape_program_eval_host: status {rc}: {validate(instr)[1]}")
    return sdf, grad


def _mirrored_boxes(size, centre, axes):
    """box(size, centre) and its mirror images across the planes of `axes`: the classes that take |x| first (Table,
    WireframeBox) evaluate box_q at ||x| - c|, which is min(|x - c|, |x + c|) - and box_q grows with each of its arguments, so the
    class is the union of the mirrored boxes, value for value"""
    out = [list(centre)]
    for a in axes:
        if centre[a] != 0.0:
            out += [[-c[i] if i == a else c[i] for i in range(3)] for c in out]
    return [box(size, c) for c in out]


def reference_class(name):
    """The expression tree that restates a registered analytic class (sw_manager.hpp:74-123, and Ball) from the op library, with
    the class's constants: the link between programs and the kinds that are pinned against the reference's compiled classes."""
    X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    if name == "CSG":                                       # Shape.hpp:2289-2295
        f = intersectionOp(sphere(3.0), box((4.5, 4.5, 4.5)))
        c = cylinder(1.5)
        c4 = unionOp(unionOp(rotate_to(c, X, X), rotate_to(c, X, Y)), rotate_to(c, X, Z))
        return differenceOp(f, c4)
    if name == "Table":
        # two boxes a1..b1 and a2..b2 evaluated at (|x|, |y|, z) (:1366-1380): each with its mirror images
        parts = []
        for a, b in (((0.0, 0.0, 0.0), (3.5, 1.75, 0.7)), ((2.8, 1.05, 0.0), (3.5, 1.75, 2.8))):
            size = [b[i] - a[i] for i in range(3)]
            parts += _mirrored_boxes(size, [(a[i] + b[i]) / 2 for i in range(3)], (0, 1))
        return unionOp(parts[0], parts[1:])
    if name == "WireframeBox":
        # The class (:1072-1084) forms q from the SHIFTED point, the op library's wireframe_box (:1787) from p itself: the op is
        # another function and cannot restate the class.  The class is the frame's twelve edge bars: g(px, qy, qz) is a box of
        # size (sx + th, th, th) at (0, +-sy / 2, +-sz / 2), and so on for y and z.
        s, th = (1.8, 2.5, 3.5), 0.1
        parts = []
        for ax in range(3):
            size = [s[i] + th if i == ax else th for i in range(3)]
            centre = [0.0 if i == ax else s[i] / 2 for i in range(3)]
            parts += _mirrored_boxes(size, centre, [i for i in range(3) if i != ax])
        return unionOp(parts[0], parts[1:])
    if name == "SmoothDifference": return differenceOp(box((3.0, 3.0, 0.5)), sphere(1.0), 0.25)
    if name == "SmoothIntersection": return intersectionOp(box((3.0, 3.0, 0.5)), sphere(1.0), 0.25)
    if name == "SmoothIntersection_big": return intersectionOp(box((9.0, 9.0, 1.5)), sphere(3.0), 0.25)
    if name == "RoundedCone": return rounded_cone(1.5, 0.6, 4.5)
    if name == "CappedCone": return capped_cone((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 2.0, 0.8)
    if name == "TwistBox": return twistOp(box((2.0, 2.0, 2.0)), 3.14159265358979323846 / 6)
    if name == "BendBox": return bendOp(box((2.0, 2.0, 2.0)), 0.5)
    if name in ("Torus", "Torus_big"):                      # the class lies in the xz plane (:839-848), the op in xy (:1799)
        return rotate(torus(2.5 if name == "Torus" else 3.5, 0.3), math.pi / 2, X)
    if name == "Ball": return sphere(1.0)
    raise KeyError(f"no program restates {name!r} (BendLinear, Trefoil and Cappedtorus are not built from the op library)")


REFERENCE_CLASSES = ["CSG", "Table", "SmoothDifference", "SmoothIntersection", "SmoothIntersection_big", "RoundedCone", "CappedCone",
                     "WireframeBox", "TwistBox", "BendBox", "Torus", "Torus_big", "Ball"]
