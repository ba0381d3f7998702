"""Inputs of the map-product edge tests (isdf_generate_esdf / isdf_gather_points / isdf_set_pointcloud), shared by the host and the
device test files, in the style of tests/retime_cases.py: every case from fixed seeds, at the SMALLEST shape that takes a loop of
csrc/map_build.hip (or of build_bits_kernel, csrc/tile_sweep.hip) past its first trip, with the references of
tests/mapbuild_reference.py computed once per session.  Each case carries PRECONDITIONS: conditions on the reference alone that prove
the case reaches the loop it is meant for, so that an edit of a seed cannot quietly make a test vacuous.  The launch shapes they speak
of: edt_z_kernel 4096 x 256 threads = 16 384 wavefronts (one z-row each), edt_line_kernel 8192 x 256 = 2 097 152 threads (one voxel
each), build_bits_kernel 8192 wavefronts, pc_count_kernel 2048 x 256 = 524 288 threads (one point each), pc_threshold_kernel
4096 x 256 = 1 048 576 threads (one voxel each), gather_scan_kernel 256 chunks of 1024 occupancy words per batch."""
import numpy as np

import mapbuild_reference as mr

Z_ROW_WAVES = 4096 * 256 // 64
LINE_THREADS = 8192 * 256
PC_COUNT_THREADS = 2048 * 256
PC_THRESHOLD_THREADS = 4096 * 256
GATHER_CHUNK = 1024
SCAN_BATCH_WORDS = 256 * GATHER_CHUNK


def holds(pre):
    """assert every (text, bool) of a precondition list"""
    for text, ok in pre:
        assert ok, "precondition: " + text


# ---- EDT --------------------------------------------------------------------------------------------------------------------------
EDT_RES = 0.3
EDT_ORIGIN = (0.5, -1.0, 2.0)
E1_Z = (31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129)          # around the 32-bit words of a z-row and the 64 lanes of its wavefront
E2_SHAPES = ((1, 1, 4096), (1, 4096, 1), (4096, 1, 1))          # a full-length line along each axis
EDT_IDS = [f"E1-z{z}" for z in E1_Z] + ["E2-" + "x".join(map(str, s)) for s in E2_SHAPES] + ["E3-130x130x3", "E3-130x130x130", "E4-9x70x40"]


def _lone(shape, *voxels):
    occ = np.zeros(shape, dtype=np.uint8)
    for v in voxels:
        occ[v] = 1
    return occ


def _e1(z):
    shape = (3, 2, z)
    maps = {"first": _lone(shape, (0, 0, 0)), "last": _lone(shape, (2, 1, z - 1))}
    for v in ((1, 0, 31), (1, 0, 32), (1, 1, 63), (1, 1, 64)):             # the last bit of a word and the first bit of the next
        if v[2] < z:
            maps[f"bit{v[2]}"] = _lone(shape, v)
    maps["row"] = np.zeros(shape, dtype=np.uint8)
    maps["row"][1, 0, :] = 1                                               # one full z-row, every other row empty
    maps["random"] = (np.random.default_rng(1000 + z).uniform(size=shape) < 0.05).astype(np.uint8)
    return maps


def _e2(shape):
    n, ax = max(shape), int(np.argmax(shape))

    def at(*idx):
        return _lone(shape, *[tuple(i if a == ax else 0 for a in range(3)) for i in idx])
    return {"first": at(0), "middle": at(2047), "ends": at(0, n - 1)}


def _build_edt(synth, gid):
    if gid.startswith("E1-z"):
        return _e1(int(gid[4:]))
    if gid.startswith("E2-"):
        return _e2(tuple(int(v) for v in gid[3:].split("x")))
    if gid == "E3-130x130x3":
        return {"boxes": synth.random_box_map((130, 130, 3), res=EDT_RES, occupancy=0.05, seed=133, edge=(0.3, 1.5))}
    if gid == "E3-130x130x130":
        return {"lone": _lone((130, 130, 130), (0, 0, 0), (129, 5, 77), (64, 129, 64)),
                "boxes": synth.random_box_map((130, 130, 130), res=EDT_RES, occupancy=0.05, seed=130, edge=(0.3, 1.5))}
    if gid == "E4-9x70x40":
        shape = (9, 70, 40)
        plane = np.zeros(shape, dtype=np.uint8); plane[8, :, :] = 1         # eight empty y-z planes: "nothing" reaches the x pass
        row = np.zeros(shape, dtype=np.uint8); row[4, 35, :] = 1            # empty z-rows in every plane, empty planes but one
        return {"plane": plane, "row": row, "full": np.ones(shape, dtype=np.uint8), "empty": np.zeros(shape, dtype=np.uint8)}
    raise KeyError(gid)


_EDT, _D2 = {}, {}


def edt_maps(synth, gid):
    """name -> occupancy (uint8 [X][Y][Z]) of one group; all maps of a group share their shape (one Engine per group)."""
    if gid not in _EDT:
        _EDT[gid] = _build_edt(synth, gid)
    return _EDT[gid]


def edt_d2(synth, gid, name):
    """mapbuild_reference.exact_d2 of one map, computed once per session; treat as read-only."""
    if (gid, name) not in _D2:
        d2 = mr.exact_d2(edt_maps(synth, gid)[name])
        d2.setflags(write=False)
        _D2[gid, name] = d2
    return _D2[gid, name]


def edt_preconditions(synth, gid):
    maps = edt_maps(synth, gid)
    shape = next(iter(maps.values())).shape
    pre = [("the maps of a group share one shape", all(m.shape == shape for m in maps.values()))]

    def finite_max(name):
        d2 = edt_d2(synth, gid, name)
        return int(d2[d2 < mr.NONE].max())
    if gid.startswith("E1-"):
        z = shape[2]
        pre += [("the far corner of `first` looks across every word of its z-row", finite_max("first") == 4 + 1 + (z - 1) ** 2),
                ("... and that of `last` the other way", finite_max("last") == 4 + 1 + (z - 1) ** 2),
                ("`random` is neither empty nor full", 0 < int(maps["random"].sum()) < maps["random"].size),
                ("`row` leaves every other z-row empty", int(maps["row"].sum()) == z and finite_max("row") == 1 + 1)]
    elif gid.startswith("E2-"):
        pre += [("a full-length line: the largest squared distance is 4095^2", max(shape) == 4096 and finite_max("first") == 4095 ** 2),
                ("`ends` halves it", finite_max("ends") == 2047 ** 2)]
    elif gid.startswith("E3-"):
        pre += [("more z-rows than edt_z_kernel has wavefronts", shape[0] * shape[1] > Z_ROW_WAVES and 16900 > 16384),
                ("`boxes` is neither empty nor full", 0 < int(maps["boxes"].sum()) < maps["boxes"].size)]
        if gid == "E3-130x130x130":
            pre += [("more voxels than edt_line_kernel has threads", shape[0] * shape[1] * shape[2] > LINE_THREADS and 2197000 > 2097152),
                    ("more 64-voxel chunks than build_bits_kernel has wavefronts", shape[0] * shape[1] * ((shape[2] + 63) // 64) > 8192),
                    ("`lone` has distances in the ten thousands", finite_max("lone") == 17665)]
    elif gid.startswith("E4-"):
        pre += [("`plane`: eight planes without an occupied voxel", finite_max("plane") == 64 and int(maps["plane"][:8].sum()) == 0),
                ("`row`: one occupied z-row", int(maps["row"].sum()) == shape[2] and finite_max("row") == 4 ** 2 + 35 ** 2),
                ("`full` is 0 everywhere", not edt_d2(synth, gid, "full").any()),
                ("`empty` is `nothing here` everywhere", bool((edt_d2(synth, gid, "empty") == mr.NONE).all()))]
    return pre


# ---- gather -----------------------------------------------------------------------------------------------------------------------
GATHER_IDS = ["G1", "G2"]
GATHER_OFFSET = (0.4, -0.3, 0.2)
_GATHER, _WANT = {}, {}


def _build_gather(name):
    if name == "G1":        # 600 x 500 z-rows of one word: 300 000 words = 293 chunks, the last of 992 words, its last wave round of 32
        shape, res, bmin = (600, 500, 20), 0.25, np.zeros(3)
        occ = (np.random.default_rng(61).uniform(size=shape) < 0.01).astype(np.uint8)
        a, b = np.array([5.0, 5.0, 2.5]), np.array([148.0, 120.0, 2.5])
        way = [a + (b - a) * k / 7 for k in range(8)]
        nxt = b + (b - a) / np.linalg.norm(b - a)                          # 1 m on: overlaps the last box, only the new rim counts
        way += [nxt, nxt.copy(), np.array([-3.0, 140.0, 9.0])]             # the same point again: nothing; then one outside the map
        way = np.array(way)
        # reversed WITH the offset: the offset shifts a waypoint's own box only, so which neighbour is subtracted matters
        runs = [("plain", way, None), ("offset", way, GATHER_OFFSET), ("reversed", way[::-1].copy(), GATHER_OFFSET)]
        return dict(occ=occ, bmin=bmin, bmax=bmin + np.array(shape) * res, res=res, half=np.array([6.0, 5.0, 3.0]), runs=runs)
    if name == "G2":        # z-rows of two words, the second with 13 voxels and 19 padding bits; an origin that is no multiple of res
        shape, res, bmin = (70, 33, 45), EDT_RES, np.array(EDT_ORIGIN)
        rng = np.random.default_rng(62)
        occ = (rng.uniform(size=shape) < 0.03).astype(np.uint8)
        ext = np.array(shape) * res
        way = bmin + rng.uniform(0.1, 0.9, (5, 3)) * ext
        # a voxel whose 3 x 3 x 3 neighbourhood is free: a box of +-0.2 m about its centre covers exactly that
        free = np.argwhere(_box_sum3(occ)[1:-1, 1:-1, 1:-1] == 0) + 1
        lonely = (free[len(free) // 2] + 0.5) * res + bmin
        runs = [("plain", way, None), ("offset", way, GATHER_OFFSET), ("nothing", lonely[None, :], None)]
        halves = {"nothing": np.array([0.2, 0.2, 0.2])}
        return dict(occ=occ, bmin=bmin, bmax=bmin + ext, res=res, half=np.array([1.5, 1.2, 1.0]), halves=halves, runs=runs)
    raise KeyError(name)


def _box_sum3(occ):
    """the number of occupied voxels in the 3 x 3 x 3 box about every voxel (the border: about what exists of it)"""
    s = occ.astype(np.int64)
    for ax in range(3):
        p = np.pad(s, [(1, 1) if a == ax else (0, 0) for a in range(3)])
        n = s.shape[ax]
        s = sum(np.take(p, np.arange(k, k + n), axis=ax) for k in range(3))
    return s


def gather_case(name):
    if name not in _GATHER:
        _GATHER[name] = _build_gather(name)
    return _GATHER[name]


def gather_half(cs, run):
    return cs.get("halves", {}).get(run, cs["half"])


def gather_want(name, run):
    """(indices int64 [M][3], centres float64 [M][3]) of one run, once per session"""
    if (name, run) not in _WANT:
        cs = gather_case(name)
        way, off = next((w, o) for r, w, o in cs["runs"] if r == run)
        I = mr.gather_indices(cs["occ"], cs["bmin"], cs["bmax"], cs["res"], way, gather_half(cs, run), off)
        _WANT[name, run] = (I, (I.astype(np.float64) + 0.5) * cs["res"] + cs["bmin"])
    return _WANT[name, run]


def gather_preconditions(name):
    cs = gather_case(name)
    X, Y, Z = cs["occ"].shape
    zw = (Z + 31) // 32
    n_words = X * Y * zw
    pre = []
    if name == "G1":
        last_chunk = (n_words - 1) // GATHER_CHUNK * GATHER_CHUNK
        pre += [("293 chunks, the last of 992 words and a last wave round of 32", zw == 1 and n_words == 300000 and (n_words + 1023) // 1024 == 293
                 and n_words - last_chunk == 992 and 992 % 64 == 32)]
        for run in ("plain", "offset", "reversed"):
            I = gather_want(name, run)[0]
            word = (I[:, 0] * Y + I[:, 1]) * zw + (I[:, 2] >> 5)
            pre += [(f"{run}: a voxel past the first scan batch of 256 chunks", bool((word >= SCAN_BATCH_WORDS).any())),
                    (f"{run}: a voxel inside the first scan batch", bool((word < SCAN_BATCH_WORDS).any())),
                    (f"{run}: a voxel in the last, partial chunk", bool((word >= last_chunk).any())),
                    (f"{run}: M > 1000", I.shape[0] > 1000)]
        as_set = {run: set(map(tuple, gather_want(name, run)[0].tolist())) for run in ("plain", "offset", "reversed")}
        pre += [("the offset moves the set", as_set["plain"] != as_set["offset"]),
                ("the reversed order lacks voxels of the call before it: a mark that survived would show", len(as_set["offset"] - as_set["reversed"]) > 0)]
    else:
        pre += [("two words per z-row, 13 voxels in the second", zw == 2 and Z - 32 == 13),
                ("plain: points in both words of a row", len(set((gather_want(name, "plain")[0][:, 2] >> 5).tolist())) == 2),
                ("plain and offset: something found", min(gather_want(name, r)[0].shape[0] for r in ("plain", "offset")) > 0),
                ("nothing: the reference is empty", gather_want(name, "nothing")[0].shape[0] == 0)]
    return pre


# ---- point cloud ------------------------------------------------------------------------------------------------------------------
_CLOUD = {}


def _build_p1():
    """600 000 points whose coordinates are multiples of 1/8 (exact in float32; half of them on voxel faces of the 0.25 m grid)."""
    rng = np.random.default_rng(71)
    bmin, bmax, res, thr = np.zeros(3), np.array([32.0, 32.0, 17.5]), 0.25, 3
    dims = np.array([128, 128, 70])
    top8 = (bmax * 8).astype(np.int64)                                      # the box in eighths of a metre
    n_total, n_out, n_face, n_two, n_three, n_late = 600000, 12000, 5000, 2000, 2000, 200
    n_rand = n_total - n_out - 6 * n_face - 2 * n_two - 3 * n_three - 3 * n_late

    def inside(n):
        return np.stack([rng.integers(0, top8[a] + 1, n) for a in range(3)], axis=1)
    parts = [inside(n_rand)]
    for a in range(3):                                                      # the six faces; a point ON a bmax face is in the last voxel
        for v in (0, top8[a]):
            f = inside(n_face); f[:, a] = v
            parts.append(f)
    out = inside(n_out)                                                     # 2 % outside, by 1/8 m .. 5 m beyond one face: voxel (0,0,0)
    ax, far, side = rng.integers(0, 3, n_out), rng.integers(1, 41, n_out), rng.integers(0, 2, n_out)
    out[np.arange(n_out), ax] = np.where(side == 1, top8[ax] + far, -far)
    parts.append(out)
    base = np.concatenate(parts)
    ins = np.all((base >= 0) & (base <= top8), axis=1)
    idx = np.minimum(base // 2, dims - 1)                                   # 2 eighths per voxel
    idx[~ins] = 0
    counts = np.zeros(tuple(dims), dtype=np.int64)
    np.add.at(counts, (idx[:, 0], idx[:, 1], idx[:, 2]), 1)
    # voxels nothing has hit yet: some get exactly 2 points, some exactly 3, some 2 early and their third at the end of the cloud
    free = np.flatnonzero(counts.ravel() == 0)
    chosen = np.stack(np.unravel_index(rng.choice(free, n_two + n_three + n_late, replace=False), tuple(dims)), axis=1)
    two, three, late = chosen[:n_two], chosen[n_two:n_two + n_three], chosen[n_two + n_three:]

    def into(vox, k):
        v = np.repeat(vox, k, axis=0)
        return 2 * v + rng.integers(0, 2, v.shape)
    body = np.concatenate([base, into(two, 2), into(three, 3)])
    body = body[rng.permutation(body.shape[0])]                            # every kind of point on both trips of pc_count_kernel
    P8 = np.concatenate([body[:100000], into(late, 2), body[100000:], into(late, 1)])
    P = (P8.astype(np.float64) / 8).astype(np.float32)
    way = np.array([[8.0, 8.0, 8.0], [9.5, 8.5, 8.0], [30.0, 30.5, 16.0]])  # two overlapping boxes and one cut by the map's corner
    return dict(P=P, bmin=bmin, bmax=bmax, res=res, thr=thr, dims=tuple(int(d) for d in dims), two=two, three=three, late=late,
                way=way, half=np.array([3.0, 2.5, 2.0]))


def _build_p2():
    rng = np.random.default_rng(72)
    bmin, bmax = np.array([-1.0, 0.5, 2.0]), np.array([3.0, 4.0, 5.0])     # 8 x 7 x 6 voxels of 0.5 m
    P = (bmin + rng.uniform(0, 1, (1000, 3)) * (bmax - bmin)).astype(np.float32)
    return dict(P=P, bmin=bmin, bmax=bmax, res=0.5, thr=0, dims=(8, 7, 6))


def cloud_case(name):
    if name not in _CLOUD:
        _CLOUD[name] = _build_p1() if name == "P1" else _build_p2()
    return _CLOUD[name]


def cloud_want(orc, name):
    """(occupancy, bmin, bmax) of oracle/pyoracle.py::pointcloud_to_occupancy, once per session"""
    cs = cloud_case(name)
    if "want" not in cs:
        cs["want"] = orc.pointcloud_to_occupancy(cs["P"], cs["res"], cs["thr"], bmin=cs["bmin"], bmax=cs["bmax"])
    return cs["want"]


def cloud_preconditions(orc, name):
    cs = cloud_case(name)
    occ = cloud_want(orc, name)[0]
    if name == "P2":
        return [("threshold 0: every voxel is occupied", occ.shape == cs["dims"] and bool(occ.all()))]
    P, n1 = cs["P"], PC_COUNT_THREADS

    def ref(points, thr):
        return orc.pointcloud_to_occupancy(points, cs["res"], thr, bmin=cs["bmin"], bmax=cs["bmax"])[0]
    first3, first2 = ref(P[:n1], 3), ref(P[:n1], 2)
    third_late = (occ == 1) & (first3 == 0) & (first2 == 1)                 # exactly 2 among the first 524 288 points, >= 3 in all
    flat = occ.ravel()
    t = tuple(cs["two"].T), tuple(cs["three"].T), tuple(cs["late"].T)
    return [("1 146 880 voxels of 0.25 m", occ.shape == cs["dims"] == (128, 128, 70) and occ.size > PC_THRESHOLD_THREADS),
            ("more points than pc_count_kernel has threads", P.shape == (600000, 3) and P.shape[0] > n1 and P.dtype == np.float32),
            ("every coordinate is a multiple of 1/8", bool(np.all(P.astype(np.float64) * 8 == np.round(P.astype(np.float64) * 8)))),
            ("the first 524 288 points alone give another occupancy", not np.array_equal(first3, occ)),
            ("at least 100 voxels go from 2 to 3 past point 524 288", int(third_late.sum()) >= 100 and bool(third_late[t[2]].all())),
            ("voxels with exactly 2 points stay free, with exactly 3 are occupied", not occ[t[0]].any() and bool(occ[t[1]].all())
             and bool(ref(P, 2)[t[0]].all()) and not ref(P, 4)[t[1]].any()),
            ("occupied voxels past pc_threshold_kernel's first trip", bool(flat[PC_THRESHOLD_THREADS:].any())),
            ("free voxels past pc_threshold_kernel's first trip", not flat[PC_THRESHOLD_THREADS:].all()),
            ("the points outside the box pile up in voxel (0, 0, 0)", occ[0, 0, 0] == 1),
            ("neither empty nor full", 0 < int(occ.sum()) < occ.size)]
