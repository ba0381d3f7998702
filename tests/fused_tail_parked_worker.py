"""Child process of tests/test_gpu_fused_tail_parked.py: every case of that file once, results into one .npz.  Run once as it is
(the fused launch) and once with ISDF_NO_FUSE=1 (read at isdf_create): the parent compares the two files byte for byte.

The cases sit at the edges of the fused tail's parked values (tile_sweep.hip, tail_piece): a tail thread keeps the basis rows,
jerk and snap of its sample in its own row of the partial-sum array while it waits for the collision sums.  K + 1 = 2 is the first
two lanes of a wavefront, 63 / 64 / 65 end below, on and past the first wavefront's last lane, 128 is a full pass of the tail's
threads and the largest step that still fuses; N = 1 and 3 give one tail workgroup and several."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K1S = (2, 63, 64, 65, 128)
NS = (1, 3)
RES = 0.5
MAP_SHAPE = (64, 64, 64)


def world(pkg):
    occ = pkg.synth.random_box_map(MAP_SHAPE, res=RES, occupancy=0.12, seed=3, edge=(1.0, 3.0))
    return occ, pkg.synth.esdf_from_occupancy(occ, RES)


def empty_esdf():
    return np.full(MAP_SHAPE, 100.0, dtype=np.float32)       # nothing within reach of any sample


def trajectory(pkg, occ, N, seed):
    ext = np.array(MAP_SHAPE) * RES
    T, Cf = pkg.synth.random_trajectory(ext, N, seed=seed, piece_T=1.5, margin=4.0, occ=occ, res=RES, jitter=0.5)
    return T, pkg.synth.colmajor(Cf)


def config(pkg, K1, enable_dyn=1):
    return pkg.synth.default_config(pkg.capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=K1 - 1, safety_hor=0.5, enable_dyn=enable_dyn)


def shape(pkg, name):
    if name == "Box":
        return pkg.synth.make_shape("Box", params=(1.2, 0.4, 0.3), grad_mode=pkg.capi.GRAD_CENTRAL)
    return pkg.synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6))


def cases():
    """name -> (map, K + 1, N, enable_dyn, shape, trajectory seed)"""
    out = {}
    for K1 in K1S:
        for N in NS:
            out[f"boxes_K1_{K1}_N{N}"] = ("boxes", K1, N, 1, "Box", 11)
            out[f"empty_K1_{K1}_N{N}"] = ("empty", K1, N, 1, "Box", 11)
            out[f"nodyn_K1_{K1}_N{N}"] = ("boxes", K1, N, 0, "Box", 11)
    out["cone_K1_65_N3"] = ("boxes", 65, 3, 1, "RoundedCone", 11)
    return out


def flat(cost, gT, gC):
    return np.concatenate([[cost], gT, gC])          # the step's 1 + 19 N outputs


def main():
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    occ, esdf = world(pkg)
    grids = {"boxes": esdf, "empty": empty_esdf()}
    res = {}
    for name, (m, K1, N, dyn, shp, seed) in cases().items():
        eng = pkg.Engine(config(pkg, K1, dyn))
        eng.set_grid(grids[m], (0, 0, 0), RES, capi.GRID_ESDF)
        eng.set_shape(shape(pkg, shp))
        T, cm = trajectory(pkg, occ, N, seed)
        res[name] = flat(*eng.eval_single(T, cm))
        res[name + "/host_path"] = np.array(eng.host_path())
        res[name + "/grad_pairs"] = np.array(eng.stats()["grad_pairs"])
        eng.close()
    # one engine, trajectory A, then B, then A again
    eng = pkg.Engine(config(pkg, 65))
    eng.set_grid(esdf, (0, 0, 0), RES, capi.GRID_ESDF)
    eng.set_shape(shape(pkg, "Box"))
    for tag, seed in (("A1", 11), ("B", 12), ("A2", 11)):
        res["aba_" + tag] = flat(*eng.eval_single(*trajectory(pkg, occ, 3, seed)))
    eng.close()
    np.savez(sys.argv[1], **res)
    print("RESULT ok")


if __name__ == "__main__":
    main()
