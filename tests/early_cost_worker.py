"""Child process of tests/test_gpu_early_cost.py: every case of that file once, results into one .npz.  Run once as it is (the fused
launch) and once with ISDF_NO_FUSE=1 (read at isdf_create): the parent compares the two files byte for byte.

A fused single-GPU step whose results stay on the device publishes each piece's cost as soon as the collision sums of its samples
are taken (tile_sweep.hip, tail_piece: `early_cost`); the tail's third wavefront adds the samples' cost terms up in the shape of the
late column sums - TL_GROUPS = 6 partial sums over rows g, g + 6, ..., then those in order.  Only isdf_eval_device takes that path,
so every case is evaluated through it; the host-pointer call that follows on the same engine keeps the late order (its rows cross
PCIe and are released before the cost), must give the same bytes, and its isdf_host_path tells that a step of this engine and
shape is ONE fused launch.

K + 1 = 2 and 5 leave row groups empty, 6 is one row per group, 7 and 65 are ragged groups, 127 and 128 end below and on the last
thread of the tail's one pass; N = 1 makes the collector take its own early cost, N = 65 sends its lanes into their second round."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K1S = (2, 5, 6, 7, 65, 127, 128)
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


def config(pkg, K1, enable_dyn=1, enable_pos=1, vmax=10.0):
    return pkg.synth.default_config(pkg.capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=K1 - 1, safety_hor=0.5, enable_dyn=enable_dyn,
                                    enable_pos=enable_pos, vmax=vmax)


def shape(pkg, name):
    if name == "Box":
        return pkg.synth.make_shape("Box", params=(1.2, 0.4, 0.3), grad_mode=pkg.capi.GRAD_CENTRAL)
    return pkg.synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6))


def cases():
    """name -> (map, K + 1, N, enable_dyn, enable_pos, shape, trajectory seed, vmax)"""
    out = {}
    for K1 in K1S:
        out[f"boxes_K1_{K1}_N3"] = ("boxes", K1, 3, 1, 1, "Box", 11, 10.0)
    out["boxes_K1_65_N1"] = ("boxes", 65, 1, 1, 1, "Box", 11, 10.0)
    out["boxes_K1_7_N65"] = ("boxes", 7, 65, 1, 1, "Box", 11, 10.0)       # (114 sweep workgroups + 65 tails: still one resident launch)
    out["empty_K1_65_N3"] = ("empty", 65, 3, 1, 1, "Box", 11, 10.0)
    out["nopos_K1_65_N3"] = ("boxes", 65, 3, 1, 0, "Box", 11, 0.5)         # (a speed limit the trajectory exceeds: the cost is the dynamics penalties')
    out["nodyn_K1_65_N3"] = ("boxes", 65, 3, 0, 1, "Box", 11, 10.0)
    out["cone_K1_65_N3"] = ("boxes", 65, 3, 1, 1, "RoundedCone", 11, 10.0)
    return out


def flat(cost, gT, gC):
    return np.concatenate([[cost], gT, gC])          # the step's 1 + 19 N outputs, as isdf_eval_device lays them out


def main():
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)                       # torch's HIP runtime first (tests/conftest.py, _torch_first)
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    stream = torch.cuda.current_stream().cuda_stream

    def device_step(eng, T, cm):
        """One device-resident step; the output buffer starts as NaN, so a value that never arrived shows."""
        N = T.size
        d_T = torch.from_numpy(T).to(dev)
        d_C = torch.from_numpy(np.ascontiguousarray(cm, dtype=np.float64).reshape(-1)).to(dev)
        d_out = torch.full((eng.out_stride(N),), float("nan"), dtype=torch.float64, device=dev)
        eng.eval_device(1, N, d_T.data_ptr(), d_C.data_ptr(), d_out.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()[:1 + 19 * N].copy()

    occ, esdf = world(pkg)
    grids = {"boxes": esdf, "empty": empty_esdf()}
    res = {}
    for name, (m, K1, N, dyn, pos, shp, seed, vmax) in cases().items():
        eng = pkg.Engine(config(pkg, K1, dyn, pos, vmax))
        eng.set_grid(grids[m], (0, 0, 0), RES, capi.GRID_ESDF)
        eng.set_shape(shape(pkg, shp))
        T, cm = trajectory(pkg, occ, N, seed)
        res[name] = device_step(eng, T, cm)
        res[name + "/overflow_device"] = np.array(eng.stats()["overflow"])
        res[name + "/host"] = flat(*eng.eval_single(T, cm))
        res[name + "/host_path"] = np.array(eng.host_path())
        st = eng.stats()
        res[name + "/grad_pairs"] = np.array(st["grad_pairs"])
        res[name + "/overflow_host"] = np.array(st["overflow"])
        res[name + "/again"] = device_step(eng, T, cm)      # (and the host-direct step handed every slot back empty as well)
        eng.close()
    # one engine, trajectory A, then B, then A again, all device-resident
    eng = pkg.Engine(config(pkg, 65))
    eng.set_grid(esdf, (0, 0, 0), RES, capi.GRID_ESDF)
    eng.set_shape(shape(pkg, "Box"))
    for tag, seed in (("A1", 11), ("B", 12), ("A2", 11)):
        res["aba_" + tag] = device_step(eng, *trajectory(pkg, occ, 3, seed))
    eng.close()
    np.savez(sys.argv[1], **res)
    print("RESULT ok")


if __name__ == "__main__":
    main()
