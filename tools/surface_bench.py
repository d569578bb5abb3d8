"""Poses per second of the buried-surface-area call on the GPU (dfm_pose_bsa) against the float64 numpy definition
(dfmdock_amd/surface.py) on the same host: the 10 240 rigid poses of the 2 400 + 2 400 atom complex of tools/sterics_bench.py.  Writes
profiles/surface.txt.

    python tools/surface_bench.py [--out profiles/surface.txt] [--reps 7] [--host-poses 64]

The atoms and the poses are those of tools/sterics_bench.py (make_case); the radii are 1.55, 1.70, 1.70, 1.52 for N, CA, C, O and 1.70 for
CB and the three side-chain pseudo-atoms; probe 1.4 A, 128 sphere points.

GPU: 2 warm-up calls, then `reps` timed calls; wall time of the whole call from a host clock, copy and kernel time from the call's own
HIP events (dfm_bsa_last_timing); median and min-max.  The definition is timed on the first `host-poses` poses (its isolated exposure
pass timed apart, since it does not grow with P) and scaled linearly to P (labelled as scaled).  Before any time is printed the call's
per-atom counts on that subset are asserted against the definition (within each atom's border points, 1e-6 A).

Two floors, computed here, both lower bounds of what the kernels must do.  Bytes: the receptor masks are zeroed, ORed into and read back
once (3 Ar K / 8 bytes per pose), every wave reads its pose and its block's sphere (112 bytes) - over the 8 TB/s HBM figure.  Float64
work: 20 operations per point and direction of a near pair whose atom has an exposed point (6 for the point, 3 subtractions, 3
multiplications, 2 additions, a square root and a compare counted as one each, rounded up) - counted by the definition on the subset
and scaled - over the MI355X data sheet's vector fp64 peak of 78.6 TFLOP/s."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BPS = 8.0e12
FP64_FLOPS = 78.6e12
BORDER = 1e-6
RAD8 = np.float32([1.55, 1.70, 1.70, 1.52, 1.70, 1.70, 1.70, 1.70])


def check_subset(got, rec, rr, lig, lr, cen, rot, tr, n, K):
    """The sanity condition: the call's per-atom counts on the first n poses against the definition, border points aside.  Returns
    (near pairs, buried points, border points, point groups of 64 a near pair must test) of the subset."""
    from dfmdock_amd import surface as SF
    er, el = SF.exposure(rec, rr, K=K), SF.exposure(lig, lr, K=K)
    pairs = buried = border = 0
    for p in range(n):
        lm, rm, np_ = SF.pose_margins(rec, rr, lig, lr, cen, rot[p], tr[p], K=K)
        for key, m, ex in (("lig_buried", lm, el), ("rec_buried", rm, er)):
            want, edge = (ex & (m < 0)).sum(1), (ex & (np.abs(m) < BORDER)).sum(1)
            assert (np.abs(got[key][p] - want) <= edge).all(), (key, p)
            buried += int(want.sum())
            border += int(edge.sum())
        pairs += np_
    return pairs, buried, border


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=64, help="poses the numpy definition is timed on (scaled linearly to P)")
    a = ap.parse_args()
    from sterics_bench import make_case
    from dfmdock_amd import engine
    from dfmdock_amd import surface as SF
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["buried surface area: GPU call (dfm_pose_bsa) vs the float64 numpy definition (surface.bsa)", engine.config_string()]
    med = lambda v: float(np.median(v))
    K = 128
    for name, R, L, P, seed in [("C3 ensemble", 300, 300, 10240, 1)]:
        rec, lig, cen, rot, tr = make_case(R, L, P, seed)
        rr, lr = np.tile(RAD8, R), np.tile(RAD8, L)
        n = min(a.host_poses, P)
        t0 = time.perf_counter()
        SF.exposure(rec, rr, K=K), SF.exposure(lig, lr, K=K)
        expo_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        SF.bsa(rec, rr, lig, lr, cen, rot[:n], tr[:n], K=K)
        host_ms = (time.perf_counter() - t0) * 1e3 - expo_ms
        t0 = time.perf_counter()
        sf = model.surface(rec, rr, lig, lr, cen, points=K)
        create_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(2):
            sf.bsa(rot, tr)
        wall, copy, kern = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            o = sf.bsa(rot, tr)
            wall.append((time.perf_counter() - t0) * 1e3)
            c, k = engine.bsa_last_timing()
            copy.append(c)
            kern.append(k)
        sub = sf.bsa(rot[:n], tr[:n], per_atom=True)
        for key in ("bsa", "lig_points", "rec_points", "class_points"):
            assert np.array_equal(o[key][:n], sub[key]), key
        pairs, buried, border = check_subset(sub, rec, rr, lig, lr, cen, rot, tr, n, K)
        info = sf.info()
        sf.close()
        waves = P * ((lig.shape[0] + 63) // 64)
        byte_ms = (P * 3 * rec.shape[0] * K / 8 + waves * 112) / HBM_BPS * 1e3
        flop_ms = pairs * P / n * 2 * K * 20 / FP64_FLOPS * 1e3
        lines += [
            f"{name}: R = {R}, L = {L} residues at 8 heavy atoms = {rec.shape[0]} + {lig.shape[0]} atoms, P = {P}, K = {K} points, probe 1.4 A; grid of "
            f"{info['n_cells']} cells of {info['cell_edge']:g} A, at most {info['max_cell_atoms']} atoms in one; isolated SASA {info['sasa_rec']:.0f} + "
            f"{info['sasa_lig']:.0f} A^2 ({int(info['rec_exposed'].sum())} + {int(info['lig_exposed'].sum())} exposed points); "
            f"{int(o['rec_points'].sum(dtype=np.int64))} + {int(o['lig_points'].sum(dtype=np.int64))} buried points, BSA {o['bsa'].min():.0f} .. "
            f"{o['bsa'].max():.0f} A^2 (median {np.median(o['bsa']):.0f}); checked against the definition on {n} poses ({pairs} near pairs, {buried} "
            f"buried points, {border} border points)",
            f"  numpy definition, 1 core  {n / host_ms * 1e3:10.1f} poses/s   {host_ms:.0f} ms for {n} poses = {host_ms * P / n:.0f} ms for P poses (scaled), "
            f"plus {expo_ms:.0f} ms of isolated exposure once",
            f"  dfm_surface_create        {create_ms:.2f} ms once (isolated exposure on the host, two sorts, 11 uploads)",
            f"  GPU call, wall            {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls"
            f" = {host_ms * P / n / med(wall):.0f} x the scaled definition",
            f"  of which host-to-device   median {med(copy):.3f} ms ({100 * med(copy) / med(wall):.0f} % of wall; {P * 24} bytes of poses)",
            f"  of which kernels          median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f})",
            f"  floors                    bytes {byte_ms:.4f} ms at 8 TB/s ({100 * byte_ms / med(kern):.1f} % of the kernel time); float64 "
            f"{flop_ms:.4f} ms at 78.6 TFLOP/s ({100 * flop_ms / med(kern):.2f} %): the kernels are bound by "
            f"{'neither: the float32 pair test over the staged receptor atoms and the serial walk of the pair queue dominate' if max(byte_ms, flop_ms) < 0.5 * med(kern) else ('bytes' if byte_ms > flop_ms else 'float64 work')}",
        ]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
