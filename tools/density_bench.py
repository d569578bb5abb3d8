"""Poses per second of the density fit on the GPU (dfm_pose_density) on a 96^3 and a 192^3 grid, next to the all-atom clash screen
(dfm_pose_sterics) in the same run on the same box: the case of tools/sterics_bench.py, 10 240 rigid poses of the 300 + 300 complex at 8
heavy atoms per residue.  Writes profiles/density.txt.

    python tools/density_bench.py [--out profiles/density.txt] [--reps 7] [--host-poses 16]

The atoms and poses are make_case of tools/sterics_bench.py; every atom weighs 6.  The grid: three channels of seeded normal values (what
the values are does not matter to a gather, where they lie does) on a cube over the receptor's and the ligand's box grown by 12 A, n nodes
per axis - at 96^3 a voxel of about 2 A, at 192^3 half that; with 16 bytes per node 13.5 MiB and 108 MiB on the device.

GPU: 2 warm-up calls, then `reps` timed calls; wall time of the whole call from a host clock, copy and kernel time from the call's own HIP
events (dfm_density_last_timing); median and min-max.  Bytes gathered: 8 corners of 16 bytes per atom inside the grid (outside atoms
gather node 0 and are not counted).  Before any time is printed the results on the first `host-poses` poses - the four arrays - are
asserted EQUAL to the definition's integers (dfmdock_amd/density.py), and the definition's own time per pose on one core is taken from
that call and a one-pose call before it (their difference: the definition checks the whole grid once per call)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(call, last_timing, reps):
    for _ in range(2):
        call()
    wall, copy, kern = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        o = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        c, k = last_timing()
        copy.append(c)
        kern.append(k)
    return o, wall, copy, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=16, help="poses the results are compared with the numpy definition on")
    a = ap.parse_args()
    from sterics_bench import make_case
    from dfmdock_amd import density as DN
    from dfmdock_amd import engine
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["density fit: GPU call (dfm_pose_density) on a 96^3 and a 192^3 grid vs dfm_pose_sterics in the same run", engine.config_string()]
    med = lambda v: float(np.median(v))
    R, L, P, seed = 300, 300, 10240, 1
    rec, lig, cen, rot, tr = make_case(R, L, P, seed)
    w = np.full(lig.shape[0], 6.0, np.float32)
    n = min(a.host_poses, P)
    lines.append(f"C3 ensemble: R = {R}, L = {L} residues at 8 heavy atoms = {rec.shape[0]} + {lig.shape[0]} atoms, P = {P}")
    with model.atoms(rec, lig, cen) as h:
        so, swall, scopy, skern = timed(lambda: h.sterics(rot, tr), engine.sterics_last_timing, a.reps)
    lines.append(f"  dfm_pose_sterics, 3 / 5 A          wall median {med(swall):.2f} ms, kernels median {med(skern):.3f} ms (min {min(skern):.3f}, max "
                 f"{max(skern):.3f}); {int(so['n_contact'].sum())} contacts")
    both = np.concatenate([rec, lig]).astype(np.float64)
    lo, hi = both.min(0) - 12.0, both.max(0) + 12.0
    ratio = {}
    for nodes in (96, 192):
        rng = np.random.default_rng(seed + nodes)
        voxel = np.float32([(hi - lo).max() / (nodes - 1)] * 3)
        origin = (0.5 * (lo + hi) - 0.5 * float(voxel[0]) * (nodes - 1)).astype(np.float32)
        grids = rng.standard_normal((3, nodes, nodes, nodes), dtype=np.float32)
        t0 = time.perf_counter()
        DN.density(grids, origin, voxel, lig, w, cen, rot[:1], tr[:1], 1.0, per_atom=True)      # the grid's check and one pose
        t1 = time.perf_counter()
        want = DN.density(grids, origin, voxel, lig, w, cen, rot[:n], tr[:n], 1.0, per_atom=True)
        host_ms = max((time.perf_counter() - t1) - (t1 - t0), 0.0) * 1e3 / max(n - 1, 1)      # per further pose: the check is paid once per call
        t0 = time.perf_counter()
        h = model.density(grids, origin, voxel, lig, w, cen, 1.0)
        create_ms = (time.perf_counter() - t0) * 1e3
        o, wall, copy, kern = timed(lambda: h.fit(rot, tr), engine.density_last_timing, a.reps)
        oa, awall, acopy, akern = timed(lambda: h.fit(rot, tr, per_atom=True), engine.density_last_timing, max(3, a.reps // 2))
        sub = h.fit(rot[:n], tr[:n], per_atom=True)
        h.close()
        for key in ("sum_q", "n_inside", "n_above"):
            assert np.array_equal(o[key], oa[key]) and np.array_equal(o[key][:n], sub[key]) and np.array_equal(sub[key], want[key]), key
        assert np.array_equal(sub["atom_q"], want["atom_q"]) and np.array_equal(oa["atom_q"][:n], want["atom_q"])
        inside = int(o["n_inside"].sum())
        gathered = inside * 8 * 16
        ratio[nodes] = med(kern) / med(skern)
        lines += [
            f"grid {nodes}^3, voxel {float(voxel[0]):.3f} A, 3 channels, {nodes ** 3 * 16 / 2.0 ** 20:.1f} MiB on the device; {inside} of {P * lig.shape[0]} posed atoms inside, "
            f"{int((o['n_inside'] == 0).sum())} poses without one; equal to the definition's integers on {n} poses ({int(want['n_inside'].sum())} atoms inside)",
            f"  dfm_density_create                 {create_ms:.2f} ms once",
            f"  sums only, wall                    {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls",
            f"  sums only, kernels                 median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}) = {inside / med(kern) / 1e6:.2f} G atoms/s, "
            f"{gathered / med(kern) / 1e9:.2f} TB/s gathered; copies {med(copy):.3f} ms; {ratio[nodes]:.2f} x the kernels of dfm_pose_sterics",
            f"  with atom_q, wall                  median {med(awall):.2f} ms (min {min(awall):.2f}, max {max(awall):.2f}); {P * lig.shape[0] * 8 / 2.0 ** 20:.0f} MiB of atom_q to the host",
            f"  with atom_q, kernels               median {med(akern):.3f} ms (min {min(akern):.3f}, max {max(akern):.3f}) = {med(akern) / med(kern):.2f} x sums only",
            f"  float64 definition, one core       {host_ms:.2f} ms per pose (beyond the call's one check of the grid) = {host_ms * P / med(wall):.0f} x the call's wall time per pose, "
            f"{host_ms * P / med(kern):.0f} x its kernels",
        ]
    lines.append(f"kernels over dfm_pose_sterics's: {ratio[96]:.2f} x at 96^3, {ratio[192]:.2f} x at 192^3")
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
