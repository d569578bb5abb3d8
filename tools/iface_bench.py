"""Poses per second of the interface energy on the GPU (dfm_pose_iface_energy) next to the clash / contact screen (dfm_pose_sterics) on
the same box and against the float64 numpy definition (dfmdock_amd/ifenergy.py) on the same host: the case of tools/sterics_bench.py,
10 240 rigid poses of the 300 + 300 complex at 8 heavy atoms per residue.  Writes profiles/iface.txt.

    python tools/iface_bench.py [--out profiles/iface.txt] [--reps 7] [--host-poses 64]

The atoms and poses are make_case of tools/sterics_bench.py.  Parameters: N, CA, C, O, CB by element (ifenergy.LJ), the three side-chain
pseudo-atoms as carbons, a seeded charge of +-0.5 on the outermost pseudo-atom of every residue.  Cutoff 8 A, the default scalars.

GPU: 2 warm-up calls, then `reps` timed calls; wall time of the whole call from a host clock, copy and kernel time from the call's own HIP
events (dfm_iface_last_timing); median and min-max.  dfm_pose_sterics (cutoffs 3 / 5 A) is timed the same way right after.  The share
of waves that walk cells is counted by the screen's exit counters on a handle whose contact cutoff is the 8 A of this call: the same
grid, the same threshold, the same early-exit tests (dfm_posewalk.h).  The definition is timed on the first `host-poses` poses and scaled
linearly to P (labelled as scaled).  Before any time is printed the timed call's results on that subset - totals and per-atom sums -
are asserted EQUAL to the definition's integers.

Two floors, computed as in tools/sterics_bench.py, both lower bounds.  Bytes: every wave reads its pose (96 bytes) and its block's sphere
(16 bytes), a wave that stays reads its 64 atoms and their parameters (2 KiB); the receptor stays in cache - over the 8 TB/s HBM figure.
Float64 work: 24 operations per atom a staying wave transforms and 26 per pair within the cutoff (8 for r2, 15 for the three terms with
a division counted as one, 3 scalings to quanta), over the MI355X data sheet's vector fp64 peak of 78.6 TFLOP/s."""
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


def eight_atom_params(n_res, rng):
    from dfmdock_amd import ifenergy as IE
    row = lambda el: [IE.LJ[el][0], np.sqrt(np.float64(IE.LJ[el][1])), 0.0]
    par = np.tile(np.float32([row(e) for e in ("N", "C", "C", "O", "C", "C", "C", "C")]), (n_res, 1))
    par[7::8, 2] = rng.choice(np.float32([-0.5, 0.5]), n_res)
    return par


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iface.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=64, help="poses the numpy definition is timed on (scaled linearly to P)")
    a = ap.parse_args()
    from sterics_bench import make_case
    from dfmdock_amd import engine
    from dfmdock_amd import ifenergy as IE
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["interface energy: GPU call (dfm_pose_iface_energy) vs dfm_pose_sterics and the float64 numpy definition (ifenergy.interface_energy)",
             engine.config_string()]
    med = lambda v: float(np.median(v))
    for name, R, L, P, seed in [("C3 ensemble", 300, 300, 10240, 1)]:
        rec, lig, cen, rot, tr = make_case(R, L, P, seed)
        prng = np.random.default_rng(seed + 100)
        rp, lp = eight_atom_params(R, prng), eight_atom_params(L, prng)
        n = min(a.host_poses, P)
        t0 = time.perf_counter()
        want = IE.interface_energy(rec, rp, lig, lp, cen, rot[:n], tr[:n], per_atom=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        h = model.interface(rec, rp, lig, lp, cen)
        create_ms = (time.perf_counter() - t0) * 1e3
        o, wall, copy, kern = timed(lambda: h.energy(rot, tr), engine.iface_last_timing, a.reps)
        sub = h.energy(rot[:n], tr[:n], per_atom=True)
        for key in ("rep_q", "att_q", "elec_q", "n_pairs"):
            assert np.array_equal(o[key][:n], sub[key]) and np.array_equal(sub[key], want[key]), key
        for key in ("lig_vdw_q", "lig_elec_q"):
            assert np.array_equal(sub[key], want[key]), key
        info = h.info()
        h.close()
        with model.atoms(rec, lig, cen) as at:
            so, swall, scopy, skern = timed(lambda: at.sterics(rot, tr), engine.sterics_last_timing, a.reps)
        with model.atoms(rec, lig, cen, 3.0, 8.0) as at8:
            engine.sterics_exit_counts(True)
            at8.sterics(rot, tr)
            waves, at_sphere, at_box = engine.sterics_exit_counts(False)
        stay = waves - at_sphere - at_box
        near = int(o["n_pairs"].sum())
        pairs = P * rec.shape[0] * lig.shape[0]
        byte_ms = (waves * 112 + stay * 2048) / HBM_BPS * 1e3
        flop_ms = (stay * 64 * 24 + near * 26) / FP64_FLOPS * 1e3
        tot = IE.total(o["rep"], o["att"], o["elec"])
        lines += [
            f"{name}: R = {R}, L = {L} residues at 8 heavy atoms = {rec.shape[0]} + {lig.shape[0]} atoms, P = {P}; grid of {info['n_cells']} cells of "
            f"{info['cell_edge']:g} A, at most {info['max_cell_atoms']} atoms in one; {near} pairs within 8 A in {pairs} atom pairs, "
            f"{int((o['n_pairs'] == 0).sum())} poses without a pair; total (weights {IE.WEIGHTS}) from {tot.min():.1f} to {tot.max():.1f} kcal/mol; sum bound "
            f"2^{np.log2(info['sum_bound_q']):.1f} quanta; equal to the definition's integers on {n} poses ({int(want['n_pairs'].sum())} pairs)",
            f"  numpy definition, 1 core  {n / host_ms * 1e3:10.1f} poses/s   {host_ms:.0f} ms for {n} poses = {host_ms * P / n:.0f} ms for P poses (scaled)",
            f"  dfm_iface_create          {create_ms:.2f} ms once (counting sort, Morton sort, 7 uploads)",
            f"  GPU call, wall            {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls"
            f" = {host_ms * P / n / med(wall):.0f} x the scaled definition",
            f"  of which host-to-device   median {med(copy):.3f} ms ({100 * med(copy) / med(wall):.0f} % of wall; {P * 24} bytes of poses)",
            f"  of which kernels          median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}) = {near / med(kern) / 1e6:.2f} G pairs within the cutoff/s",
            f"  dfm_pose_sterics, same box wall median {med(swall):.2f} ms, kernels median {med(skern):.3f} ms (min {min(skern):.3f}, max {max(skern):.3f}); "
            f"{int(so['n_contact'].sum(dtype=np.int64))} pairs below 5 A: the energy's kernels take {med(kern) / med(skern):.2f} x the screen's for "
            f"{near / max(1, int(so['n_contact'].sum(dtype=np.int64))):.2f} x the pairs",
            f"  early exits (8 A grid)    {waves} waves: {100 * at_sphere / waves:.1f} % leave at the sphere test, {100 * at_box / waves:.1f} % at the box test, "
            f"{100 * stay / waves:.1f} % walk cells",
            f"  floors                    bytes {byte_ms:.4f} ms at 8 TB/s ({100 * byte_ms / med(kern):.1f} % of the kernel time); float64 "
            f"{flop_ms:.4f} ms at 78.6 TFLOP/s ({100 * flop_ms / med(kern):.2f} %): the kernels are "
            f"{'near neither floor: the float32 reject over the staged receptor atoms and the converged fp64 recipe of the waves that stay dominate' if max(byte_ms, flop_ms) < 0.5 * med(kern) else ('near the byte floor' if byte_ms > flop_ms else 'near the float64 floor')}",
        ]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
