"""Poses per second of the tabulated pair potential on the GPU (dfm_pose_pairpot) at cutoffs 8 A and 15 A, without and with the pair
counts, next to the interface energy (dfm_pose_iface_energy, 8 A) in the same run on the same box: the case of tools/sterics_bench.py and
tools/iface_bench.py, 10 240 rigid poses of the 300 + 300 complex at 8 heavy atoms per residue.  Writes profiles/pairpot.txt.

    python tools/pairpot_bench.py [--out profiles/pairpot.txt] [--reps 7] [--host-poses 16]

The atoms and poses are make_case of tools/sterics_bench.py.  Types: 20 residue types drawn per residue with a seed, every atom of a
residue carrying its residue's type (T = 20); bins of 0.5 A from 0 to the cutoff (NB = 16 at 8 A, 30 at 15 A); a seeded asymmetric table
in [-1, 1] kcal/mol - a table of no merit: the project ships none.

GPU: 2 warm-up calls, then `reps` timed calls; wall time of the whole call from a host clock, copy and kernel time from the call's own HIP
events (dfm_pairpot_last_timing, dfm_pairpot_last_phases); median and min-max.  The counts call moves P T T NB int32 to the host, so its
wall time is mostly that copy; its kernel time is what the atomics cost.  Before any time is printed the results on the first
`host-poses` poses - totals, per-atom sums and counts - are asserted EQUAL to the definition's integers (dfmdock_amd/pairpot.py)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairpot.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=16, help="poses the results are compared with the numpy definition on")
    a = ap.parse_args()
    from iface_bench import eight_atom_params
    from sterics_bench import make_case
    from dfmdock_amd import engine
    from dfmdock_amd import pairpot as PP
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["tabulated pair potential: GPU call (dfm_pose_pairpot) without and with pair counts vs dfm_pose_iface_energy in the same run",
             engine.config_string()]
    med = lambda v: float(np.median(v))
    R, L, P, seed, T = 300, 300, 10240, 1, 20
    rec, lig, cen, rot, tr = make_case(R, L, P, seed)
    rng = np.random.default_rng(seed + 200)
    rt, lt = np.repeat(rng.integers(0, T, R), 8).astype(np.int32), np.repeat(rng.integers(0, T, L), 8).astype(np.int32)
    n = min(a.host_poses, P)
    lines.append(f"C3 ensemble: R = {R}, L = {L} residues at 8 heavy atoms = {rec.shape[0]} + {lig.shape[0]} atoms, P = {P}, T = {T} types")
    # the parent's nearest kernel, in the same run
    prng = np.random.default_rng(seed + 100)
    with model.interface(rec, eight_atom_params(R, prng), lig, eight_atom_params(L, prng), cen) as h:
        io, iwall, icopy, ikern = timed(lambda: h.energy(rot, tr), engine.iface_last_timing, a.reps)
    lines.append(f"  dfm_pose_iface_energy, 8 A         wall median {med(iwall):.2f} ms, kernels median {med(ikern):.3f} ms (min {min(ikern):.3f}, max "
                 f"{max(ikern):.3f}); {int(io['n_pairs'].sum())} pairs")
    ratio = {}
    for cutoff in (8.0, 15.0):
        NB = int(round(cutoff / 0.5))
        edges = np.linspace(0.0, cutoff, NB + 1).astype(np.float32)
        table = rng.uniform(-1.0, 1.0, (T, T, NB)).astype(np.float32)
        want = PP.pair_potential(rec, rt, lig, lt, cen, rot[:n], tr[:n], edges, table, per_atom=True, counts=True)
        t0 = time.perf_counter()
        h = model.pairpot(rec, rt, lig, lt, cen, edges, table)
        create_ms = (time.perf_counter() - t0) * 1e3
        o, wall, copy, kern = timed(lambda: h.energy(rot, tr), engine.pairpot_last_timing, a.reps)
        ph = engine.pairpot_last_phases()
        oc, cwall, ccopy, ckern = timed(lambda: h.energy(rot, tr, counts=True), engine.pairpot_last_timing, max(3, a.reps // 2))
        cph = engine.pairpot_last_phases()
        sub = h.energy(rot[:n], tr[:n], per_atom=True, counts=True)
        info = h.info()
        h.close()
        for key in ("energy_q", "n_pairs"):
            assert np.array_equal(o[key], oc[key]) and np.array_equal(o[key][:n], sub[key]) and np.array_equal(sub[key], want[key]), key
        for key in ("lig_q", "counts"):
            assert np.array_equal(sub[key], want[key]), key
        assert np.array_equal(oc["counts"][:n], want["counts"])
        near = int(o["n_pairs"].sum())
        ratio[cutoff] = med(kern) / med(ikern)
        lines += [
            f"cutoff {cutoff:g} A, NB = {NB} bins of 0.5 A: grid of {info['n_cells']} cells, at most {info['max_cell_atoms']} atoms in one, pair bound "
            f"{info['pair_bound']:.3g}; {near} pairs in range, {int((o['n_pairs'] == 0).sum())} poses without one; table slab of one receptor type "
            f"{T * NB * 4} bytes, whole table {T * T * NB * 4} bytes; equal to the definition's integers on {n} poses ({int(want['n_pairs'].sum())} pairs)",
            f"  dfm_pairpot_create                 {create_ms:.2f} ms once",
            f"  energy only, wall                  {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls",
            f"  energy only, kernels               median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}) = {near / med(kern) / 1e6:.2f} G pairs/s; last call by phase: "
            f"memsets {ph[0]:.3f}, walk {ph[1]:.3f}, finish {ph[2]:.3f} ms; {ratio[cutoff]:.2f} x the kernels of dfm_pose_iface_energy at 8 A",
            f"  with counts, wall                  median {med(cwall):.2f} ms (min {min(cwall):.2f}, max {max(cwall):.2f}); {P * T * T * NB * 4 / 2.0 ** 20:.0f} MiB of counts to the host",
            f"  with counts, kernels               median {med(ckern):.3f} ms (min {min(ckern):.3f}, max {max(ckern):.3f}) = {med(ckern) / med(kern):.2f} x energy only, "
            f"{near / med(ckern) / 1e6:.2f} G atomics/s; last call by phase: memsets {cph[0]:.3f}, walk {cph[1]:.3f}, finish {cph[2]:.3f} ms",
        ]
    lines.append(f"energy-only kernels over dfm_pose_iface_energy's at 8 A: {ratio[8.0]:.2f} x at 8 A, {ratio[15.0]:.2f} x at 15 A")
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
