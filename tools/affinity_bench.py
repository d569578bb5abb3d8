"""Poses per second of the residue contacts by class on the GPU (dfm_pose_rescon) next to the clash / contact screen (dfm_pose_sterics)
at the same cutoff on the same box - the same walk and the same counting atom pairs - and against the float64 numpy definition
(dfmdock_amd/affinity.py) on the same host: the case of tools/sterics_bench.py, 10 240 rigid poses of the 300 + 300 complex at 8 heavy
atoms per residue.  Writes profiles/affinity.txt.

    python tools/affinity_bench.py [--out profiles/affinity.txt] [--reps 7] [--host-poses 64]

The atoms and poses are make_case of tools/sterics_bench.py; residue = atom index // 8, classes seeded.  Cutoff 5.5 A.

GPU: 2 warm-up calls, then `reps` timed calls; wall time of the whole call from a host clock, copy and kernel time from the call's own HIP
events (dfm_rescon_last_timing: the memset of the bitmap, k_rescon_pose, k_rescon, k_rescon_finish); median and min-max.
dfm_pose_sterics with contact cutoff 5.5 A is timed the same way right after.  The definition is timed on the first `host-poses` poses and
scaled linearly to P (labelled as scaled).  Before any time is printed the timed call's results on that subset - every array - are
asserted EQUAL to the definition's, and the screen's n_contact > 0 is asserted to be n_pairs > 0.

Where the extra over the screen goes: the call's own events split its kernel time into zeroing the bitmap, the walk (k_rescon_pose,
k_rescon) and k_rescon_finish (dfm_rescon_last_phases; medians over the same timed calls).  The walk's own extra - the atomics, the loads
before them, the residue bits - is the walk's time minus the screen's whole kernel time of the same run, which is the same walk with
counters in registers instead.  Both calls are also timed on P poses 500 A away, where every wave leaves at the sphere test, to show
what the zeroing and the finish cost when there is nothing to find: k_rescon_finish has no data-dependent branch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affinity.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=64, help="poses the numpy definition is timed on (scaled linearly to P)")
    a = ap.parse_args()
    from iface_bench import timed
    from sterics_bench import make_case
    from dfmdock_amd import affinity as AF
    from dfmdock_amd import engine
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["residue contacts by class: GPU call (dfm_pose_rescon) vs dfm_pose_sterics at the same cutoff and the float64 numpy definition "
             "(affinity.residue_contacts)", engine.config_string()]
    med = lambda v: float(np.median(v))
    keys = ("ic", "n_pairs", "n_rec_res", "n_lig_res", "rec_degree", "lig_degree", "contact_bits")
    for name, R, L, P, seed in [("C3 ensemble", 300, 300, 10240, 1)]:
        rec, lig, cen, rot, tr = make_case(R, L, P, seed)
        prng = np.random.default_rng(seed + 200)
        rres, lres = (np.arange(rec.shape[0]) // 8).astype(np.int32), (np.arange(lig.shape[0]) // 8).astype(np.int32)
        rcls, lcls = prng.integers(0, 3, R).astype(np.uint8), prng.integers(0, 3, L).astype(np.uint8)
        far = tr + np.float32([500.0, 0.0, 0.0])
        n = min(a.host_poses, P)
        t0 = time.perf_counter()
        want = AF.residue_contacts(rec, rres, rcls, lig, lres, lcls, cen, rot[:n], tr[:n], 5.5, per_residue=True, bits=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        h = model.contacts(rec, rres, rcls, lig, lres, lcls, cen, 5.5)
        create_ms = (time.perf_counter() - t0) * 1e3
        phases = []

        def both():
            phases.append(engine.rescon_last_phases())
            return engine.rescon_last_timing()
        o, wall, copy, kern = timed(lambda: h.count(rot, tr), both, a.reps)
        ph = np.median(np.array(phases[-a.reps:]), 0)
        _, _, _, kern_far = timed(lambda: h.count(rot, far), both, a.reps)
        ph_far = np.median(np.array(phases[-a.reps:]), 0)
        _, wall_b, _, kern_b = timed(lambda: h.count(rot, tr, per_residue=True, bits=True), engine.rescon_last_timing, a.reps)
        sub = h.count(rot[:n], tr[:n], per_residue=True, bits=True)
        for key in keys:
            assert np.array_equal(sub[key], want[key]), key
        for key in keys[:4]:
            assert np.array_equal(o[key][:n], sub[key]), key
        info = h.info()
        h.close()
        with model.atoms(rec, lig, cen, 3.0, 5.5) as at:
            so, swall, scopy, skern = timed(lambda: at.sterics(rot, tr), engine.sterics_last_timing, a.reps)
            _, _, _, skern_far = timed(lambda: at.sterics(rot, far), engine.sterics_last_timing, a.reps)
        assert np.array_equal(so["n_contact"] > 0, o["n_pairs"] > 0)
        atom_pairs, res_pairs = int(so["n_contact"].sum(dtype=np.int64)), int(o["n_pairs"].sum(dtype=np.int64))
        W = info["row_words"]
        chunks = -(-P // info["chunk_poses"])
        bitmap = P * L * W * 4
        walk = ph[1] - med(skern)
        lines += [
            f"{name}: R = {R}, L = {L} residues at 8 heavy atoms = {rec.shape[0]} + {lig.shape[0]} atoms, P = {P}; grid of {info['n_cells']} cells of "
            f"{info['cell_edge']:g} A, at most {info['max_cell_atoms']} atoms in one; {res_pairs} residue pairs from {atom_pairs} atom pairs below 5.5 A "
            f"({atom_pairs / max(1, res_pairs):.1f} atom pairs per residue pair), {int((o['n_pairs'] == 0).sum())} poses without a pair; bitmap "
            f"{L} x {W} words per pose = {bitmap / 2 ** 20:.1f} MiB per call in {chunks} chunks of at most {info['chunk_poses']} poses; every array "
            f"equal to the definition's on {n} poses ({int(want['n_pairs'].sum())} residue pairs)",
            f"  numpy definition, 1 core  {n / host_ms * 1e3:10.1f} poses/s   {host_ms:.0f} ms for {n} poses = {host_ms * P / n:.0f} ms for P poses (scaled)",
            f"  dfm_rescon_create         {create_ms:.2f} ms once (counting sort, Morton sort, class masks, 6 uploads)",
            f"  GPU call, wall            {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls"
            f" = {host_ms * P / n / med(wall):.0f} x the scaled definition",
            f"  of which host-to-device   median {med(copy):.3f} ms ({100 * med(copy) / med(wall):.0f} % of wall; {P * 24} bytes of poses)",
            f"  of which kernels          median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}) = {atom_pairs / med(kern) / 1e6:.2f} G atom pairs below the cutoff/s",
            f"  with degrees and bits     wall median {med(wall_b):.2f} ms, kernels median {med(kern_b):.3f} ms ({(P * (R + L) * 4 + bitmap) / 2 ** 20:.0f} MiB more to the host)",
            f"  dfm_pose_sterics at 5.5 A wall median {med(swall):.2f} ms, kernels median {med(skern):.3f} ms (min {min(skern):.3f}, max {max(skern):.3f}), same run, "
            f"same walk, same {atom_pairs} counting pairs: the contacts' kernels take {med(kern) / med(skern):.2f} x the screen's",
            f"  by phase (own events)     zeroing the bitmap {ph[0]:.3f} ms, the walk {ph[1]:.3f} ms, k_rescon_finish {ph[2]:.3f} ms",
            f"  where the extra goes      of the {med(kern) - med(skern):.3f} ms over the screen: zeroing {ph[0]:.3f} ms, finish {ph[2]:.3f} ms, the walk's own extra "
            f"(atomics, the loads before them: walk - the screen's kernels) {walk:.3f} ms",
            f"  every pose 500 A away     contacts' kernels median {med(kern_far):.3f} ms (zeroing {ph_far[0]:.3f}, walk {ph_far[1]:.3f}, finish {ph_far[2]:.3f}), the "
            f"screen's {med(skern_far):.3f} ms (every wave leaves at the sphere test)",
        ]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
