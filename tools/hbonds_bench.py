"""Poses per second of the interface hydrogen bonds and salt bridges on the GPU (dfm_pose_hbonds) next to the residue contacts
(dfm_pose_rescon, 5.5 A over ALL heavy atoms) of the same complex and poses in the same process, and against the float64 numpy definition
(dfmdock_amd/hbonds.py) on the same host: the case of tools/sterics_bench.py, 10 240 rigid poses of the 300 + 300 complex at 8 heavy
atoms per residue, typed at the natural polar fraction.  Writes profiles/hbonds.txt.

    python tools/hbonds_bench.py [--out profiles/hbonds.txt] [--reps 7] [--host-poses 64]

The atoms and poses are make_case of tools/sterics_bench.py (N, CA, C, O, CB and three side-chain atoms per residue).  Typing: N is a
donor with antecedent CA, O an acceptor with antecedent C, and in a seeded two thirds of the residues the outermost side-chain atom is
polar with the atom before it as antecedent - donor, acceptor, both, cationic donor, anionic acceptor or the HIS role, in that order with
shares 0.2, 0.2, 0.2, 0.15, 0.2, 0.05 - which makes a third of the heavy atoms polar, as in a protein.  Defaults: 3.5 A, 90 degrees, 4.0 A.

GPU: 2 warm-up calls, then `reps` timed calls; wall time of the whole call from a host clock, copy and kernel time from the call's own HIP
events (dfm_hbond_last_timing: the memsets, k_hbond_pose, k_hbond, k_hbond_finish), split by phase (dfm_hbond_last_phases); median and
min-max.  dfm_pose_rescon is timed the same way right after.  The definition is timed on the first `host-poses` poses and scaled linearly
to P (labelled as scaled).  Before any time is printed the timed call's results on that subset - every array - are asserted EQUAL to the
definition's.  Both calls are also timed on P poses 500 A away, where every wave leaves at the sphere test."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIDE_ROLES = ((1 | 16, 0.2), (2 | 16, 0.2), (1 | 2 | 16, 0.2), (1 | 4 | 16, 0.15), (2 | 8 | 16, 0.2), (1 | 2 | 4 | 16, 0.05))


def typed(atoms, n_res, rng):
    """The polar atoms of a chain of n_res residues at 8 heavy atoms (make_case's order: N, CA, C, O, CB, three side-chain atoms)."""
    a = atoms.reshape(n_res, 8, 3)
    has = rng.random(n_res) < 2.0 / 3.0
    side = rng.choice([r for r, _ in SIDE_ROLES], n_res, p=[w for _, w in SIDE_ROLES]).astype(np.uint8)[has]
    r = np.arange(n_res)
    return {"xyz": np.concatenate([a[:, 0], a[:, 3], a[has, 7]]), "ante": np.concatenate([a[:, 1], a[:, 2], a[has, 6]]),
            "role": np.concatenate([np.full(n_res, 1, np.uint8), np.full(n_res, 2, np.uint8), side]),
            "res": np.concatenate([r, r, r[has]]).astype(np.int32), "n_res": n_res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hbonds.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=64, help="poses the numpy definition is timed on (scaled linearly to P)")
    a = ap.parse_args()
    from iface_bench import timed
    from sterics_bench import make_case
    from dfmdock_amd import engine
    from dfmdock_amd import hbonds as HB
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["hydrogen bonds and salt bridges: GPU call (dfm_pose_hbonds) vs dfm_pose_rescon on the same complex and poses and the float64 numpy "
             "definition (hbonds.hbonds)", engine.config_string()]
    med = lambda v: float(np.median(v))
    keys = ("n_hbond", "hb_kind", "n_salt", "n_salt_atoms", "rec_hb", "lig_hb", "rec_sb", "lig_sb")
    for name, R, L, P, seed in [("C3 ensemble", 300, 300, 10240, 1)]:
        rec, lig, cen, rot, tr = make_case(R, L, P, seed)
        prng = np.random.default_rng(seed + 300)
        rp, lp = typed(rec, R, prng), typed(lig, L, prng)
        far = tr + np.float32([500.0, 0.0, 0.0])
        n = min(a.host_poses, P)
        t0 = time.perf_counter()
        want = HB.hbonds(rp, lp, cen, rot[:n], tr[:n], per_atom=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        h = model.hbonds(rp, lp, cen)
        create_ms = (time.perf_counter() - t0) * 1e3
        phases = []

        def both():
            phases.append(engine.hbond_last_phases())
            return engine.hbond_last_timing()
        o, wall, copy, kern = timed(lambda: h.count(rot, tr), both, a.reps)
        ph = np.median(np.array(phases[-a.reps:]), 0)
        _, _, _, kern_far = timed(lambda: h.count(rot, far), both, a.reps)
        ph_far = np.median(np.array(phases[-a.reps:]), 0)
        _, wall_b, _, kern_b = timed(lambda: h.count(rot, tr, per_atom=True), engine.hbond_last_timing, a.reps)
        sub = h.count(rot[:n], tr[:n], per_atom=True)
        for key in keys:
            assert np.array_equal(sub[key], want[key]), key
        for key in keys[:4]:
            assert np.array_equal(o[key][:n], sub[key]), key
        info = h.info()
        h.close()
        # the yardstick: the residue contacts over every heavy atom of the same complex, 5.5 A, same poses, same process
        rres, lres = (np.arange(rec.shape[0]) // 8).astype(np.int32), (np.arange(lig.shape[0]) // 8).astype(np.int32)
        rcls, lcls = prng.integers(0, 3, R).astype(np.uint8), prng.integers(0, 3, L).astype(np.uint8)
        rphases = []

        def rboth():
            rphases.append(engine.rescon_last_phases())
            return engine.rescon_last_timing()
        with model.contacts(rec, rres, rcls, lig, lres, lcls, cen, 5.5) as rc:
            ro, rwall, _, rkern = timed(lambda: rc.count(rot, tr), rboth, a.reps)
            rph = np.median(np.array(rphases[-a.reps:]), 0)
            _, _, _, rkern_far = timed(lambda: rc.count(rot, far), rboth, a.reps)
        Nr, Nl = len(rp["role"]), len(lp["role"])
        bonds, bridges, sb_atoms = (int(o[k].sum(dtype=np.int64)) for k in ("n_hbond", "n_salt", "n_salt_atoms"))
        Wc = (info["n_rec_charged"] + 31) // 32
        chunks = -(-P // info["chunk_poses"])
        ratio = med(kern) / med(rkern)
        lines += [
            f"{name}: R = {R}, L = {L} residues at 8 heavy atoms = {rec.shape[0]} + {lig.shape[0]} atoms, of which {Nr} + {Nl} are polar "
            f"({100 * (Nr + Nl) / (rec.shape[0] + lig.shape[0]):.0f} %), P = {P}; grid of {info['n_cells']} cells of {info['cell_edge']:g} A, at most "
            f"{info['max_cell_atoms']} polar atoms in one; {bonds} hydrogen bonds ({int((o['n_hbond'] == 0).sum())} poses without one; backbone-backbone / mixed / "
            f"side-side {o['hb_kind'].sum(0, dtype=np.int64).tolist()}), {bridges} salt bridges from {sb_atoms} atom pairs; {info['n_rec_charged']} + "
            f"{info['n_lig_charged']} charged residues, bitmap {info['n_lig_charged']} x {Wc} words per pose in {chunks} chunks of at most "
            f"{info['chunk_poses']} poses; every array equal to the definition's on {n} poses ({int(want['n_hbond'].sum())} bonds, {int(want['n_salt'].sum())} bridges)",
            f"  numpy definition, 1 core  {n / host_ms * 1e3:10.1f} poses/s   {host_ms:.0f} ms for {n} poses = {host_ms * P / n:.0f} ms for P poses (scaled)",
            f"  dfm_hbond_create          {create_ms:.2f} ms once (counting sort, Morton sort, charged residues, 8 uploads)",
            f"  GPU call, wall            {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls"
            f" = {host_ms * P / n / med(wall):.0f} x the scaled definition",
            f"  of which host-to-device   median {med(copy):.3f} ms ({100 * med(copy) / med(wall):.0f} % of wall; {P * 24} bytes of poses)",
            f"  of which kernels          median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f})",
            f"  by phase (own events)     memsets {ph[0]:.3f} ms, the walk (k_hbond_pose, k_hbond) {ph[1]:.3f} ms, k_hbond_finish {ph[2]:.3f} ms",
            f"  with per-atom counts      wall median {med(wall_b):.2f} ms, kernels median {med(kern_b):.3f} ms ({P * (Nr + Nl) * 8 / 2 ** 20:.0f} MiB more to the host)",
            f"  dfm_pose_rescon at 5.5 A  wall median {med(rwall):.2f} ms, kernels median {med(rkern):.3f} ms (min {min(rkern):.3f}, max {max(rkern):.3f}; zeroing "
            f"{rph[0]:.3f}, walk {rph[1]:.3f}, finish {rph[2]:.3f}), same run, all {rec.shape[0]} + {lig.shape[0]} heavy atoms, {int(ro['n_pairs'].sum(dtype=np.int64))} "
            f"residue pairs",
            f"  ratio                     the hydrogen bonds' kernels take {ratio:.2f} x the residue contacts' ({'faster' if ratio < 1 else 'NOT faster'}); "
            f"walk against walk {ph[1] / rph[1]:.2f} x",
            f"  every pose 500 A away     hydrogen bonds' kernels median {med(kern_far):.3f} ms (memsets {ph_far[0]:.3f}, walk {ph_far[1]:.3f}, finish "
            f"{ph_far[2]:.3f}), the residue contacts' {med(rkern_far):.3f} ms (every wave leaves at the sphere test)",
        ]
        if ratio >= 1:
            worst = int(np.argmax(ph))
            lines.append(f"  where the time goes       the largest phase is {('the memsets', 'the walk', 'k_hbond_finish')[worst]} at {ph[worst]:.3f} ms of "
                         f"{med(kern):.3f}; the residue contacts' same phase takes {rph[worst]:.3f} ms")
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
