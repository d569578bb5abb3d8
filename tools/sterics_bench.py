"""Poses per second of the all-atom clash / contact screen on the GPU (dfm_pose_sterics) against the float64 numpy definition
(dfmdock_amd/sterics.py) on the same host: 10 240 rigid poses of the 300 + 300 complex at 8 heavy atoms per residue.  Writes
profiles/sterics.txt.

    python tools/sterics_bench.py [--out profiles/sterics.txt] [--reps 7] [--host-poses 64]

The atoms: N, CA, C, O and the virtual CB of pdbio.full_backbone plus three side-chain pseudo-atoms per residue on the CA -> CB ray, 1.5,
3.0 and 4.5 A beyond CB, each moved by a seeded N(0, 0.3^2) A per axis - 2 400 + 2 400 atoms at about a protein's density.  The poses:
the spread of tools/consensus_bench.py, scales 0 ... 1 of a rotation vector s N(0,1)^3 rad about the CA centroid and a translation
N(0, (10 s)^2) A per axis, handed over as (rot, tr): 24 bytes per pose.

GPU: warm-up calls, then `reps` timed calls; wall time of the whole call (upload, kernels, download, CAPRI's rule on the host) from a host
clock, copy and kernel time from the call's own HIP events (dfm_sterics_last_timing); median and min-max.  The fractions of waves that
leave at the sphere and at the box test come from one further, untimed call with the exit counters on (dfm_sterics_exit_counts).  The
definition is timed on the first `host-poses` poses and scaled linearly to P (labelled as scaled).  Before any time is printed the timed
call's results on that subset are asserted against the definition (per-atom counts within each atom's border pairs, 1e-3 A).

Two floors, computed here, both lower bounds of what the kernels must do.  Bytes: every wave reads its pose (96 bytes) and its block's
sphere (16 bytes), a wave that stays reads its 64 atoms (1 KiB); the 38 KiB of receptor atoms stay in cache - over the 8 TB/s HBM figure.
Float64 work: 24 operations per atom a staying wave transforms and 9 per pair below the contact cutoff (3 subtractions, 3
multiplications, 2 additions, 1 square root counted as one), over the MI355X data sheet's vector fp64 peak of 78.6 TFLOP/s."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12
FP64_FLOPS = 78.6e12
BORDER = 1e-3


def eight_atoms(bb, rng):
    from dfmdock_amd import pdbio
    five = pdbio.full_backbone(bb).astype(np.float64)
    ray = five[:, 4] - five[:, 1]
    ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
    side = [five[:, 4] + k * 1.5 * ray + 0.3 * rng.standard_normal(ray.shape) for k in (1, 2, 3)]
    return np.concatenate([five, np.stack(side, 1)], 1).reshape(-1, 3).astype(np.float32)


def make_case(R, L, P, seed):
    from dfmdock_amd.synthetic import make_complex
    cx = make_complex(R, L, seed=seed)
    rng = np.random.default_rng(seed)
    rec, lig = eight_atoms(cx["rec_pos"], rng), eight_atoms(cx["lig_pos"], rng)
    cen = np.asarray(cx["lig_pos"], np.float64)[:, 1].mean(0).astype(np.float32)
    s = ((np.arange(P) % 16) / 15.0)[:, None]
    rot = (s * rng.standard_normal((P, 3))).astype(np.float32)
    tr = (10.0 * s * rng.standard_normal((P, 3))).astype(np.float32)
    return rec, lig, cen, rot, tr


def check_subset(got, rec, lig, cen, rot, tr, n):
    """The sanity condition: the call's per-atom counts on the first n poses against the definition, border pairs aside."""
    from dfmdock_amd import sterics as ST
    clash = contact = border = 0
    for p in range(n):
        a, _, d = ST.near_pairs(rec, ST.pose_atoms(lig, cen, rot[p], tr[p]), 5.0 + BORDER)
        for key, cut in (("lig_clash", 3.0), ("lig_contact", 5.0)):
            want, edge = np.bincount(a[d < cut], minlength=lig.shape[0]), np.bincount(a[np.abs(d - cut) < BORDER], minlength=lig.shape[0])
            assert (np.abs(got[key][p] - want) <= edge).all(), (key, p)
            border += int(edge.sum())
        clash += int((d < 3.0).sum())
        contact += int((d < 5.0).sum())
    return clash, contact, border


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sterics.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=64, help="poses the numpy definition is timed on (scaled linearly to P)")
    a = ap.parse_args()
    from dfmdock_amd import engine
    from dfmdock_amd import sterics as ST
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["all-atom clash / contact screen: GPU call (dfm_pose_sterics) vs the float64 numpy definition (sterics.sterics)", engine.config_string()]
    med = lambda v: float(np.median(v))
    for name, R, L, P, seed in [("C3 ensemble", 300, 300, 10240, 1)]:
        rec, lig, cen, rot, tr = make_case(R, L, P, seed)
        n = min(a.host_poses, P)
        t0 = time.perf_counter()
        ST.sterics(rec, lig, cen, rot[:n], tr[:n])
        host_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        at = model.atoms(rec, lig, cen)
        create_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(2):
            at.sterics(rot, tr)
        wall, copy, kern = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            o = at.sterics(rot, tr)
            wall.append((time.perf_counter() - t0) * 1e3)
            c, k = engine.sterics_last_timing()
            copy.append(c)
            kern.append(k)
        engine.sterics_exit_counts(True)
        counted = at.sterics(rot, tr)
        waves, at_sphere, at_box = engine.sterics_exit_counts(False)
        sub = at.sterics(rot[:n], tr[:n], per_atom=True)
        for key in ("n_clash", "n_contact", "min_dist"):
            assert np.array_equal(o[key], counted[key]) and np.array_equal(o[key][:n], sub[key]), key
        clash, contact, border = check_subset(sub, rec, lig, cen, rot, tr, n)
        info = at.info()
        at.close()
        stay = waves - at_sphere - at_box
        pairs = P * rec.shape[0] * lig.shape[0]
        byte_ms = (waves * 112 + stay * 1024) / HBM_BPS * 1e3
        flop_ms = (stay * 64 * 24 + int(o["n_contact"].sum(dtype=np.int64)) * 9) / FP64_FLOPS * 1e3
        lines += [
            f"{name}: R = {R}, L = {L} residues at 8 heavy atoms = {rec.shape[0]} + {lig.shape[0]} atoms, P = {P}; grid of {info['n_cells']} cells of "
            f"{info['cell_edge']:g} A, at most {info['max_cell_atoms']} atoms in one; {int(o['n_clash'].sum(dtype=np.int64))} clash and "
            f"{int(o['n_contact'].sum(dtype=np.int64))} contact pairs in {pairs} atom pairs, {int((o['n_contact'] == 0).sum())} poses without a contact, "
            f"{int(o['flags'].sum())} flagged (threshold {o['threshold']:.1f} clashes); checked against the definition on {n} poses ({clash} clash, "
            f"{contact} contact, {border} border pairs)",
            f"  numpy definition, 1 core  {n / host_ms * 1e3:10.1f} poses/s   {host_ms:.0f} ms for {n} poses = {host_ms * P / n:.0f} ms for P poses (scaled)",
            f"  dfm_atoms_create          {create_ms:.2f} ms once (counting sort, Morton sort, 5 uploads)",
            f"  GPU call, wall            {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls"
            f" = {host_ms * P / n / med(wall):.0f} x the scaled definition",
            f"  of which host-to-device   median {med(copy):.3f} ms ({100 * med(copy) / med(wall):.0f} % of wall; {P * 24} bytes of poses)",
            f"  of which kernels          median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}) = {pairs / med(kern) / 1e6:.1f} G atom pairs/s nominal",
            f"  early exits               {waves} waves: {100 * at_sphere / waves:.1f} % leave at the sphere test, {100 * at_box / waves:.1f} % at the box test, "
            f"{100 * stay / waves:.1f} % walk cells",
            f"  floors                    bytes {byte_ms:.4f} ms at 8 TB/s ({100 * byte_ms / med(kern):.1f} % of the kernel time); float64 "
            f"{flop_ms:.4f} ms at 78.6 TFLOP/s ({100 * flop_ms / med(kern):.2f} %): the kernels are bound by "
            f"{'neither: the float32 reject over the staged receptor atoms of the waves that stay dominates' if max(byte_ms, flop_ms) < 0.5 * med(kern) else ('bytes' if byte_ms > flop_ms else 'float64 work')}",
        ]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
