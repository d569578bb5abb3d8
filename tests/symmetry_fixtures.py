"""Inputs of the symmetry tests, written by the tests themselves: a monomer as two PDB files (A.pdb and A2.pdb, the same chain moved
by a whole number of milli-Angstrom, so that the file's three decimals hold an exact rigid image), a third file of another sequence
on the same backbone, and the features of the pair."""
import os

import numpy as np

SEQ = "MKTAYIAKQRQISFVKSHFSRQLE"        # 24 residues
SEQ_OTHER = "MKTAYIAKQRGISFVKSHFSRQLE"  # one residue differs


def monomer():
    """(features [24,1301], backbone [24,3,3] rounded to the PDB format's three decimals) of the 24-residue synthetic receptor."""
    from dfmdock_amd.synthetic import make_complex, seq_to_onehot
    cx = make_complex(24, 16, seed=5)
    x = np.concatenate([np.asarray(cx["rec_x"], np.float32)[:, :1280], seq_to_onehot(SEQ)], 1)
    return x, np.round(np.asarray(cx["rec_pos"], np.float64), 3)


def _write_chain(path, bb, seq, chain, shift=(0.0, 0.0, 0.0)):
    """N, CA, C, O, CB per residue (CB skipped for GLY) through pdbio.write_complex_pdb; every coordinate a multiple of 0.001."""
    from dfmdock_amd import pdbio
    full = np.round(np.asarray(pdbio.full_backbone(bb), np.float64), 3) + np.asarray(shift, np.float64)
    atoms, coords = [], []
    for r, res in enumerate(full):
        for name, xyz in zip(("N", "CA", "C", "O", "CB"), res):
            if name == "CB" and seq[r] == "G":
                continue
            atoms.append({"hetero": False, "name": name, "res_name": pdbio.ONE_TO_THREE[seq[r]], "chain": chain, "res_id": r + 1, "ins": " ",
                          "coord": tuple(xyz), "element": name[0]})
            coords.append(xyz)
    pdbio.write_complex_pdb(path, [], atoms, np.asarray(coords))
    return path


def write_homodimer(tmp, shift=(30.0, -4.0, 7.0)):
    """A.pdb (chain A), A2.pdb (chain B: the same atoms shifted), features.npz and other.pdb (A2 with one residue renamed)."""
    x, bb = monomer()
    a = _write_chain(os.path.join(tmp, "A.pdb"), bb, SEQ, "A")
    a2 = _write_chain(os.path.join(tmp, "A2.pdb"), bb, SEQ, "B", shift)
    other = _write_chain(os.path.join(tmp, "other.pdb"), bb, SEQ_OTHER, "B", shift)
    feat = os.path.join(tmp, "features.npz")
    np.savez(feat, rec_esm=x[:, :1280], lig_esm=x[:, :1280])
    return a, a2, feat, other


# ---------------------------------------------------------------------------------------------------------------------------------
# homodimers of the GPU tests and of tools/symmetry_bench.py: the builders, the evaluation poses and the check against the definition
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def receptor(size):
    """(features [M,1301], backbone [M,3,3] float32) of the receptor of an existing case: synthetic 9 / 24 / 300 residues, or "7CEI"."""
    from dfmdock_amd.synthetic import make_complex, seq_to_onehot
    if size == "7CEI":
        d = np.load(os.path.join(GOLDEN, "cx_7CEI.npz"), allow_pickle=False)
        return np.concatenate([d["rec_esm16"].astype(F32), seq_to_onehot(str(d["rec_seq"]))], 1).astype(F32), np.asarray(d["rec_pos"], F32)
    cx = make_complex(size, size, seed={9: 6, 24: 5, 300: 1}[size])
    return np.asarray(cx["rec_x"], F32), np.asarray(cx["rec_pos"], F32)


def turn(y, theta, u, point, screw=0.0):
    """y turned by theta about the axis (point, u) and shifted by screw along it, float64."""
    from dfmdock_amd.restraints import axis_angle_to_matrix
    y = np.asarray(y, np.float64)
    u = np.asarray(u, np.float64) / np.linalg.norm(u)
    return (y - point) @ axis_angle_to_matrix(theta * u).T + point + screw * u


def outside_point(y, d, gap):
    """A point `gap` A outside the chain in direction d from its centroid."""
    a = np.asarray(y, np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d)
    c = a.mean(0)
    return c + d * (((a - c) @ d).max() + gap)


def homodimer(model, size, n=3):
    """(engine.Complex, receptor backbone, start pose) of a homodimer: the receptor's features on both sides, the ligand the receptor
    turned by 2 pi / n + 0.4 about an axis 4 A outside the chain."""
    from dfmdock_amd import engine
    x, y = receptor(size)
    p = outside_point(y, np.array([1.0, 0.3, -0.2]), 4.0)
    lig0 = turn(y, 2 * np.pi / n + 0.4, np.array([0.2, -0.5, 1.0]), p, 1.5).astype(F32)
    return engine.Complex(model, x, x, y, lig0), y, lig0


def exact_translation(y):
    """y shifted by a translation that fp32 holds exactly for every coordinate, so that the fitted rotation is the identity to float64
    rounding and not to fp32 rounding (which would be an axis of ~1e-7 rad, far above the no-axis threshold)."""
    y = np.asarray(y, F32)
    for t in ([16.0, -8.0, 4.0], [1.0, -0.5, 0.25], [2.0 ** -6, -2.0 ** -7, 2.0 ** -8], [-2.0 ** -8, -2.0 ** -9, -2.0 ** -10],
              [2.0 ** -10, 2.0 ** -10, 2.0 ** -10], [-2.0 ** -10, 2.0 ** -11, -2.0 ** -10], [2.0 ** -12, -2.0 ** -12, 2.0 ** -12],
              [-2.0 ** -13, 2.0 ** -13, 2.0 ** -12]):
        x = y + F32(t)
        if np.array_equal(x.astype(np.float64), y.astype(np.float64) + np.asarray(t)):
            return x
    return y.copy()


def poses(y, n, B, rng):
    """B rigid poses of the chain y: theta in [0.05, pi - 0.05] about random axes a few A outside the chain with random screws, and
    the special ones: [0] exactly symmetric (m = 1), [1] theta = pi exactly (n = 2: symmetric as well), [2] one whose step clips
    (25 A of screw, 0.9 rad off), [3] one that does not (0.1 rad, 1 A), [4] a pure translation (no axis), [5] NaN.
    Returns float32 [B,M,3,3]."""
    out = np.empty((B,) + y.shape, F32)
    for b in range(B):
        d, u = rng.standard_normal(3), rng.standard_normal(3)
        p = outside_point(y, d, rng.uniform(2.0, 8.0))
        theta, screw = rng.uniform(0.05, np.pi - 0.05), 3.0 * rng.standard_normal()
        if b == 0:
            theta, screw = 2 * np.pi / n, 0.0
        elif b == 1:
            theta, screw = np.pi, 0.0 if n == 2 else 2.0
        elif b == 2:
            theta, screw = (2 * np.pi / n - 0.9 if n <= 4 else 2 * np.pi / n + 0.9), 25.0
        elif b == 3:
            theta, screw = 2 * np.pi / n + (-0.1 if n == 2 else 0.1), 1.0
        out[b] = turn(y, theta, u, p, screw).astype(F32)
    out[4] = exact_translation(y)
    out[5, len(y) // 2, 1, 2] = np.nan
    return out


def ulp32(v):
    return float(np.spacing(F32(abs(v))))


def device_step(ev, b, n, p32):
    """The step recomputed in float64 from the device's own float64 outputs of pose b, in the kernel's operation order: gains, then
    clip(v, m) = v m / |v| where |v| > m."""
    m = int(ev["order_m"][b])
    if m == 0:
        return np.zeros(6)
    u, theta, screw = ev["axis"][b], float(ev["theta"][b]), float(ev["screw"][b])
    ts = 2.0 * 3.14159265358979323846 * float(m) / float(n)
    st = np.concatenate([-p32.gain_tr * screw * u, p32.gain_rot * (ts - theta) * u])
    for h, mx in ((0, p32.max_tr), (1, p32.max_rot)):
        v = st[h * 3:h * 3 + 3]
        nn = float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
        if nn > mx:
            st[h * 3:h * 3 + 3] = v * (mx / nn)
    return st


def check_eval(ev, y, poses_, n, params, center="ca"):
    """dfm_symmetry_eval of every pose against symmetry.evaluate: order_m exact; theta within 1e-11 rad, axis 1e-10, screw, axis_point,
    fit_rmsd, sym_rmsd 1e-8 A; every component of the fp32 step within 2 fp32 ulp, taken at that 3-vector's largest component, of
    device_step.  Returns the worst deviations (step in ulp, over EVERY finite pose) and the clip decisions of the definition."""
    from dfmdock_amd import symmetry as SY
    p32 = SY.SymmetryParams(**{k: float(F32(getattr(params, k))) for k in ("gain_rot", "gain_tr", "max_rot", "max_tr", "t_start")},
                            snap_last=params.snap_last)
    worst = {k: 0.0 for k in ("theta", "axis", "screw", "axis_point", "fit_rmsd", "sym_rmsd", "step_ulp")}
    clipped = []
    for b in range(len(poses_)):
        e = SY.evaluate(y, poses_[b], n, p32, center)
        if not np.isfinite(poses_[b]).all():
            assert ev["order_m"][b] == 0 and np.isnan(ev["step"][b]).all(), b
            for k in ("theta", "screw", "axis", "axis_point", "fit_rmsd", "sym_rmsd"):
                assert np.isnan(ev[k][b]).all(), (b, k)
            clipped.append((False, False))
            continue
        assert int(ev["order_m"][b]) == e["m"], (b, ev["order_m"][b], e["m"])
        for k, gate in (("theta", 1e-11), ("axis", 1e-10), ("screw", 1e-8), ("axis_point", 1e-8), ("fit_rmsd", 1e-8), ("sym_rmsd", 1e-8)):
            got, want = np.asarray(ev[k][b], np.float64), np.asarray(e[k], np.float64)
            assert (np.isnan(got) == np.isnan(want)).all(), (b, k, got, want)
            if np.isnan(want).all():
                continue
            dev = float(np.abs(got - want).max())
            worst[k] = max(worst[k], dev)
            assert dev <= gate, (b, k, dev, got, want)
        want = device_step(ev, b, n, p32)
        for h in (0, 1):
            w3 = want[h * 3:h * 3 + 3]
            ulp = ulp32(np.abs(w3).max())
            dev = float(np.abs(ev["step"][b, h * 3:h * 3 + 3].astype(np.float64) - w3).max())
            worst["step_ulp"] = max(worst["step_ulp"], dev / ulp)
            assert dev <= 2 * ulp, (b, h, dev, ulp, ev["step"][b], w3)
        if e["m"] == 0:
            clipped.append((False, False))
            continue
        # the definition's own step agrees as far as its theta and screw do (their gates times the gain), clip decision included
        assert np.abs(want[:3] - e["step"][:3]).max() <= p32.gain_tr * 1e-8 and np.abs(want[3:] - e["step"][3:]).max() <= p32.gain_rot * 1e-11, b
        s, dth = e["screw"], e["theta_star"] - e["theta"]
        clipped.append((abs(p32.gain_tr * s) > p32.max_tr, abs(p32.gain_rot * dth) > p32.max_rot))
    return worst, np.array(clipped)


def closure(y, pose, n, center="ca"):
    """(closure under T^n, |theta - theta*|, |screw|) of one pose by the float64 definition."""
    from dfmdock_amd import symmetry as SY
    e = SY.evaluate(y, pose, n, center=center)
    return SY.closure(y, e["Q"], e["tau"], n), abs(e["theta"] - e["theta_star"]), abs(e["screw"])
