"""Interface energy of an ensemble of rigid ligand poses - soft Lennard-Jones plus Coulomb with a distance-dependent dielectric over the
heavy-atom pairs within a cutoff: the float64 numpy definition of dfm_pose_iface_energy (include/dfmdock_amd.h, kernels_iface.hip) and
its host finishes.  No reference counterpart.  This is the short physics term docking pipelines re-rank with (ZRANK, HADDOCK,
RosettaDock); here it has no hydrogens, formal charges only, no desolvation, and the cutoff is a plain truncation without a switching
function.

  pose p of the ligand   sterics.pose_atoms
  per pair               everything widened to float64, in exactly this order of operations - no square root (eps = slope * r makes
                         Coulomb a function of r2, LJ is one anyway) and one division per term:
                             r2 = (dx*dx + dy*dy) + dz*dz ;  the pair counts iff r2 < cutoff*cutoff   (strict; NaN is no pair)
                             Rm = rh_a + rh_b ; f = soft*Rm ; r2v = r2 < f*f ? f*f : r2
                             s2 = (Rm*Rm)/r2v ; s6 = (s2*s2)*s2 ; e = se_a*se_b
                             rep = e*(s6*s6) ;  att = -2.0*(e*s6)
                             m = elec_min_dist ; r2c = r2 < m*m ? m*m : r2
                             elec = ((332.0637/dielectric_slope)*(q_a*q_b))/r2c
  quantisation           each term on its own: Q(x) = int64(rint(x * 2^20)), one quantum = 2^-20 kcal/mol, ties to even
  rep_q, att_q, elec_q   [P] int64 sums of the quantised terms; n_pairs [P] int64
  lig_vdw_q, lig_elec_q  [P,Al] int64: rep + att and elec per ligand atom, in the caller's atom order

Integer sums do not depend on their order, so the device's results equal these integer for integer, whatever the blocks and chunks.
Energies in kcal/mol are q * 2^-20 (kcal): equal integers give bitwise equal floats.  A pose with a non-finite transform gets zeros.
"""
from __future__ import annotations

import numpy as np

from . import sterics as ST

CUTOFF = 8.0
SOFT = 0.6
ELEC_MIN_DIST = 3.0
DIELECTRIC_SLOPE = 4.0
COULOMB = 332.0637            # kcal A / (mol e^2)
QUANTA = 1048576.0            # 2^20 per kcal/mol
WEIGHTS = (0.18, 1.0, 0.5)    # total(): repulsion, attraction, electrostatics - ZRANK-like starting values, NOT fitted here
_PAIR_BUDGET = 1 << 20        # atom pairs per broadcast block

# AMBER-style Rmin/2 (A) and epsilon (kcal/mol) by element
LJ = {"C": (1.9080, 0.0860), "N": (1.8240, 0.1700), "O": (1.6612, 0.2100), "S": (2.0000, 0.2500), "SE": (2.0000, 0.2500),
      "P": (2.1000, 0.2000)}
LJ_OTHER = (2.0, 0.2)
# formal charges by (residue, atom)
FORMAL = {("ASP", "OD1"): -0.5, ("ASP", "OD2"): -0.5, ("GLU", "OE1"): -0.5, ("GLU", "OE2"): -0.5, ("LYS", "NZ"): 1.0,
          ("ARG", "NH1"): 0.5, ("ARG", "NH2"): 0.5}


def check_scalars(cutoff=CUTOFF, soft=SOFT, elec_min_dist=ELEC_MIN_DIST, dielectric_slope=DIELECTRIC_SLOPE):
    """The scalars as the device takes them: float32, widened.  ValueError outside the limits of dfm_iface_create: cutoff in (0, 16],
    soft in [0.5, 1], elec_min_dist >= 1, dielectric_slope > 0, all finite."""
    c, s, m, d = (float(np.float32(v)) for v in (cutoff, soft, elec_min_dist, dielectric_slope))
    if not (np.isfinite(c) and 0 < c <= 16):
        raise ValueError(f"cutoff must be in (0, 16], got {cutoff}")
    if not (np.isfinite(s) and 0.5 <= s <= 1):
        raise ValueError(f"soft must be in [0.5, 1], got {soft}")
    if not (np.isfinite(m) and m >= 1):
        raise ValueError(f"elec_min_dist must be finite and >= 1, got {elec_min_dist}")
    if not (np.isfinite(d) and d > 0):
        raise ValueError(f"dielectric_slope must be finite and > 0, got {dielectric_slope}")
    return c, s, m, d


def check_params(params, n, who="params"):
    """Per-atom parameters [n,3] float32 = (rmin_half, sqrt_eps, charge).  ValueError outside the limits of dfm_iface_create:
    rmin_half in (0, 8], sqrt_eps in [0, 2], |charge| <= 4, all finite."""
    p = np.asarray(params, np.float32)
    if p.shape != (n, 3):
        raise ValueError(f"{who} must be [{n},3] (rmin_half, sqrt_eps, charge), got {p.shape}")
    ok = np.isfinite(p).all() and (p[:, 0] > 0).all() and (p[:, 0] <= 8).all() and (p[:, 1] >= 0).all() and (p[:, 1] <= 2).all() \
        and (np.abs(p[:, 2]) <= 4).all()
    if not ok:
        raise ValueError(f"{who}: rmin_half must be in (0, 8], sqrt_eps in [0, 2], |charge| <= 4, all finite")
    return p


def near_r2(rec_atoms, X, cutoff, shortcut=True):
    """Every pair (ligand atom a, receptor atom b) with r2 < cutoff*cutoff, as (a, b, r2) in ligand-major order; X [Al,3] float64 is one
    pose.  The shortcut of sterics.near_pairs: atoms farther than cutoff + 1 A from the other chain's bounding box along an axis are
    dropped before the distances are taken - such a pair is more than cutoff + 1 apart, so nothing below the cutoff is lost.  A pose
    with a non-finite coordinate skips it; `shortcut=False` takes every pair (the test that it changes nothing)."""
    rec = np.asarray(rec_atoms, np.float64).reshape(-1, 3)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    cut2 = float(cutoff) * float(cutoff)
    ia, ib = np.arange(X.shape[0]), np.arange(rec.shape[0])
    if shortcut and np.isfinite(X).all() and np.isfinite(rec).all():
        pad = float(cutoff) + 1.0
        ia = ia[((X >= rec.min(0) - pad) & (X <= rec.max(0) + pad)).all(1)]
        if ia.size:
            ib = ib[((rec >= X[ia].min(0) - pad) & (rec <= X[ia].max(0) + pad)).all(1)]
    out_a, out_b, out_r = [], [], []
    if ia.size and ib.size:
        rb = rec[ib]
        step = max(1, _PAIR_BUDGET // ib.size)
        for lo in range(0, ia.size, step):
            xa = X[ia[lo:lo + step]]
            dx, dy, dz = (xa[:, None, k] - rb[None, :, k] for k in range(3))
            r2 = (dx * dx + dy * dy) + dz * dz
            with np.errstate(invalid="ignore"):
                a, b = np.nonzero(r2 < cut2)
            out_a.append(ia[lo + a])
            out_b.append(ib[b])
            out_r.append(r2[a, b])
    if not out_a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    return np.concatenate(out_a), np.concatenate(out_b), np.concatenate(out_r)


def quantise(x):
    """Q(x) = int64(rint(x * 2^20)): ties to even."""
    return np.rint(np.asarray(x, np.float64) * QUANTA).astype(np.int64)


def pair_terms(r2, par_a, par_b, soft, elec_min_dist, dielectric_slope):
    """(rep_q, att_q, elec_q) int64 of pairs at squared distance r2 [n] float64 with parameters par_a, par_b [n,3] (ligand, receptor):
    the per-pair recipe of the module docstring, operation by operation."""
    r2 = np.asarray(r2, np.float64)
    pa, pb = np.asarray(par_a, np.float32).astype(np.float64), np.asarray(par_b, np.float32).astype(np.float64)
    soft, m, slope = float(soft), float(elec_min_dist), float(dielectric_slope)
    Rm = pa[:, 0] + pb[:, 0]
    f = soft * Rm
    ff = f * f
    r2v = np.where(r2 < ff, ff, r2)
    s2 = (Rm * Rm) / r2v
    s6 = (s2 * s2) * s2
    e = pa[:, 1] * pb[:, 1]
    rep = e * (s6 * s6)
    att = -2.0 * (e * s6)
    mm = m * m
    r2c = np.where(r2 < mm, mm, r2)
    elec = ((COULOMB / slope) * (pa[:, 2] * pb[:, 2])) / r2c
    return quantise(rep), quantise(att), quantise(elec)


def interface_energy(rec_atoms, rec_params, lig_atoms, lig_params, center, rot, tr, cutoff=CUTOFF, soft=SOFT,
                     elec_min_dist=ELEC_MIN_DIST, dielectric_slope=DIELECTRIC_SLOPE, per_atom=False, shortcut=True):
    """The definition.  rec_atoms [Ar,3], lig_atoms [Al,3], *_params [n,3] = (rmin_half, sqrt_eps, charge), center [3], rot [P,3]
    axis-angle, tr [P,3].  Returns {rep_q, att_q, elec_q, n_pairs [P] int64} and, with `per_atom`, lig_vdw_q / lig_elec_q [P,Al] int64."""
    c, s, m, d = check_scalars(cutoff, soft, elec_min_dist, dielectric_slope)
    rec = np.asarray(rec_atoms, np.float32).reshape(-1, 3)
    lig = np.asarray(lig_atoms, np.float32).reshape(-1, 3)
    rp, lp = check_params(rec_params, rec.shape[0], "rec_params"), check_params(lig_params, lig.shape[0], "lig_params")
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    if rot.shape != tr.shape:
        raise ValueError(f"rot and tr must both be [P,3], got {rot.shape} and {tr.shape}")
    P, Al = rot.shape[0], lig.shape[0]
    out = {k: np.zeros(P, np.int64) for k in ("rep_q", "att_q", "elec_q", "n_pairs")}
    if per_atom:
        out["lig_vdw_q"], out["lig_elec_q"] = np.zeros((P, Al), np.int64), np.zeros((P, Al), np.int64)
    for p in range(P):
        if not (np.isfinite(rot[p]).all() and np.isfinite(tr[p]).all()):
            continue
        a, b, r2 = near_r2(rec, ST.pose_atoms(lig, center, rot[p], tr[p]), c, shortcut)
        rep, att, elec = pair_terms(r2, lp[a], rp[b], s, m, d)
        out["rep_q"][p], out["att_q"][p], out["elec_q"][p], out["n_pairs"][p] = rep.sum(), att.sum(), elec.sum(), r2.size
        if per_atom:
            np.add.at(out["lig_vdw_q"][p], a, rep + att)
            np.add.at(out["lig_elec_q"][p], a, elec)
    return out


def kcal(q):
    """Quanta -> kcal/mol (float64; exact for |q| < 2^53)."""
    return np.asarray(q, np.int64).astype(np.float64) / QUANTA


def total(rep, att, elec, weights=WEIGHTS):
    """The weighted sum (w_rep rep + w_att att) + w_elec elec of the three terms in kcal/mol, float64.  The default weights 0.18 / 1.0 /
    0.5 are ZRANK-like starting values: they are NOT fitted here, and nothing about ranking quality is claimed for them without a
    trained checkpoint to evaluate the whole pipeline with."""
    w = np.asarray(weights, np.float64).reshape(-1)
    if w.size != 3 or not np.isfinite(w).all():
        raise ValueError(f"weights must be three finite numbers (rep, att, elec), got {weights}")
    rep, att, elec = (np.asarray(v, np.float64) for v in (rep, att, elec))
    return (w[0] * rep + w[1] * att) + w[2] * elec


def element_of(atom):
    """Element symbol (upper case) of a pdbio.read_pdb record: the element column, else the leading letters of the name (SE of a
    selenomethionine's SE, else the first letter)."""
    el = atom.get("element", "").strip().upper()
    if el:
        return el
    name = atom["name"].strip().upper().lstrip("0123456789")
    return "SE" if name.startswith("SE") else name[:1]


def atom_parameters(atoms, heavy_index=None):
    """[n,3] float32 (rmin_half, sqrt_eps, charge) of the atoms `heavy_index` (default: sterics.heavy_atoms) of pdbio.read_pdb records.
    LJ by element (LJ, LJ_OTHER); sqrt_eps = sqrt(eps) in float64, rounded to float32.  Formal charges: FORMAL, +1 on the N of each
    chain's first residue, -0.5 on O and on OXT of a residue that has an OXT, 0 elsewhere."""
    index = ST.heavy_atoms(atoms) if heavy_index is None else np.asarray(heavy_index, np.int64)
    key = lambda a: (a["chain"], a["res_id"], a["ins"], a["res_name"])
    first, with_oxt = {}, set()
    for i in index:
        a = atoms[int(i)]
        first.setdefault(a["chain"], key(a))
        if a["name"] == "OXT":
            with_oxt.add(key(a))
    out = np.zeros((index.size, 3), np.float32)
    for n, i in enumerate(index):
        a = atoms[int(i)]
        rh, eps = LJ.get(element_of(a), LJ_OTHER)
        q = FORMAL.get((a["res_name"], a["name"]), 0.0)
        if a["name"] == "N" and first[a["chain"]] == key(a):
            q = 1.0
        if a["name"] in ("O", "OXT") and key(a) in with_oxt:
            q = -0.5
        out[n] = (rh, np.sqrt(np.float64(eps)), q)
    return out


def residue_energy(per_atom, res, n_res):
    """Per-atom quanta [.., n] summed per residue -> [.., n_res] int64 (sterics.residue_counts)."""
    return ST.residue_counts(per_atom, res, n_res)


def write_energy_residues(path, keys, vdw, elec):
    """--energy-residues: one line `chain:resnum[icode] res_name vdw elec` (kcal/mol, unweighted) per ligand residue with a nonzero sum."""
    with open(path, "w") as f:
        f.write("# ligand residue, name, soft LJ (rep + att) and Coulomb interface energy in kcal/mol, unweighted\n")
        for k, v, e in zip(keys, vdw, elec):
            if v != 0 or e != 0:
                f.write(f"{k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''} {k[3]} {float(kcal(v)):.6f} {float(kcal(e)):.6f}\n")
