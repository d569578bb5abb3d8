"""All-atom clash and contact screen of an ensemble of rigid ligand poses: the float64 numpy definition of dfm_pose_sterics
(include/dfmdock_amd.h, kernels_sterics.hip) and its host finishes.  No reference counterpart: the reference carries the side chains
along on the host (modify_aa_coords, src/inference_base.py:354-364) and never looks at them.

CAPRI's assessment rule is the standard one: a clash is a pair of non-hydrogen atoms of the two chains closer than 3.0 A, a model whose
clash count exceeds the ensemble's mean by more than two standard deviations is disqualified, and the interface size is counted the same
way as atom pairs closer than 5 A.

  pose p of the ligand   (lig - center) @ R(rot_p).T + center + tr_p, everything widened to float64, R = pdbio.axis_angle_to_matrix:
                         pdbio.apply_pose_all_atom with the centre made explicit (the CA centroid for family 0, the all-atom mean for
                         family 1); rot / tr are what dfm_traj_out.rot_update / tr_update hold
  distance of a pair     d = sqrt((dx*dx + dy*dy) + dz*dz) in float64
  n_clash[p]             pairs (receptor atom, ligand atom) with d < clash_cutoff (strict)
  n_contact[p]           pairs with d < contact_cutoff (>= clash_cutoff)
  min_dist[p]            the smallest d among the pairs with d < contact_cutoff, +inf without one
  lig_clash / lig_contact [p,a]   the same counts for each ligand atom

A NaN distance is neither a clash nor a contact: a pose with a NaN transform gets 0, 0 and +inf.  The atoms are heavy atoms; the caller
filters hydrogens (heavy_atoms).
"""
from __future__ import annotations

import numpy as np

from . import pdbio

CLASH_CUTOFF = 3.0
CONTACT_CUTOFF = 5.0
_PAIR_BUDGET = 1 << 21      # atom pairs per broadcast block of near_pairs


def pose_atoms(lig_atoms, center, rot, tr):
    """One pose of the ligand atoms, [Al,3] float64: (lig - center) @ R(rot).T + center + tr."""
    R = pdbio.axis_angle_to_matrix(np.asarray(rot).reshape(3))
    return (np.asarray(lig_atoms, np.float64) - np.asarray(center, np.float64).reshape(3)) @ R.T \
        + np.asarray(center, np.float64).reshape(3) + np.asarray(tr, np.float64).reshape(3)


def near_pairs(rec_atoms, X, reach):
    """Every pair (ligand atom a, receptor atom b) with d < reach, as (a, b, d) in ligand-major order; X [Al,3] float64 is one pose.
    Atoms farther than reach + 1 A from the other chain's bounding box along an axis are dropped before the distances are taken: such
    a pair has d > reach + 1, so nothing that can be below `reach` is lost.  A pose with a non-finite coordinate skips the shortcut."""
    rec = np.asarray(rec_atoms, np.float64).reshape(-1, 3)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    ia, ib = np.arange(X.shape[0]), np.arange(rec.shape[0])
    if np.isfinite(X).all() and np.isfinite(rec).all():
        pad = float(reach) + 1.0
        ia = ia[((X >= rec.min(0) - pad) & (X <= rec.max(0) + pad)).all(1)]
        if ia.size:
            ib = ib[((rec >= X[ia].min(0) - pad) & (rec <= X[ia].max(0) + pad)).all(1)]
    out_a, out_b, out_d = [], [], []
    if ia.size and ib.size:
        rb = rec[ib]
        step = max(1, _PAIR_BUDGET // ib.size)
        for lo in range(0, ia.size, step):
            xa = X[ia[lo:lo + step]]
            dx, dy, dz = (xa[:, None, k] - rb[None, :, k] for k in range(3))
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
            with np.errstate(invalid="ignore"):
                a, b = np.nonzero(d < reach)
            out_a.append(ia[lo + a])
            out_b.append(ib[b])
            out_d.append(d[a, b])
    if not out_a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    return np.concatenate(out_a), np.concatenate(out_b), np.concatenate(out_d)


def check_cutoffs(clash_cutoff, contact_cutoff):
    """The cutoffs as the device takes them: float32, widened.  ValueError unless finite, > 0 and contact >= clash."""
    cc, ct = float(np.float32(clash_cutoff)), float(np.float32(contact_cutoff))
    if not (np.isfinite(cc) and np.isfinite(ct) and cc > 0 and ct > 0 and ct >= cc):
        raise ValueError(f"cutoffs must be finite and > 0 with contact >= clash, got clash {clash_cutoff}, contact {contact_cutoff}")
    return cc, ct


def sterics(rec_atoms, lig_atoms, center, rot, tr, clash_cutoff=CLASH_CUTOFF, contact_cutoff=CONTACT_CUTOFF, per_atom=False):
    """The definition.  rec_atoms [Ar,3], lig_atoms [Al,3], center [3], rot [P,3] axis-angle, tr [P,3].  Returns {n_clash [P] int32,
    n_contact [P] int32, min_dist [P] float64} and, with `per_atom`, lig_clash / lig_contact [P,Al] int32."""
    cc, ct = check_cutoffs(clash_cutoff, contact_cutoff)
    rec = np.asarray(rec_atoms, np.float32).reshape(-1, 3)
    lig = np.asarray(lig_atoms, np.float32).reshape(-1, 3)
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    if rot.shape != tr.shape:
        raise ValueError(f"rot and tr must both be [P,3], got {rot.shape} and {tr.shape}")
    P, Al = rot.shape[0], lig.shape[0]
    out = {"n_clash": np.zeros(P, np.int32), "n_contact": np.zeros(P, np.int32), "min_dist": np.full(P, np.inf, np.float64)}
    if per_atom:
        out["lig_clash"], out["lig_contact"] = np.zeros((P, Al), np.int32), np.zeros((P, Al), np.int32)
    for p in range(P):
        a, _, d = near_pairs(rec, pose_atoms(lig, center, rot[p], tr[p]), ct)
        clash = d < cc
        out["n_clash"][p], out["n_contact"][p] = int(clash.sum()), d.size
        if d.size:
            out["min_dist"][p] = d.min()
        if per_atom:
            out["lig_clash"][p] = np.bincount(a[clash], minlength=Al)
            out["lig_contact"][p] = np.bincount(a, minlength=Al)
    return out


def capri_flags(n_clash, members=None):
    """CAPRI's disqualification rule: thr = mean + 2 std of the member poses' clash counts (population std, ddof 0); a pose - member or
    not - is flagged when n_clash > thr.  Returns (flags [P] bool, thr, mean, std); with fewer than two members nothing is flagged and
    thr is +inf (mean / std: of the members there are, NaN without any)."""
    n = np.asarray(n_clash, np.float64).reshape(-1)
    m = np.ones(n.size, bool) if members is None else np.asarray(members).reshape(-1).astype(bool)
    if m.size != n.size:
        raise ValueError(f"members must have {n.size} entries, got {m.size}")
    k = int(m.sum())
    mean, std = (float(n[m].mean()), float(n[m].std())) if k else (float("nan"), float("nan"))
    if k < 2:
        return np.zeros(n.size, bool), float("inf"), mean, std
    thr = mean + 2.0 * std
    return n > thr, thr, mean, std


def is_hydrogen(atom):
    """A pdbio.read_pdb record: element H or D, or - with an empty element column - a name that starts with H or with a digit followed
    by H (1HB, 2HG1)."""
    el = atom.get("element", "").strip().upper()
    if el:
        return el in ("H", "D")
    name = atom["name"].strip().upper()
    return name[:1] == "H" or (len(name) > 1 and name[0].isdigit() and name[1] == "H")


def heavy_atoms(atoms):
    """Indices (into `atoms`, pdbio.read_pdb records) of the atoms the screen counts: no hydrogens, no HETATM (as
    pdbio.backbone_from_atoms drops them)."""
    return np.array([i for i, a in enumerate(atoms) if not a["hetero"] and not is_hydrogen(a)], np.int64)


def residue_of_atoms(atoms, index=None):
    """(keys, res) of the atoms `index` (default: all) of pdbio.read_pdb records: keys = the (chain, res_id, ins, res_name) of every
    residue in order of first appearance, res [n] = the position of each atom's residue in keys."""
    index = np.arange(len(atoms)) if index is None else np.asarray(index, np.int64)
    keys, pos, res = [], {}, np.zeros(index.size, np.int64)
    for n, i in enumerate(index):
        a = atoms[int(i)]
        key = (a["chain"], a["res_id"], a["ins"], a["res_name"])
        if key not in pos:
            pos[key] = len(keys)
            keys.append(key)
        res[n] = pos[key]
    return keys, res


def residue_counts(per_atom, res, n_res):
    """Per-atom counts [.., n] summed per residue -> [.., n_res]."""
    per_atom = np.asarray(per_atom)
    out = np.zeros(per_atom.shape[:-1] + (n_res,), np.int64)
    np.add.at(out, (Ellipsis, res), per_atom)
    return out


def write_clash_residues(path, keys, clash, contact):
    """--clash-residues: one line `chain:resnum[icode] res_name n_clash n_contact` per ligand residue with a contact."""
    with open(path, "w") as f:
        f.write("# ligand residue, name, atom pairs closer than the clash cutoff, atom pairs closer than the contact cutoff\n")
        for k, c, t in zip(keys, clash, contact):
            if t > 0:
                f.write(f"{k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''} {k[3]} {int(c)} {int(t)}\n")
