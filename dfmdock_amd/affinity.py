"""Residue contacts by class and a contacts-based binding-affinity estimate of an ensemble of rigid ligand poses: the float64 numpy
definition of dfm_pose_rescon (include/dfmdock_amd.h, kernels_rescon.hip) and its host finishes.  No reference counterpart.

  pose p of the ligand   sterics.pose_atoms
  distance of a pair     d = sqrt((dx*dx + dy*dy) + dz*dz) in float64 (sterics.py); an atom pair counts iff d < cutoff (strict; the cutoff
                         is a float32, widened; a NaN is no pair)
  C_p                    the SET of (receptor residue i, ligand residue j) with at least one counting atom pair: a residue pair with
                         twelve atom pairs is one member
  ic [P,6] int32         |C_p| split by the unordered pair of residue classes (0 apolar, 1 polar, 2 charged) in the order AA, AP, AC, PP,
                         PC, CC: index a*(5-a)/2 + b for classes a <= b
  n_pairs [P] int32      |C_p| = ic.sum(1)
  n_rec_res, n_lig_res   [P] int32: residues of each chain with at least one contact
  rec_degree [P,Rr], lig_degree [P,Lr] int32   the number of partner residues (per_residue)
  contact_bits [P,Lr,W] uint32, W = ceil(Rr/32)   bit i & 31 of word i >> 5 of row j is set iff (i, j) is in C_p (bits)

Everything is an integer, so the device's arrays equal these, whatever the waves, blocks and chunks.  A pose with a non-finite transform
gets zeros.  A residue without atoms is legal and never in contact.

The host finishes are the contacts-based affinity predictor IC-NIS (PRODIGY; Vangone & Bonvin, eLife 2015): a linear model over the
interfacial contacts by class and the composition of the non-interacting surface.  COEF, IC_CLASS, NIS_CLASS and REF_ASA were written
down from the publications without the published tool at hand to check them against: they are starting values of overridable arguments,
NOT verified.  The surface that feeds the model here is this project's own 128-point Shrake-Rupley with its own element radii
(surface.py), not the surface program of the published tool.  No agreement with the PRODIGY server's numbers is claimed or tested, and
nothing is calibrated.
"""
from __future__ import annotations

import numpy as np

from . import sterics as ST

CUTOFF = 5.5
MAX_RES = 4096              # residues per chain (dfm_rescon_create)
MAX_POSES = 65536           # poses per call (dfm_pose_rescon)
_PAIR_BUDGET = 1 << 21      # atom pairs per broadcast block of the shortcut-free path

APOLAR, POLAR, CHARGED = 0, 1, 2
_A, _P, _C = APOLAR, POLAR, CHARGED
# residue classes of the interfacial contacts, by three-letter name
IC_CLASS = {"ASP": _C, "GLU": _C, "LYS": _C, "ARG": _C, "HIS": _C,
            "ASN": _P, "GLN": _P, "SER": _P, "THR": _P,
            "ALA": _A, "CYS": _A, "GLY": _A, "PHE": _A, "ILE": _A, "MET": _A, "LEU": _A, "PRO": _A, "TRP": _A, "VAL": _A, "TYR": _A}
# residue classes of the non-interacting surface
NIS_CLASS = {"ASP": _C, "GLU": _C, "LYS": _C, "ARG": _C,
             "CYS": _P, "HIS": _P, "ASN": _P, "GLN": _P, "SER": _P, "THR": _P, "TRP": _P, "TYR": _P,
             "ALA": _A, "GLY": _A, "PHE": _A, "ILE": _A, "MET": _A, "LEU": _A, "PRO": _A, "VAL": _A}
# theoretical maximum accessible surface area per residue in A^2 (Tien et al., PLoS ONE 2013)
REF_ASA = {"ALA": 129.0, "ARG": 274.0, "ASN": 195.0, "ASP": 193.0, "CYS": 167.0, "GLN": 225.0, "GLU": 223.0, "GLY": 104.0, "HIS": 224.0,
           "ILE": 197.0, "LEU": 201.0, "LYS": 236.0, "MET": 224.0, "PHE": 240.0, "PRO": 159.0, "SER": 155.0, "THR": 172.0, "TRP": 285.0,
           "TYR": 263.0, "VAL": 174.0}
# dg(): weights of the CC, AC, PP, AP contacts, of %NIS apolar and %NIS charged, and the intercept - IC-NIS as published, NOT verified or
# calibrated here
COEF = (-0.09459, -0.10007, 0.19577, -0.22671, 0.18681, 0.13810, -15.9433)
GAS_CONSTANT = 0.0019858775      # kcal / (mol K)
IC_AA, IC_AP, IC_AC, IC_PP, IC_PC, IC_CC = range(6)
ONE_LETTER = {"A": "ALA", "R": "ARG", "N": "ASN", "D": "ASP", "C": "CYS", "Q": "GLN", "E": "GLU", "G": "GLY", "H": "HIS", "I": "ILE",
              "L": "LEU", "K": "LYS", "M": "MET", "F": "PHE", "P": "PRO", "S": "SER", "T": "THR", "W": "TRP", "Y": "TYR", "V": "VAL"}


def residue_name(name):
    """A residue name as the tables hold it: upper case, a one-letter code widened, MSE as MET."""
    n = str(name).strip().upper()
    n = ONE_LETTER.get(n, n)
    return "MET" if n == "MSE" else n


def residue_classes(names, table=IC_CLASS, other=APOLAR):
    """(classes [n] uint8, the number of names that are not in `table` and fell to `other`)."""
    cls = np.zeros(len(names), np.uint8)
    missed = 0
    for k, n in enumerate(names):
        n = residue_name(n)
        if n not in table:
            missed += 1
        cls[k] = table.get(n, other)
    return cls, missed


def ic_index(a, b):
    """The column of ic of the unordered class pair {a, b}: lo*(5-lo)/2 + hi."""
    lo, hi = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
    return lo * (5 - lo) // 2 + hi


def check_cutoff(cutoff=CUTOFF):
    """The cutoff as the device takes it: float32, widened.  ValueError unless finite, > 0 and <= 16."""
    c = float(np.float32(cutoff))
    if not (np.isfinite(c) and 0 < c <= 16):
        raise ValueError(f"cutoff must be in (0, 16], got {cutoff}")
    return c


def check_residues(res, n_atoms, cls, who="rec"):
    """(res [n_atoms] int32, classes [n_res] uint8) of one chain.  ValueError outside the limits of dfm_rescon_create: one residue index
    per atom, 1 <= n_res <= 4096, every index in [0, n_res), every class in {0, 1, 2}."""
    r, c = np.asarray(res), np.asarray(cls)
    if r.shape != (n_atoms,):
        raise ValueError(f"{who}_res must be [{n_atoms}], one residue index per atom, got {r.shape}")
    if c.ndim != 1 or not (1 <= c.size <= MAX_RES):
        raise ValueError(f"{who}_class must be [n_res] with 1 <= n_res <= {MAX_RES}, got {c.shape}")
    if r.size and (r.min() < 0 or r.max() >= c.size):
        bad = int(np.nonzero((r < 0) | (r >= c.size))[0][0])
        raise ValueError(f"{who}_res: atom {bad} has residue {int(r[bad])} outside [0, {c.size})")
    if ((c < 0) | (c > 2)).any():
        bad = int(np.nonzero((c < 0) | (c > 2))[0][0])
        raise ValueError(f"{who}_class: residue {bad} has class {int(c[bad])}, not 0, 1 or 2")
    return r.astype(np.int32), c.astype(np.uint8)


def check_poses(P):
    """ValueError unless 1 <= P <= 65536 (dfm_pose_rescon)."""
    if not (1 <= P <= MAX_POSES):
        raise ValueError(f"need 1 <= P <= {MAX_POSES} poses per call, got {P}")
    return P


def _all_pairs(rec, X, reach):
    """near_pairs without the bounding-box shortcut: every one of the Ar * Al distances is taken."""
    out_a, out_b = [], []
    step = max(1, _PAIR_BUDGET // max(rec.shape[0], 1))
    for lo in range(0, X.shape[0], step):
        xa = X[lo:lo + step]
        dx, dy, dz = (xa[:, None, k] - rec[None, :, k] for k in range(3))
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        with np.errstate(invalid="ignore"):
            a, b = np.nonzero(d < reach)
        out_a.append(lo + a)
        out_b.append(b)
    return (np.concatenate(out_a), np.concatenate(out_b)) if out_a else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def residue_contacts(rec_atoms, rec_res, rec_class, lig_atoms, lig_res, lig_class, center, rot, tr, cutoff=CUTOFF, per_residue=False,
                     bits=False, shortcut=True):
    """The definition.  rec_atoms [Ar,3], lig_atoms [Al,3] float32 heavy atoms; rec_res [Ar], lig_res [Al] the residue index of each atom;
    rec_class [Rr], lig_class [Lr] in {0, 1, 2}; center [3]; rot [P,3] axis-angle, tr [P,3].  Returns {ic [P,6], n_pairs, n_rec_res,
    n_lig_res [P]} int32, with `per_residue` rec_degree [P,Rr] / lig_degree [P,Lr] int32, with `bits` contact_bits [P,Lr,W] uint32.
    shortcut: sterics.near_pairs (atoms far from the other chain's box are dropped first); without it every atom pair is taken."""
    ct = check_cutoff(cutoff)
    rec = np.asarray(rec_atoms, np.float32).reshape(-1, 3)
    lig = np.asarray(lig_atoms, np.float32).reshape(-1, 3)
    rres, rcls = check_residues(rec_res, rec.shape[0], rec_class, "rec")
    lres, lcls = check_residues(lig_res, lig.shape[0], lig_class, "lig")
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    if rot.shape != tr.shape:
        raise ValueError(f"rot and tr must both be [P,3], got {rot.shape} and {tr.shape}")
    P, Rr, Lr = check_poses(rot.shape[0]), rcls.size, lcls.size
    W = (Rr + 31) // 32
    out = {"ic": np.zeros((P, 6), np.int32), "n_pairs": np.zeros(P, np.int32), "n_rec_res": np.zeros(P, np.int32),
           "n_lig_res": np.zeros(P, np.int32)}
    if per_residue:
        out["rec_degree"], out["lig_degree"] = np.zeros((P, Rr), np.int32), np.zeros((P, Lr), np.int32)
    if bits:
        out["contact_bits"] = np.zeros((P, Lr, W), np.uint32)
    rec64 = rec.astype(np.float64)
    for p in range(P):
        if not (np.isfinite(rot[p]).all() and np.isfinite(tr[p]).all()):
            continue
        X = ST.pose_atoms(lig, center, rot[p], tr[p])
        if shortcut:
            a, b, _ = ST.near_pairs(rec, X, ct)
        else:
            a, b = _all_pairs(rec64, X, ct)
        m = np.zeros((Lr, Rr), bool)
        m[lres[a], rres[b]] = True
        j, i = np.nonzero(m)
        out["ic"][p] = np.bincount(ic_index(lcls[j], rcls[i]), minlength=6)
        out["n_pairs"][p] = j.size
        out["n_rec_res"][p], out["n_lig_res"][p] = m.any(0).sum(), m.any(1).sum()
        if per_residue:
            out["rec_degree"][p], out["lig_degree"][p] = m.sum(0), m.sum(1)
        if bits:
            out["contact_bits"][p] = pack_bits(m)
    return out


def pack_bits(m):
    """[Lr,Rr] bool -> [Lr,W] uint32: bit i & 31 of word i >> 5."""
    m = np.asarray(m, bool)
    Lr, Rr = m.shape
    W = (Rr + 31) // 32
    pad = np.zeros((Lr, W * 32), np.uint64)
    pad[:, :Rr] = m
    return (pad.reshape(Lr, W, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def unpack_bits(bits_row_block, n_rec_res=None):
    """[Lr,W] uint32 -> [Lr, n_rec_res or 32 W] bool."""
    b = np.asarray(bits_row_block, np.uint32)
    m = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(b.shape[0], -1)
    return m if n_rec_res is None else m[:, :n_rec_res]


def pairs_of(bits_row_block):
    """One pose's block of contact_bits [Lr,W] as [n,2] int32 (receptor residue, ligand residue), ascending in (ligand, receptor)."""
    j, i = np.nonzero(unpack_bits(bits_row_block))
    return np.stack([i, j], 1).astype(np.int32)


def popcount(bits):
    """Set bits over the last two axes of contact_bits: [P,Lr,W] -> [P]."""
    b = np.asarray(bits, np.uint32)
    return np.unpackbits(b.view(np.uint8).reshape(b.shape[:-2] + (-1,)), axis=-1).sum(-1).astype(np.int64)


def dg_contacts(ic, coef=COEF):
    """The four contact terms of dg alone, float64 [P], in this order of operations:
    ((coef[0]*CC + coef[1]*AC) + coef[2]*PP) + coef[3]*AP, the counts widened to float64."""
    ic = np.asarray(ic, np.float64).reshape(-1, 6)
    c = [float(v) for v in coef]
    return ((c[0] * ic[:, IC_CC] + c[1] * ic[:, IC_AC]) + c[2] * ic[:, IC_PP]) + c[3] * ic[:, IC_AP]


def dg(ic, nis_apolar, nis_charged, coef=COEF):
    """Predicted binding free energy in kcal/mol, float64 [P]:
    ((dg_contacts(ic, coef) + coef[4]*nis_apolar) + coef[5]*nis_charged) + coef[6], nis_* in percent.  NaN where a share is NaN."""
    c = [float(v) for v in coef]
    if len(c) != 7:
        raise ValueError(f"coef must have 7 entries (CC, AC, PP, AP, %NIS apolar, %NIS charged, intercept), got {len(c)}")
    a, q = np.asarray(nis_apolar, np.float64).reshape(-1), np.asarray(nis_charged, np.float64).reshape(-1)
    return ((dg_contacts(ic, c) + c[4] * a) + c[5] * q) + c[6]


def kd(dg_value, temp_c=25.0):
    """Dissociation constant in M: exp(dg / (0.0019858775 * (temp_c + 273.15)))."""
    return np.exp(np.asarray(dg_value, np.float64) / (GAS_CONSTANT * (float(temp_c) + 273.15)))


def nis_percent(rec_sasa, lig_sasa, rec_names, lig_names, ref_asa=REF_ASA, threshold=0.05, table=NIS_CLASS):
    """Composition of the non-interacting surface, float64 [P,3] = percent apolar, polar, charged.  rec_sasa [P,Rr], lig_sasa [P,Lr]: the
    residues' accessible area IN the complex (complex_residue_sasa); a residue is on the surface iff sasa / ref_asa[name] >= threshold
    (one float64 division; a name missing from ref_asa or from `table` is never on it).  Per pose and class: 100.0 * count / n over the
    surface residues of both chains, n their number; NaN for all three when there are none."""
    rs, ls = np.atleast_2d(np.asarray(rec_sasa, np.float64)), np.atleast_2d(np.asarray(lig_sasa, np.float64))
    if rs.shape[0] != ls.shape[0] or rs.shape[1] != len(rec_names) or ls.shape[1] != len(lig_names):
        raise ValueError(f"sasa must be [P,{len(rec_names)}] and [P,{len(lig_names)}], got {rs.shape} and {ls.shape}")
    names = [residue_name(n) for n in list(rec_names) + list(lig_names)]
    known = np.array([n in ref_asa and n in table for n in names], bool)
    ref = np.array([float(ref_asa[n]) if k else 1.0 for n, k in zip(names, known)], np.float64)
    cls = np.array([table[n] if k else 0 for n, k in zip(names, known)], np.int64)
    on = (np.concatenate([rs, ls], 1) / ref >= float(threshold)) & known
    n = on.sum(1).astype(np.float64)
    out = np.full((on.shape[0], 3), np.nan)
    for c in range(3):
        cnt = (on & (cls == c)).sum(1).astype(np.float64)
        out[n > 0, c] = 100.0 * cnt[n > 0] / n[n > 0]
    return out


def complex_residue_sasa(exposed, buried, radius, res, n_res, probe, K):
    """Accessible area of every residue of one chain inside the complex, float64 [P,n_res] A^2: per atom the sphere points exposed in
    isolation (exposed [n], Surface.info) minus those the partner buries (buried [P,n], Surface.bsa(per_atom=True)), summed per residue
    and radius value, times the value's area per point (surface.class_areas), values in ascending order."""
    from . import surface as SF
    radius = np.asarray(radius, np.float32).reshape(-1)
    free = np.asarray(exposed, np.int64).reshape(1, -1) - np.atleast_2d(np.asarray(buried, np.int64))
    vals = np.unique(radius)
    area = SF.class_areas(vals, probe, K)
    out = np.zeros((free.shape[0], n_res), np.float64)
    for c, v in enumerate(vals):
        m = radius == v
        out = out + ST.residue_counts(free[:, m], np.asarray(res)[m], n_res) * area[c]
    return out


def write_contact_residues(path, rec_keys, lig_keys, pairs):
    """--contact-residues: one line `chainR:num[icode] name  chainL:num[icode] name` per residue pair of `pairs` [n,2] (receptor, ligand);
    keys as sterics.residue_of_atoms gives them."""
    fmt = lambda k: f"{k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''} {k[3]}"
    with open(path, "w") as f:
        f.write("# receptor residue, name, ligand residue, name: heavy atoms of the two closer than the cutoff\n")
        for i, j in np.asarray(pairs, np.int64).reshape(-1, 2):
            f.write(f"{fmt(rec_keys[int(i)])}  {fmt(lig_keys[int(j)])}\n")
