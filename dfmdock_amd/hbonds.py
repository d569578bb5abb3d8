"""Interface hydrogen bonds and salt bridges of an ensemble of rigid ligand poses: the float64 numpy definition of dfm_pose_hbonds
(include/dfmdock_amd.h, kernels_hbond.hip) and its host finishes.  No reference counterpart.

The PDB files here carry no hydrogens, so the criteria are on heavy atoms only: a distance and two angles on the atom pair and the two
antecedents (the bonded heavy atom the angle is taken at), the form of HBPLUS's heavy-atom conditions.  HIS is treated as donor AND
acceptor on both ring nitrogens, and as a cation.  CYS SG and MET SD are neither donor nor acceptor.  No agreement with the counts of
PISA, HBPLUS or any other published tool is claimed or tested.

  roles       uint8 bits per atom: DONOR 1, ACCEPTOR 2, CATION 4, ANION 8, SIDECHAIN 16 (polar_atoms)
  pose        sterics.pose_atoms of the ligand's atoms AND of their antecedents: the antecedent rides with the ligand
  per pair    posed ligand atom X with antecedent XA, receptor atom Y with antecedent YA, everything widened to float64, no square root
              and no division:
                  dx,dy,dz = Y - X ;  r2 = (dx*dx + dy*dy) + dz*dz
                  ux,uy,uz = XA - X ; uu = (ux*ux + uy*uy) + uz*uz ; du =  (ux*dx + uy*dy) + uz*dz
                  wx,wy,wz = YA - Y ; ww = (wx*wx + wy*wy) + wz*wz ; dw = -((wx*dx + wy*dy) + wz*dz)
              hydrogen bond  iff  one atom is a DONOR and the other an ACCEPTOR (in either direction)
                             and  r2 < hb_cutoff*hb_cutoff                     (strict)
                             and  du <= 0 and du*du >= c2*(uu*r2)               (angle XA-X..Y >= min_angle)
                             and  dw <= 0 and dw*dw >= c2*(ww*r2)               (angle YA-Y..X >= min_angle)
              salt-bridge atom pair  iff  one atom is a CATION and the other an ANION, and r2 < salt_cutoff*salt_cutoff
              c2 = 0.0 for min_angle 90, else cos(radians(min_angle))**2 (min_cos2).  A NaN makes every comparison false.  A coincident
              antecedent (uu == 0) has du == 0 and passes its angle test.  A pair whose atoms are both donor and acceptor is ONE bond;
              a pair can be a hydrogen bond and a salt-bridge pair at once, and then counts as both.
  n_hbond [P] int32        hydrogen bonds of the pose
  hb_kind [P,3] int32      bonds by the number of SIDECHAIN atoms among the two: backbone-backbone, mixed, side chain-side chain
  n_salt [P] int32         DISTINCT (receptor residue, ligand residue) pairs with at least one salt-bridge atom pair
  n_salt_atoms [P] int32   the salt-bridge atom pairs
  rec_hb [P,Nr], lig_hb [P,Nl], rec_sb, lig_sb (per_atom)   bonds / salt-bridge partners of each polar atom, the caller's order

Everything is an integer, so the device's arrays equal these, whatever the waves, blocks and chunks.  A pose with a non-finite transform
gets zeros.
"""
from __future__ import annotations

import math

import numpy as np

from . import sterics as ST
from .affinity import residue_name

DONOR, ACCEPTOR, CATION, ANION, SIDECHAIN = 1, 2, 4, 8, 16
ROLE_MASK = 31
HB_CUTOFF, MIN_ANGLE, SALT_CUTOFF = 3.5, 90.0, 4.0
MAX_CUTOFF = 8.0
MAX_RES = 4096              # residues per chain (dfm_hbond_create)
MAX_POSES = 65536           # poses per call (dfm_pose_hbonds)
_PAIR_BUDGET = 1 << 21      # atom pairs per broadcast block of the shortcut-free path

_D, _A, _C, _N, _S = DONOR, ACCEPTOR, CATION, ANION, SIDECHAIN
# side-chain polar atoms: (residue, atom) -> (role, antecedent)
SIDE_CHAIN = {
    ("ARG", "NE"): (_D | _C | _S, "CZ"), ("ARG", "NH1"): (_D | _C | _S, "CZ"), ("ARG", "NH2"): (_D | _C | _S, "CZ"),
    ("ASN", "OD1"): (_A | _S, "CG"), ("ASN", "ND2"): (_D | _S, "CG"),
    ("GLN", "OE1"): (_A | _S, "CD"), ("GLN", "NE2"): (_D | _S, "CD"),
    ("ASP", "OD1"): (_A | _N | _S, "CG"), ("ASP", "OD2"): (_A | _N | _S, "CG"),
    ("GLU", "OE1"): (_A | _N | _S, "CD"), ("GLU", "OE2"): (_A | _N | _S, "CD"),
    ("HIS", "ND1"): (_D | _A | _C | _S, "CG"), ("HIS", "NE2"): (_D | _A | _C | _S, "CE1"),
    ("LYS", "NZ"): (_D | _C | _S, "CE"),
    ("SER", "OG"): (_D | _A | _S, "CB"), ("THR", "OG1"): (_D | _A | _S, "CB"), ("TYR", "OH"): (_D | _A | _S, "CZ"),
    ("TRP", "NE1"): (_D | _S, "CD1"),
}
BACKBONE_ANTECEDENT = {"N": "CA", "O": "C", "OXT": "C"}


def polar_atoms(atoms, heavy_index=None):
    """The atoms with a role among the heavy atoms `heavy_index` (default: sterics.heavy_atoms) of pdbio.read_pdb records, by (residue
    name, atom name) through affinity.residue_name (MSE is MET, which has no role).  Backbone N is a donor except in PRO and a cation in
    a chain's first residue; O and OXT are acceptors, and anions in a residue that has an OXT (the terminus rule of
    ifenergy.atom_parameters); the side chains are SIDE_CHAIN.  CYS SG and MET SD get no role.  A polar atom whose antecedent is missing
    from its residue gets no role either and is counted in `untyped`.  Returns {index [n] (into the heavy-atom order), xyz [n,3] and ante
    [n,3] float32, role [n] uint8, res [n] int32 (sterics.residue_of_atoms numbering over the heavy atoms), n_res, keys, untyped}."""
    heavy = ST.heavy_atoms(atoms) if heavy_index is None else np.asarray(heavy_index, np.int64)
    keys, res = ST.residue_of_atoms(atoms, heavy)
    by_name = [{} for _ in keys]      # residue -> atom name -> coordinate (the first atom of a name)
    first = {}
    for n, i in enumerate(heavy):
        a = atoms[int(i)]
        by_name[res[n]].setdefault(a["name"], a["coord"])
        first.setdefault(a["chain"], res[n])
    index, xyz, ante, role, rres, untyped = [], [], [], [], [], 0
    for n, i in enumerate(heavy):
        a = atoms[int(i)]
        r, name, rn = int(res[n]), a["name"], residue_name(a["res_name"])
        if name in BACKBONE_ANTECEDENT:
            if name == "N":
                bits = (0 if rn == "PRO" else DONOR) | (CATION if first[a["chain"]] == r else 0)
            else:
                bits = ACCEPTOR | (ANION if "OXT" in by_name[r] else 0)
            back = BACKBONE_ANTECEDENT[name]
        elif (rn, name) in SIDE_CHAIN:
            bits, back = SIDE_CHAIN[(rn, name)]
        else:
            continue
        if not bits:
            continue
        if back not in by_name[r]:
            untyped += 1
            continue
        index.append(n); xyz.append(a["coord"]); ante.append(by_name[r][back]); role.append(bits); rres.append(r)
    return {"index": np.asarray(index, np.int64), "xyz": np.asarray(xyz, np.float32).reshape(-1, 3),
            "ante": np.asarray(ante, np.float32).reshape(-1, 3), "role": np.asarray(role, np.uint8), "res": np.asarray(rres, np.int32),
            "n_res": len(keys), "keys": keys, "untyped": untyped}


def min_cos2(min_angle=MIN_ANGLE):
    """c2 of the angle tests, the double both sides use: exactly 0.0 for 90 degrees, else cos(radians(min_angle))**2.  ValueError unless
    90 <= min_angle < 180."""
    m = float(min_angle)
    if not (90.0 <= m < 180.0):
        raise ValueError(f"min_angle must be in [90, 180) degrees, got {min_angle}")
    return 0.0 if m == 90.0 else math.cos(math.radians(m)) ** 2


def check_cutoffs(hb_cutoff=HB_CUTOFF, salt_cutoff=SALT_CUTOFF):
    """The cutoffs as the device takes them: float32, widened.  ValueError unless both are in (0, 8]."""
    h, s = float(np.float32(hb_cutoff)), float(np.float32(salt_cutoff))
    if not (np.isfinite(h) and 0 < h <= MAX_CUTOFF):
        raise ValueError(f"hb_cutoff must be in (0, {MAX_CUTOFF:g}], got {hb_cutoff}")
    if not (np.isfinite(s) and 0 < s <= MAX_CUTOFF):
        raise ValueError(f"salt_cutoff must be in (0, {MAX_CUTOFF:g}], got {salt_cutoff}")
    return h, s


def check_chain(chain, who="rec"):
    """(xyz [n,3] float32, ante [n,3] float32, role [n] uint8, res [n] int32, n_res) of one chain's polar atoms (a polar_atoms dict).
    ValueError outside the limits of dfm_hbond_create: n >= 1, one antecedent, role and residue per atom, every role within the five
    bits, 1 <= n_res <= 4096, every residue index in [0, n_res), every coordinate finite."""
    xyz, ante = np.asarray(chain["xyz"], np.float32), np.asarray(chain["ante"], np.float32)
    role, res, n_res = np.asarray(chain["role"]), np.asarray(chain["res"]), int(chain["n_res"])
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f"{who}: xyz must be [n,3] with n >= 1, got {xyz.shape}")
    n = xyz.shape[0]
    if ante.shape != (n, 3) or role.shape != (n,) or res.shape != (n,):
        raise ValueError(f"{who}: ante must be [{n},3], role and res [{n}], got {ante.shape}, {role.shape}, {res.shape}")
    if not (np.isfinite(xyz).all() and np.isfinite(ante).all()):
        raise ValueError(f"{who}: a coordinate is not finite")
    if ((role.astype(np.int64) < 0) | (role.astype(np.int64) > ROLE_MASK)).any():
        raise ValueError(f"{who}_role: a role is outside the five bits")
    if not (1 <= n_res <= MAX_RES):
        raise ValueError(f"{who}: need 1 <= n_res <= {MAX_RES}, got {n_res}")
    if res.min() < 0 or res.max() >= n_res:
        raise ValueError(f"{who}_res: a residue index is outside [0, {n_res})")
    return xyz, ante, role.astype(np.uint8), res.astype(np.int32), n_res


def _pairs(rec64, X, reach, shortcut):
    """(ligand atom a, receptor atom b) of every pair the tests are made on: with the shortcut sterics.near_pairs at a reach a little
    above the largest cutoff (nothing that can pass r2 < cutoff^2 is lost), without it every pair."""
    if shortcut:
        a, b, _ = ST.near_pairs(rec64, X, reach + 1e-6)
        return a, b
    n = rec64.shape[0]
    a = np.repeat(np.arange(X.shape[0]), n)
    return a, np.tile(np.arange(n), X.shape[0])


def pair_tests(X, XA, Y, YA, role_x, role_y, hb_cutoff, c2, salt_cutoff):
    """(hydrogen bond, salt-bridge atom pair) bool [n] of n pairs: the per-pair recipe of the module docstring, operation by operation.
    X, XA (posed ligand atom, its posed antecedent), Y, YA (receptor atom, its antecedent) [n,3] float64; role_* [n]."""
    dx, dy, dz = (Y[:, k] - X[:, k] for k in range(3))
    r2 = (dx * dx + dy * dy) + dz * dz
    ux, uy, uz = (XA[:, k] - X[:, k] for k in range(3))
    uu = (ux * ux + uy * uy) + uz * uz
    du = (ux * dx + uy * dy) + uz * dz
    wx, wy, wz = (YA[:, k] - Y[:, k] for k in range(3))
    ww = (wx * wx + wy * wy) + wz * wz
    dw = -((wx * dx + wy * dy) + wz * dz)
    rx, ry = role_x.astype(np.int64), role_y.astype(np.int64)
    compl = (((rx & DONOR) != 0) & ((ry & ACCEPTOR) != 0)) | (((rx & ACCEPTOR) != 0) & ((ry & DONOR) != 0))
    ionic = (((rx & CATION) != 0) & ((ry & ANION) != 0)) | (((rx & ANION) != 0) & ((ry & CATION) != 0))
    with np.errstate(invalid="ignore", over="ignore"):
        hb = compl & (r2 < hb_cutoff * hb_cutoff) & (du <= 0) & (du * du >= c2 * (uu * r2)) & (dw <= 0) & (dw * dw >= c2 * (ww * r2))
        sb = ionic & (r2 < salt_cutoff * salt_cutoff)
    return hb, sb


def hbonds(rec, lig, center, rot, tr, hb_cutoff=HB_CUTOFF, min_angle=MIN_ANGLE, salt_cutoff=SALT_CUTOFF, per_atom=False, shortcut=True):
    """The definition.  rec, lig: the polar atoms of the two chains (polar_atoms dicts: xyz, ante, role, res, n_res); center [3]; rot
    [P,3] axis-angle, tr [P,3].  Returns {n_hbond [P], hb_kind [P,3], n_salt [P], n_salt_atoms [P]} int32 and, with `per_atom`, rec_hb /
    rec_sb [P,Nr] and lig_hb / lig_sb [P,Nl] int32.  shortcut: sterics.near_pairs; without it every atom pair is taken."""
    hc, sc = check_cutoffs(hb_cutoff, salt_cutoff)
    c2 = min_cos2(min_angle)
    rx, ra, rrole, rres, Rr = check_chain(rec, "rec")
    lx, la, lrole, lres, _ = check_chain(lig, "lig")
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    if rot.shape != tr.shape or not (1 <= rot.shape[0] <= MAX_POSES):
        raise ValueError(f"rot and tr must both be [P,3] with 1 <= P <= {MAX_POSES}, got {rot.shape} and {tr.shape}")
    P, Nr, Nl = rot.shape[0], rx.shape[0], lx.shape[0]
    out = {"n_hbond": np.zeros(P, np.int32), "hb_kind": np.zeros((P, 3), np.int32), "n_salt": np.zeros(P, np.int32),
           "n_salt_atoms": np.zeros(P, np.int32)}
    if per_atom:
        out.update(rec_hb=np.zeros((P, Nr), np.int32), lig_hb=np.zeros((P, Nl), np.int32), rec_sb=np.zeros((P, Nr), np.int32),
                   lig_sb=np.zeros((P, Nl), np.int32))
    Y, YA = rx.astype(np.float64), ra.astype(np.float64)
    side_l, side_r = (lrole.astype(np.int64) >> 4) & 1, (rrole.astype(np.int64) >> 4) & 1
    for p in range(P):
        if not (np.isfinite(rot[p]).all() and np.isfinite(tr[p]).all()):
            continue
        X, XA = ST.pose_atoms(lx, center, rot[p], tr[p]), ST.pose_atoms(la, center, rot[p], tr[p])
        a, b = _pairs(Y, X, max(hc, sc), shortcut)
        hb = np.zeros(a.size, bool)
        sb = np.zeros(a.size, bool)
        for lo in range(0, a.size, _PAIR_BUDGET):
            s = slice(lo, lo + _PAIR_BUDGET)
            hb[s], sb[s] = pair_tests(X[a[s]], XA[a[s]], Y[b[s]], YA[b[s]], lrole[a[s]], rrole[b[s]], hc, c2, sc)
        out["n_hbond"][p] = hb.sum()
        out["hb_kind"][p] = np.bincount(side_l[a[hb]] + side_r[b[hb]], minlength=3)
        out["n_salt_atoms"][p] = sb.sum()
        out["n_salt"][p] = np.unique(rres[b[sb]].astype(np.int64) * (1 << 20) + lres[a[sb]]).size
        if per_atom:
            out["rec_hb"][p], out["lig_hb"][p] = np.bincount(b[hb], minlength=Nr), np.bincount(a[hb], minlength=Nl)
            out["rec_sb"][p], out["lig_sb"][p] = np.bincount(b[sb], minlength=Nr), np.bincount(a[sb], minlength=Nl)
    return out


def residue_bonds(per_atom, res, n_res):
    """Per-atom counts [.., n] (rec_hb, lig_sb, ...) summed per residue -> [.., n_res] (sterics.residue_counts)."""
    return ST.residue_counts(per_atom, res, n_res)


def unsatisfied(role, exposed, buried, hb, percent=100):
    """The polar atoms a pose buries and leaves without a partner.  role [n]; exposed [n]: the sphere points of each polar atom that are
    exposed in isolation, buried [P,n]: those the partner buries in each pose (the per-atom point counts of surface.bsa / dfm_pose_bsa,
    gathered to the polar atoms); hb [P,n]: rec_hb or lig_hb.  An atom is unsatisfied in a pose iff it is a donor or an acceptor, exposed
    > 0, buried * 100 >= percent * exposed (integers) and hb == 0.  Returns {mask [P,n] bool, n_unsat [P], n_unsat_donor,
    n_unsat_acceptor, n_unsat_both [P] (atoms that are donors only, acceptors only, both)} int32."""
    if not (0 < int(percent) <= 100) or int(percent) != percent:
        raise ValueError(f"percent must be an integer in 1 .. 100, got {percent}")
    role, exposed = np.asarray(role).astype(np.int64).reshape(-1), np.asarray(exposed).astype(np.int64).reshape(-1)
    buried, hb = np.atleast_2d(np.asarray(buried).astype(np.int64)), np.atleast_2d(np.asarray(hb).astype(np.int64))
    if exposed.shape != role.shape or buried.shape != hb.shape or buried.shape[1] != role.size:
        raise ValueError(f"need role and exposed [n], buried and hb [P,n], got {role.shape}, {exposed.shape}, {buried.shape}, {hb.shape}")
    da = role & (DONOR | ACCEPTOR)
    mask = (da != 0)[None] & (exposed > 0)[None] & (buried * 100 >= int(percent) * exposed[None]) & (hb == 0)
    cnt = lambda sel: (mask & sel[None]).sum(1).astype(np.int32)
    return {"mask": mask, "n_unsat": mask.sum(1).astype(np.int32), "n_unsat_donor": cnt(da == DONOR), "n_unsat_acceptor": cnt(da == ACCEPTOR),
            "n_unsat_both": cnt(da == (DONOR | ACCEPTOR))}


def write_hbond_residues(path, rec_keys, rec_hb, rec_sb, lig_keys, lig_hb, lig_sb):
    """--hbond-residues: one line `R|L chain:resnum[icode] res_name n_hbond n_salt_atoms` per residue of either chain with a nonzero
    count; keys as sterics.residue_of_atoms gives them, counts per residue (residue_bonds)."""
    with open(path, "w") as f:
        f.write("# chain (R receptor, L ligand), residue, name, hydrogen bonds, salt-bridge atom pairs its atoms take part in\n")
        for side, keys, hb, sb in (("R", rec_keys, rec_hb, rec_sb), ("L", lig_keys, lig_hb, lig_sb)):
            for k, h, s in zip(keys, hb, sb):
                if h != 0 or s != 0:
                    f.write(f"{side} {k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''} {k[3]} {int(h)} {int(s)}\n")
