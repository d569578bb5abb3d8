"""Buried solvent-accessible surface area (Shrake-Rupley) of an ensemble of rigid ligand poses: the float64 numpy definition of
dfm_pose_bsa (include/dfmdock_amd.h, kernels_surface.hip) and its host finishes.  No reference counterpart: the reference never looks at
the surface of a pose.

  sphere points          sphere_points(K): the golden-spiral lattice z_k = 1 - (2k+1)/K, r_k = sqrt(1 - z_k^2), phi_k = k pi (3 - sqrt 5),
                         u_k = (r cos phi, r sin phi, z) rounded to float32.  K is a multiple of 64 in 64 .. 256.
  radius of atom i       R_i = float64(radius_i) + float64(probe); both chains together hold at most 16 distinct radius values (float32
                         bit patterns); the class of an atom is the index of its value in their ascending list
  distance               d = sqrt((dx*dx + dy*dy) + dz*dz) in float64
  isolated exposure      per chain, in the chain's input frame: point k of atom i is c_i + R_i u_k; it is exposed iff no OTHER atom j of
                         the same chain has d < R_j (strict)
  pose p                 x_a = sterics.pose_atoms(lig, center, rot_p, tr_p); w_k = (R[:,0] u0 + R[:,1] u1) + R[:,2] u2 with
                         R = pdbio.axis_angle_to_matrix(rot_p); ligand point x_a + R_a w_k, receptor point c_b + R_b u_k
  buried                 a point that is exposed in isolation and has d < R_j (strict) to some atom j of the OTHER chain
  lig_buried / rec_buried [p,a]   buried points per atom; lig_points / rec_points [p] their sums; class_points [p,2,16] the sums per chain
                         (receptor = 0) and radius class
  bsa [p]                sum over chain (receptor first) and class (ascending) of count * (4.0 pi R_c R_c / K), left to right: equal
                         counts give bitwise equal areas.  The total over both sides; the "interface area" is half of it.

A NaN distance buries nothing: a pose with a non-finite transform gets all zeros.  The candidate atoms of a point come from
sterics.near_pairs (bounding boxes, then centre distances below the largest R_a + R_b plus 1e-3 A): a point of atom a lies R_a from its
centre, so an atom b that buries it has its centre closer than R_a + R_b.  The atoms are heavy atoms; the caller filters hydrogens.
"""
from __future__ import annotations

import numpy as np

from . import pdbio
from . import sterics as ST

PROBE = 1.4
POINTS = 128
MAX_CLASSES = 16
_REACH_PAD = 1e-3           # added to the largest R_a + R_b of near_pairs: far above any rounding of a point's distance from its centre
_PAIR_CHUNK = 4096          # near pairs per broadcast block [pairs, K, 3]
_RADII = {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80, "P": 1.80, "SE": 1.90}
_OTHER_RADIUS = 1.80


def check_points(K):
    K = int(K)
    if K < 64 or K > 256 or K % 64:
        raise ValueError(f"sphere points must be a multiple of 64 in 64 .. 256, got {K}")
    return K


def sphere_points(K):
    """[K,3] float32: the golden-spiral lattice of the definition."""
    K = check_points(K)
    k = np.arange(K, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / K
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)


def check_probe(probe):
    pr = float(np.float32(probe))
    if not (np.isfinite(pr) and pr > 0):
        raise ValueError(f"probe must be finite and > 0, got {probe}")
    return pr


def radius_classes(rec_radius, lig_radius):
    """(values [n] float32 ascending, rec_class [Ar], lig_class [Al]).  ValueError for a radius that is not finite and > 0 or for more
    than 16 distinct values."""
    rr, lr = np.asarray(rec_radius, np.float32).reshape(-1), np.asarray(lig_radius, np.float32).reshape(-1)
    both = np.concatenate([rr, lr])
    if not (np.isfinite(both).all() and (both > 0).all()):
        raise ValueError("radii must be finite and > 0")
    vals = np.unique(both)
    if vals.size > MAX_CLASSES:
        raise ValueError(f"at most {MAX_CLASSES} distinct radii, got {vals.size}")
    return vals, np.searchsorted(vals, rr), np.searchsorted(vals, lr)


def class_areas(values, probe, K):
    """[16] float64: the area 4.0 pi R_c R_c / K of one point of each radius class (0 past the last class)."""
    out = np.zeros(MAX_CLASSES, np.float64)
    for c, v in enumerate(np.asarray(values, np.float32)):
        R = float(v) + float(np.float32(probe))
        out[c] = 4.0 * np.pi * R * R / K
    return out


def bsa_from_class_points(class_points, values, probe, K):
    """bsa [P] float64 of class_points [P,2,16]: receptor first, classes ascending, summed left to right."""
    cp = np.asarray(class_points).reshape(-1, 2, MAX_CLASSES)
    area = class_areas(values, probe, K)
    out = np.zeros(cp.shape[0], np.float64)
    for p in range(cp.shape[0]):
        s = 0.0
        for chain in range(2):
            for c in range(len(values)):
                s = s + float(cp[p, chain, c]) * area[c]
        out[p] = s
    return out


def _all_pairs(n_a, n_b):
    a, b = np.divmod(np.arange(n_a * n_b, dtype=np.int64), n_b)
    return a, b


def _hits(centers, R, dirs, ia, other, R_other, ib):
    """[pairs, K] bool: point k of atom ia (centre `centers`, radius R, directions dirs [K,3] or per-pair) is closer than R_other[ib] to
    atom ib of `other`.  d = sqrt((dx*dx + dy*dy) + dz*dz), strict; NaN is no hit."""
    out = np.zeros((ia.size, dirs.shape[0]), bool)
    for lo in range(0, ia.size, _PAIR_CHUNK):
        a, b = ia[lo:lo + _PAIR_CHUNK], ib[lo:lo + _PAIR_CHUNK]
        dx, dy, dz = ((centers[a, k][:, None] + R[a][:, None] * dirs[None, :, k]) - other[b, k][:, None] for k in range(3))
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        with np.errstate(invalid="ignore"):
            out[lo:lo + _PAIR_CHUNK] = d < R_other[b][:, None]
    return out


def _or_rows(n, K, rows, hits):
    out = np.zeros((n, K), bool)
    if rows.size:
        np.logical_or.at(out, rows, hits)
    return out


def exposure(atoms, radius, probe=PROBE, K=POINTS, shortcut=True):
    """Isolated exposure of one chain: [n,K] bool.  `shortcut`: candidates from sterics.near_pairs, else every pair."""
    x = np.asarray(atoms, np.float32).reshape(-1, 3).astype(np.float64)
    R = np.asarray(radius, np.float32).reshape(-1).astype(np.float64) + float(np.float32(probe))
    u = sphere_points(K).astype(np.float64)
    if shortcut:
        i, j, _ = ST.near_pairs(x, x, 2.0 * R.max() + _REACH_PAD)      # (a of X, b of rec) = (i, j)
    else:
        i, j = _all_pairs(x.shape[0], x.shape[0])
    keep = i != j
    i, j = i[keep], j[keep]
    return ~_or_rows(x.shape[0], u.shape[0], i, _hits(x, R, u, i, x, R, j))


def near_atom_pairs(rec, X, reach, shortcut=True):
    """(a, b) of the candidate pairs of one pose: ligand atom a, receptor atom b."""
    if shortcut:
        a, b, _ = ST.near_pairs(rec, X, reach)
        return a, b
    return _all_pairs(X.shape[0], rec.shape[0])


def bsa(rec_atoms, rec_radius, lig_atoms, lig_radius, center, rot, tr, probe=PROBE, K=POINTS, per_atom=True, shortcut=True, stats=None):
    """The definition.  Returns {lig_buried [P,Al], rec_buried [P,Ar] (with `per_atom`), lig_points, rec_points [P] int32, class_points
    [P,2,16] int32, bsa [P] float64, sasa_rec, sasa_lig (float64), rec_exposed [Ar], lig_exposed [Al] int32, class_radius}.  `stats`: a dict
    that receives near_pairs (the candidate pairs summed over the poses)."""
    K, pr = check_points(K), check_probe(probe)
    rec = np.asarray(rec_atoms, np.float32).reshape(-1, 3).astype(np.float64)
    lig = np.asarray(lig_atoms, np.float32).reshape(-1, 3)
    vals, rcls, lcls = radius_classes(rec_radius, lig_radius)
    if rcls.size != rec.shape[0] or lcls.size != lig.shape[0]:
        raise ValueError("one radius per atom")
    Rr, Rl = vals[rcls].astype(np.float64) + pr, vals[lcls].astype(np.float64) + pr
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    if rot.shape != tr.shape:
        raise ValueError(f"rot and tr must both be [P,3], got {rot.shape} and {tr.shape}")
    P, Ar, Al = rot.shape[0], rec.shape[0], lig.shape[0]
    u = sphere_points(K).astype(np.float64)
    exp_r, exp_l = exposure(rec, vals[rcls], pr, K, shortcut), exposure(lig, vals[lcls], pr, K, shortcut)
    out = {"lig_points": np.zeros(P, np.int32), "rec_points": np.zeros(P, np.int32), "class_points": np.zeros((P, 2, MAX_CLASSES), np.int32),
           "rec_exposed": exp_r.sum(1).astype(np.int32), "lig_exposed": exp_l.sum(1).astype(np.int32), "class_radius": vals}
    iso = np.zeros((2, 2, MAX_CLASSES), np.int64)      # the isolated areas: class sums in the order of bsa
    iso[0, 0] = np.bincount(rcls, weights=out["rec_exposed"], minlength=MAX_CLASSES)
    iso[1, 0] = np.bincount(lcls, weights=out["lig_exposed"], minlength=MAX_CLASSES)
    out["sasa_rec"], out["sasa_lig"] = (float(v) for v in bsa_from_class_points(iso, vals, pr, K))
    lb, rb = np.zeros((P, Al), np.int32), np.zeros((P, Ar), np.int32)
    reach = Rr.max() + Rl.max() + _REACH_PAD
    n_pairs = 0
    for p in range(P):
        if not (np.isfinite(rot[p]).all() and np.isfinite(tr[p]).all()):
            continue
        X = ST.pose_atoms(lig, center, rot[p], tr[p])
        M = pdbio.axis_angle_to_matrix(rot[p].reshape(3)).astype(np.float64)
        w = (M[None, :, 0] * u[:, 0:1] + M[None, :, 1] * u[:, 1:2]) + M[None, :, 2] * u[:, 2:3]
        a, b = near_atom_pairs(rec, X, reach, shortcut)
        n_pairs += a.size
        lb[p] = (_or_rows(Al, K, a, _hits(X, Rl, w, a, rec, Rr, b)) & exp_l).sum(1)
        rb[p] = (_or_rows(Ar, K, b, _hits(rec, Rr, u, b, X, Rl, a)) & exp_r).sum(1)
        out["class_points"][p, 0] = np.bincount(rcls, weights=rb[p], minlength=MAX_CLASSES)
        out["class_points"][p, 1] = np.bincount(lcls, weights=lb[p], minlength=MAX_CLASSES)
    out["lig_points"][:], out["rec_points"][:] = lb.sum(1), rb.sum(1)
    out["bsa"] = bsa_from_class_points(out["class_points"], vals, pr, K)
    if per_atom:
        out["lig_buried"], out["rec_buried"] = lb, rb
    if stats is not None:
        stats["near_pairs"] = stats.get("near_pairs", 0) + n_pairs
    return out


def pose_margins(rec_atoms, rec_radius, lig_atoms, lig_radius, center, rot, tr, probe=PROBE, K=POINTS):
    """How far every point of ONE pose is from being held: (lig_margin [Al,K], rec_margin [Ar,K], near pairs), margin = the smallest
    d - R_j over the candidate atoms j of the other chain (+inf without one).  A point is held iff its margin is below 0; tests call a
    point whose |margin| is tiny a border point."""
    K, pr = check_points(K), check_probe(probe)
    rec = np.asarray(rec_atoms, np.float32).reshape(-1, 3).astype(np.float64)
    lig = np.asarray(lig_atoms, np.float32).reshape(-1, 3)
    Rr = np.asarray(rec_radius, np.float32).reshape(-1).astype(np.float64) + pr
    Rl = np.asarray(lig_radius, np.float32).reshape(-1).astype(np.float64) + pr
    rot, tr = np.asarray(rot, np.float32).reshape(3), np.asarray(tr, np.float32).reshape(3)
    u = sphere_points(K).astype(np.float64)
    X = ST.pose_atoms(lig, center, rot, tr)
    M = pdbio.axis_angle_to_matrix(rot).astype(np.float64)
    w = (M[None, :, 0] * u[:, 0:1] + M[None, :, 1] * u[:, 1:2]) + M[None, :, 2] * u[:, 2:3]
    a, b = near_atom_pairs(rec, X, Rr.max() + Rl.max() + _REACH_PAD)

    def margin(n, centers, R, dirs, ia, other, R_other, ib):
        out = np.full((n, K), np.inf)
        for lo in range(0, ia.size, _PAIR_CHUNK):
            i, j = ia[lo:lo + _PAIR_CHUNK], ib[lo:lo + _PAIR_CHUNK]
            dx, dy, dz = ((centers[i, k][:, None] + R[i][:, None] * dirs[None, :, k]) - other[j, k][:, None] for k in range(3))
            np.minimum.at(out, i, np.sqrt((dx * dx + dy * dy) + dz * dz) - R_other[j][:, None])
        return out
    return margin(lig.shape[0], X, Rl, w, a, rec, Rr, b), margin(rec.shape[0], rec, Rr, u, b, X, Rl, a), int(a.size)


def side_areas(class_points, values, probe, K):
    """(bsa_rec [P], bsa_lig [P]): the two sides of bsa, each summed over its classes in ascending order."""
    cp = np.asarray(class_points).reshape(-1, 2, MAX_CLASSES)
    zero = np.zeros_like(cp)
    rec, lig = zero.copy(), zero.copy()
    rec[:, 0], lig[:, 1] = cp[:, 0], cp[:, 1]
    return bsa_from_class_points(rec, values, probe, K), bsa_from_class_points(lig, values, probe, K)


def element_radius(atom):
    """Van der Waals radius of a pdbio.read_pdb record: C 1.70, N 1.55, O 1.52, S 1.80, P 1.80, SE 1.90, anything else 1.80.  The element
    is the element column or - when that is empty - the first letter of the atom name (the rule family of sterics.is_hydrogen)."""
    el = atom.get("element", "").strip().upper()
    if not el:
        name = atom["name"].strip().upper().lstrip("0123456789")
        el = name[:1]
    return _RADII.get(el, _OTHER_RADIUS)


def atom_radii(atoms, index=None):
    """float32 [n]: element_radius of the atoms `index` (default: all) of pdbio.read_pdb records."""
    index = range(len(atoms)) if index is None else index
    return np.array([element_radius(atoms[int(i)]) for i in index], np.float32)


def residue_bsa(buried, radius, res, n_res, probe=PROBE, K=POINTS):
    """Per-residue buried area [.., n_res] float64 of per-atom point counts [.., n]: the points of each residue's atoms summed per radius
    value (sterics.residue_counts), then times the value's area per point, values in ascending order."""
    buried = np.asarray(buried)
    radius = np.asarray(radius, np.float32).reshape(-1)
    out = np.zeros(buried.shape[:-1] + (n_res,), np.float64)
    for v in np.unique(radius):
        m = radius == v
        R = float(v) + float(np.float32(probe))
        out = out + ST.residue_counts(buried[..., m], np.asarray(res)[m], n_res) * (4.0 * np.pi * R * R / K)
    return out


def write_interface_residues(path, keys, area):
    """--interface-residues: one line `side chain:resnum[icode] res_name area` per residue whose buried area is above 0.  keys / area: one
    (list of residue keys, areas) per side, receptor first."""
    with open(path, "w") as f:
        f.write("# side, residue, name, buried solvent-accessible area in A^2\n")
        for side, ks, ar in zip(("rec", "lig"), keys, area):
            for k, v in zip(ks, ar):
                if v > 0:
                    f.write(f"{side} {k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''} {k[3]} {float(v):.2f}\n")


def min_bsa_flags(bsa_values, threshold):
    """bool [P]: the poses whose bsa is below `threshold` A^2 (NaN: not flagged)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(bsa_values, np.float64) < float(threshold)
