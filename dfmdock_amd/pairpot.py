"""Tabulated pair potential and pair counts of an ensemble of rigid ligand poses - E = sum over heavy-atom pairs of
table[type_a][type_b][bin(r)], the shape of DFIRE, DOPE, ITScore-PP, ZRANK's ACE term or a table fitted to one's own decoys - and the
pair-count histogram N[type_a][type_b][bin] that such a potential is a linear function of: the float64 numpy definition of
dfm_pose_pairpot (include/dfmdock_amd.h, kernels_pairpot.hip) and its host finishes.  No reference counterpart.  The project ships NO
table and no typing scheme: the table, its bin edges and its type names come from the user's file, and nothing is claimed about the
ranking quality of any potential.

  pose p of the ligand   sterics.pose_atoms
  table_q                int64(rint(float64(table) * 2^20)), ties to even: table [T,T,NB] float32, kcal/mol, |x| <= 1024, indexed
                         (ligand type, receptor type, bin); it need not be symmetric
  e2                     float64(edges[k]) * float64(edges[k]): exact, 24 bits times 24 bits; edges [NB+1] float32, strictly ascending,
                         0 <= edges[0], edges[NB] <= 16
  per pair               r2 = (dx*dx + dy*dy) + dz*dz in float64 on the widened float32 receptor atom and the float64 posed ligand atom
                         (ifenergy.near_r2); the pair counts iff e2[0] <= r2 < e2[NB] (a NaN is no pair); its bin is
                         k = #{j : e2[j] <= r2} - 1.  No square root anywhere
  energy_q, n_pairs      [P] int64: the sum of table_q[ta, tb, k] over the pose's pairs; their number (also where the table holds 0)
  lig_q                  [P,Al] int64: the same sum per ligand atom, in the caller's atom order
  counts                 [P,T,T,NB] int32: the pairs by (ligand type, receptor type, bin)

Integer sums do not depend on their order, so the device's results equal these integer for integer, whatever the blocks and chunks.
Energies in kcal/mol are q * 2^-20 (kcal).  A pose with a non-finite transform gets zeros.
"""
from __future__ import annotations

import numpy as np

from . import ifenergy as IE
from . import sterics as ST

QUANTA = 1048576.0            # 2^20 per kcal/mol
MAX_TYPES = 256
MAX_BINS = 64
MAX_CUTOFF = 16.0             # the largest reach of a rigid-pose frame
MAX_ENTRY = 1024.0            # kcal/mol


def check_edges(edges):
    """Bin edges [NB+1] as the device takes them: float32.  ValueError outside the limits of dfm_pairpot_create: 1 <= NB <= 64, finite,
    strictly ascending, edges[0] >= 0, edges[NB] <= 16."""
    e = np.asarray(edges, np.float32)
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError(f"edges must be [NB+1] with 1 <= NB <= {MAX_BINS}, got shape {e.shape}")
    if not np.isfinite(e).all():
        raise ValueError("edges must be finite")
    if not (np.diff(e.astype(np.float64)) > 0).all():
        raise ValueError("edges must be strictly ascending")
    if not (e[0] >= 0 and e[-1] <= MAX_CUTOFF):
        raise ValueError(f"edges must lie in [0, {MAX_CUTOFF:g}], got {float(e[0])} .. {float(e[-1])}")
    return e


def check_table(table, NB=None):
    """The table [T,T,NB] as the device takes it: float32.  ValueError outside the limits of dfm_pairpot_create: 1 <= T <= 256, as many
    bins as the edges leave (`NB`, when given), finite, |x| <= 1024."""
    t = np.asarray(table, np.float32)
    if t.ndim != 3 or t.shape[0] != t.shape[1] or not 1 <= t.shape[0] <= MAX_TYPES or not 1 <= t.shape[2] <= MAX_BINS:
        raise ValueError(f"table must be [T,T,NB] with 1 <= T <= {MAX_TYPES} and 1 <= NB <= {MAX_BINS}, got shape {t.shape}")
    if NB is not None and t.shape[2] != int(NB):
        raise ValueError(f"table has {t.shape[2]} bins, the edges leave {int(NB)}")
    if not np.isfinite(t).all() or not (np.abs(t) <= MAX_ENTRY).all():
        raise ValueError(f"table entries must be finite and at most {MAX_ENTRY:g} kcal/mol in magnitude")
    return t


def check_types(types, n, T, who="types"):
    """Atom types [n] as the device takes them: int32 in [0, T)."""
    t = np.asarray(types)
    if t.shape != (n,) or t.dtype.kind not in "iu":
        raise ValueError(f"{who} must be {n} integers, got {t.dtype} {t.shape}")
    if n and (t.min() < 0 or t.max() >= T):
        raise ValueError(f"{who} must be in [0, {T})")
    return t.astype(np.int32)


def quantise(table):
    """table_q = int64(rint(float64(table) * 2^20)): ties to even; |q| <= 2^30."""
    return np.rint(np.asarray(table, np.float32).astype(np.float64) * QUANTA).astype(np.int64)


def edges2(edges):
    """e2 [NB+1] float64 = the squares of the float32 edges, exact."""
    e = np.asarray(edges, np.float32).astype(np.float64)
    return e * e


def bin_of(r2, e2):
    """k = #{j : e2[j] <= r2} - 1 for r2 [n] float64: -1 below e2[0], NB at and above e2[NB]."""
    return np.searchsorted(e2, np.asarray(r2, np.float64), side="right") - 1


def pair_potential(rec_atoms, rec_type, lig_atoms, lig_type, center, rot, tr, edges, table, per_atom=False, counts=False, shortcut=True):
    """The definition.  rec_atoms [Ar,3], lig_atoms [Al,3], rec_type [Ar] / lig_type [Al] in [0, T), center [3], rot [P,3] axis-angle,
    tr [P,3], edges [NB+1], table [T,T,NB] (ligand type, receptor type, bin).  Returns {energy_q, n_pairs [P] int64} and, with `per_atom`,
    lig_q [P,Al] int64, with `counts`, counts [P,T,T,NB] int32."""
    e = check_edges(edges)
    NB = e.size - 1
    tq = quantise(check_table(table, NB))
    T = tq.shape[0]
    rec = np.asarray(rec_atoms, np.float32).reshape(-1, 3)
    lig = np.asarray(lig_atoms, np.float32).reshape(-1, 3)
    rt, lt = check_types(rec_type, rec.shape[0], T, "rec_type"), check_types(lig_type, lig.shape[0], T, "lig_type")
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    if rot.shape != tr.shape:
        raise ValueError(f"rot and tr must both be [P,3], got {rot.shape} and {tr.shape}")
    e2 = edges2(e)
    P, Al = rot.shape[0], lig.shape[0]
    out = {"energy_q": np.zeros(P, np.int64), "n_pairs": np.zeros(P, np.int64)}
    if per_atom:
        out["lig_q"] = np.zeros((P, Al), np.int64)
    if counts:
        out["counts"] = np.zeros((P, T, T, NB), np.int32)
    for p in range(P):
        if not (np.isfinite(rot[p]).all() and np.isfinite(tr[p]).all()):
            continue
        a, b, r2 = IE.near_r2(rec, ST.pose_atoms(lig, center, rot[p], tr[p]), float(e[NB]), shortcut)
        keep = r2 >= e2[0]
        a, b, r2 = a[keep], b[keep], r2[keep]
        k = bin_of(r2, e2)
        q = tq[lt[a], rt[b], k]
        out["energy_q"][p], out["n_pairs"][p] = q.sum(), r2.size
        if per_atom:
            np.add.at(out["lig_q"][p], a, q)
        if counts:
            np.add.at(out["counts"][p], (lt[a], rt[b], k), 1)
    return out


def kcal(q):
    """Quanta -> kcal/mol (float64; exact for |q| < 2^53)."""
    return np.asarray(q, np.int64).astype(np.float64) / QUANTA


def save(path, edges, table, type_names):
    """Write a potential file: an .npz with `edges` [NB+1] float32, `table` [T,T,NB] float32 (ligand type, receptor type, bin; kcal/mol)
    and `type_names` [T] (atom_types explains the names).  The checks of check_edges / check_table apply."""
    e = check_edges(edges)
    t = check_table(table, e.size - 1)
    names = np.asarray([str(n) for n in type_names])
    if names.shape != (t.shape[0],) or len(set(names.tolist())) != names.size:
        raise ValueError(f"type_names must be {t.shape[0]} distinct names, got {names.shape}")
    with open(path, "wb") as f:      # (a file object: numpy appends no suffix)
        np.savez(f, edges=e, table=t, type_names=names)


def load(path):
    """Read a potential file written by `save` (or by anything that writes the same three arrays), allow_pickle=False.  Returns
    {edges, table, type_names (a list of str)}, checked."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("edges", "table", "type_names") if k not in z.files]
        if missing:
            raise ValueError(f"{path}: no array named {', '.join(missing)}")
        e, t, names = z["edges"], z["table"], z["type_names"]
    e = check_edges(e)
    t = check_table(t, e.size - 1)
    if names.dtype.kind not in "US" or names.shape != (t.shape[0],):
        raise ValueError(f"{path}: type_names must be {t.shape[0]} strings, got {names.dtype} {names.shape}")
    names = [n.decode() if isinstance(n, bytes) else str(n) for n in names.tolist()]
    if len(set(names)) != len(names):
        raise ValueError(f"{path}: type_names are not distinct")
    return {"edges": e, "table": t, "type_names": names}


def atom_types(atoms, type_names, heavy_index=None):
    """(types [n] int32, kept_index [n] int64, n_untyped) of the atoms `heavy_index` (default: sterics.heavy_atoms) of pdbio.read_pdb
    records.  A type name is one of RES:ATOM, RES:*, *:ATOM, @ELEMENT or *; an atom takes the first of these, in that order, that is in
    `type_names` (its position there is the type).  An atom that matches none is left out - kept_index lists the others, as indices
    into `atoms` - and counted in n_untyped.  So the 167 residue-specific heavy-atom types, the 20 residue types, element types and
    anything between are all a matter of the file's names; no typing scheme is built in."""
    index = ST.heavy_atoms(atoms) if heavy_index is None else np.asarray(heavy_index, np.int64)
    pos = {}
    for t, n in enumerate(type_names):
        pos.setdefault(str(n), t)
    types, kept, untyped = [], [], 0
    for i in index:
        a = atoms[int(i)]
        res, name = a["res_name"].strip(), a["name"].strip()
        for cand in (f"{res}:{name}", f"{res}:*", f"*:{name}", "@" + IE.element_of(a), "*"):
            if cand in pos:
                types.append(pos[cand])
                kept.append(int(i))
                break
        else:
            untyped += 1
    return np.asarray(types, np.int32), np.asarray(kept, np.int64), untyped


def residue_energy(per_atom, res, n_res):
    """Per-atom quanta [.., n] summed per residue -> [.., n_res] int64 (sterics.residue_counts)."""
    return ST.residue_counts(per_atom, res, n_res)


def write_pairpot_residues(path, keys, q):
    """--pairpot-residues: one line `chain:resnum[icode] res_name energy` (kcal/mol) per ligand residue with a nonzero sum."""
    with open(path, "w") as f:
        f.write("# ligand residue, name, tabulated pair potential in kcal/mol\n")
        for k, v in zip(keys, q):
            if v != 0:
                f.write(f"{k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''} {k[3]} {float(kcal(v)):.6f}\n")
