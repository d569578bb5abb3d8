"""PDB front / back end of the docking drivers without biotite.  Host side only.

  read_pdb / backbone_from_atoms   <- get_info_from_pdb            (src/inference_base.py:72-126)
  read_models / match_model        every model of a decoy file, matched to the input pair residue by residue (no reference counterpart)
  apply_pose_all_atom              <- modify_aa_coords             (src/inference_base.py:354-364)
  write_complex_pdb                <- combine_atom_arrays + PDBFile.write (src/inference_base.py:37-66,:659-668)
  place_fourth_atom, full_backbone <- utils/pdb.py:31-56, inference_mlsb.py:68-85 (O / virtual-CB placement)
  write_backbone_pdb, write_trajectory_pdb <- utils/pdb.py:59-84 (save_PDB), inference_mlsb.py:130-159 (save_trj)
"""
from __future__ import annotations

import numpy as np

THREE_TO_ONE = {
    "ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H",
    "ILE": "I", "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W",
    "TYR": "Y", "VAL": "V",
}   # residue_constants.py:959 restype_3to1
ONE_TO_THREE = {v: k for k, v in THREE_TO_ONE.items()}
ONE_TO_THREE.update({"-": "GAP", "X": "URI"})   # utils/pdb.py:4-27


def read_pdb(path):
    """ATOM records of the first model (first alternate location only) as a list of dicts."""
    atoms = []
    with open(path) as f:
        for line in f:
            rec = line[:6]
            if rec.startswith("ENDMDL"):
                break
            a = _atom_record(line)
            if a is not None:
                atoms.append(a)
    return atoms


def _atom_record(line):
    """One ATOM / HETATM line as read_pdb's dict, or None for any other record and for an alternate location past the first
    (read_pdb's rule: blank or A)."""
    rec = line[:6]
    if rec not in ("ATOM  ", "HETATM") or line[16] not in (" ", "A"):
        return None
    return {
        "hetero": rec == "HETATM", "name": line[12:16].strip(), "res_name": line[17:20].strip(),
        "chain": line[21], "res_id": int(line[22:26]), "ins": line[26],
        "coord": (float(line[30:38]), float(line[38:46]), float(line[46:54])),
        "element": line[76:78].strip() if len(line) >= 78 else "",
    }


def read_models(path):
    """The atom records of EVERY model of a PDB file, as a list (one entry per MODEL ... ENDMDL block, in file order) of read_pdb's
    lists of dicts, under read_pdb's alternate-location rule.  A MODEL record opens a block and closes the one before it (files of
    write_trajectory_pdb hold no ENDMDL); a file without MODEL records is one model.  A MODEL record followed at once by another, or
    by ENDMDL, is a model without atoms: it keeps its place in the list, and match_model reports its first ligand residue missing."""
    models, cur, in_model = [], [], False
    with open(path) as f:
        for line in f:
            rec = line[:6]
            if rec.startswith("MODEL"):
                if in_model or cur:
                    models.append(cur)
                cur, in_model = [], True
            elif rec.startswith("ENDMDL"):
                models.append(cur)
                cur, in_model = [], False
            else:
                a = _atom_record(line)
                if a is not None:
                    cur.append(a)
    if in_model or cur:
        models.append(cur)
    return models


def _chain_ids(residues):
    out = []
    for key in residues:
        if key[0] not in out:
            out.append(key[0])
    return out


def match_model(atoms, rec, lig, rec_chains=None, lig_chains=None, source="decoy", model=1):
    """The backbone of one decoy model (`atoms`: one entry of read_models) in the residue order of the input pair (rec, lig: the dicts
    of backbone_from_atoms): (lig_bb [L,3,3], rec_bb [R,3,3] or None) float64.  The model's residues are matched to the inputs'
    `residues` keys - chain, number, insertion code and name.  The ligand must be complete and in the input's order; the receptor is
    used when the model holds any atom of a receptor chain, and must then be complete and in order as well; atoms of other residues
    (and HETATM records) are ignored.  rec_chains / lig_chains: the chain ids the two sides have IN THE DECOY FILE, one per chain id
    of the input file in its order of appearance (default: the input files' own ids).  Raises ValueError naming `source`, `model` and
    the first residue that is missing or out of place; and, when the two inputs share a chain id and no chains are given, asking for
    them."""
    ids = {"rec": _chain_ids(rec["residues"]), "lig": _chain_ids(lig["residues"])}
    given = {"rec": rec_chains, "lig": lig_chains}
    if rec_chains is None and lig_chains is None and set(ids["rec"]) & set(ids["lig"]):
        raise ValueError(f"receptor and ligand input share the chain id(s) {sorted(set(ids['rec']) & set(ids['lig']))}: "
                         "name the chains the two sides have in the decoys (rec_chains / lig_chains, --decoy-chains RCHAINS LCHAINS)")
    maps = {}
    for side in ("rec", "lig"):
        g = ids[side] if given[side] is None else list(given[side])
        if len(g) != len(ids[side]):
            raise ValueError(f"{side}_chains {''.join(g)!r} must name one chain per chain of the input ({''.join(ids[side])!r})")
        maps[side] = dict(zip(ids[side], g))
    if set(maps["rec"].values()) & set(maps["lig"].values()):
        raise ValueError("rec_chains and lig_chains must not share a chain id")
    found, order = {}, {}
    for a in atoms:
        if a["hetero"] or a["name"] not in ("N", "CA", "C"):
            continue
        key = (a["chain"], a["res_id"], a["ins"], a["res_name"])
        order.setdefault(key, len(order))
        found.setdefault(key, {}).setdefault(a["name"], a["coord"])

    def side_bb(side, chain):
        bb, last = np.empty((len(chain["residues"]), 3, 3), np.float64), -1
        for i, key in enumerate(chain["residues"]):
            k = (maps[side][key[0]],) + tuple(key[1:])
            label = f"{k[3]} {k[0]}{k[1]}{k[2].strip()}"
            if k not in found or len(found[k]) < 3:
                raise ValueError(f"{source}, model {model}: {'ligand' if side == 'lig' else 'receptor'} residue {label} is missing"
                                 + ("" if k not in found else " an N, CA or C atom"))
            if order[k] < last:
                raise ValueError(f"{source}, model {model}: {'ligand' if side == 'lig' else 'receptor'} residue {label} is out of place")
            last = order[k]
            bb[i] = [found[k]["N"], found[k]["CA"], found[k]["C"]]
        return bb
    lig_bb = side_bb("lig", lig)
    rec_here = set(maps["rec"].values())
    rec_bb = side_bb("rec", rec) if any(a["chain"] in rec_here and not a["hetero"] for a in atoms) else None
    return lig_bb, rec_bb


def backbone_from_atoms(atoms):
    """get_info_from_pdb semantics: drop HETATM; a residue (keyed by res_id, as the reference does) is kept when
    it has N, CA and C; seq via 3->1 (unknown -> X); bb_coords [n,3,3] float64 in file order; residues [n] their keys."""
    atoms = [a for a in atoms if not a["hetero"]]
    names_by_res = {}
    for a in atoms:
        names_by_res.setdefault(a["res_id"], set()).add(a["name"])
    valid = {r for r, names in names_by_res.items() if {"N", "CA", "C"} <= names}
    kept = [a for a in atoms if a["res_id"] in valid]
    seq, order, last = [], [], None
    for a in kept:      # residue starts: change of (chain, res_id, ins, res_name)
        key = (a["chain"], a["res_id"], a["ins"], a["res_name"])
        if key != last:
            order.append(key)
            seq.append(THREE_TO_ONE.get(a["res_name"], "X"))
            last = key
    pick = lambda nm: np.array([a["coord"] for a in kept if a["name"] == nm], dtype=np.float64)
    n, ca, c = pick("N"), pick("CA"), pick("C")
    if not (len(n) == len(ca) == len(c) == len(seq)):
        raise ValueError("backbone atom counts do not match the residue count (duplicate residue ids?)")
    bb = np.stack([n, ca, c], axis=1)
    aa = np.array([a["coord"] for a in atoms], dtype=np.float64)
    # residues: the (chain, res_id, ins, res_name) key of every kept residue, in bb_coords order (restraint files name residues by it)
    return {"atoms": atoms, "seq": "".join(seq), "aa_coords": aa, "bb_coords": bb, "residues": order}


def axis_angle_to_matrix(aa):
    """geometry.py:154-198 in float64 (host-side pose application)."""
    aa = np.asarray(aa, np.float64).reshape(3)
    ang = np.linalg.norm(aa)
    s = 0.5 - ang * ang / 48.0 if abs(ang) < 1e-6 else np.sin(0.5 * ang) / ang
    r, (i, j, k) = np.cos(0.5 * ang), aa * s
    two_s = 2.0 / (r * r + i * i + j * j + k * k)
    return np.array([[1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)],
                     [two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)],
                     [two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)]])


def apply_pose_all_atom(aa_coords, bb_coords, rot, tr, center="ca"):
    """Rigid (rot, tr) of the sampler applied to all atoms.  center="ca": about the ORIGINAL backbone CA centroid
    (modify_aa_coords of src/inference_base.py:354-364, first model family); center="all_atoms": about the mean of the
    all-atom array itself, which is what the second family's script does (src/inference.py:256-266)."""
    if center == "all_atoms":
        center = np.asarray(aa_coords, np.float64).reshape(-1, 3).mean(axis=0)
    else:
        center = np.asarray(bb_coords, np.float64)[:, 1].mean(axis=0)
    R = axis_angle_to_matrix(np.asarray(rot).reshape(3))
    return (np.asarray(aa_coords, np.float64) - center) @ R.T + center + np.asarray(tr, np.float64).reshape(3)


def write_complex_pdb(path, rec_atoms, lig_atoms, lig_coords, remarks=None):
    """Receptor atoms as read + ligand atoms at `lig_coords`, one PDB model.  `remarks`: lines written as REMARK records on top."""
    with open(path, "w") as f:
        for r in remarks or ():
            f.write("REMARK " + r + "\n")
        k = 0
        for atoms, coords in ((rec_atoms, None), (lig_atoms, lig_coords)):
            for idx, a in enumerate(atoms):
                x, y, z = a["coord"] if coords is None else coords[idx]
                k += 1
                name = a["name"] if len(a["name"]) == 4 else " " + a["name"]
                f.write("%-6s%5d %-4s %3s %s%4d%s   %8.3f%8.3f%8.3f%6.2f%6.2f          %2s\n" % (
                    "HETATM" if a["hetero"] else "ATOM", k % 100000, name, a["res_name"], a["chain"], a["res_id"], a["ins"],
                    x, y, z, 1.0, 0.0, a["element"]))
        f.write("END\n")


def place_fourth_atom(a, b, c, length, planar, dihedral):
    """utils/pdb.py:31-56."""
    bc = b - c
    bc = bc / np.linalg.norm(bc, axis=-1, keepdims=True)
    n = np.cross(np.broadcast_to(b - a, bc.shape), bc)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    m = [bc, np.cross(n, bc), n]
    d = [length * np.cos(planar), length * np.sin(planar) * np.cos(dihedral), -length * np.sin(planar) * np.sin(dihedral)]
    return c + sum(mi * di for mi, di in zip(m, d))


def full_backbone(coords):
    """[n,3,3] (N,CA,C) -> [n,5,3] (N,CA,C,O,CB); O from the NEXT residue's N, wrapping at the end like the reference."""
    coords = np.asarray(coords, np.float32)
    N, CA, C = coords[:, 0], coords[:, 1], coords[:, 2]
    b, c = CA - N, C - CA
    a = np.cross(b, c)
    CB = np.float32(-0.58273431) * a + np.float32(0.56802827) * b - np.float32(0.54067466) * c + CA
    O = place_fourth_atom(np.roll(N, -1, axis=0), CA, C, np.float32(1.231), np.float32(2.108), np.float32(-3.142))
    return np.stack([N, CA, C, O.astype(np.float32), CB], axis=1)


def write_backbone_pdb(path, coords5, seq, delim=-1, mode="a"):
    """utils/pdb.py:59-84 save_PDB: chain A for residues <= delim, B after; CB skipped for GLY."""
    names = ["N", "CA", "C", "O", "CB"]
    with open(path, mode) as f:
        k = 0
        for r, residue in enumerate(coords5):
            aa3 = ONE_TO_THREE[seq[r]]
            for a, atom in enumerate(residue):
                if aa3 == "GLY" and names[a] == "CB":
                    continue
                f.write("ATOM  %5d  %-2s  %3s %s%4d    %8.3f%8.3f%8.3f  %4.2f %4.2f\n" % (
                    k + 1, names[a], aa3, "A" if r <= delim else "B", r + 1, atom[0], atom[1], atom[2], 1, 0.0))
                k += 1


def write_trajectory_pdb(path, rec_frames, lig_frames, rec_seq, lig_seq):
    """inference_mlsb.py:130-159 save_trj: one MODEL per frame (N,CA,C,O,CB), appended."""
    open(path, "w").close()
    for i, (x1, x2) in enumerate(zip(rec_frames, lig_frames)):
        with open(path, "a") as f:
            f.write("MODEL        " + str(i) + "\n")
        write_backbone_pdb(path, full_backbone(np.concatenate([x1, x2], 0)), rec_seq + lig_seq, delim=len(rec_seq) - 1)
