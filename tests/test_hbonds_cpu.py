"""Interface hydrogen bonds and salt bridges without a GPU: the float64 definition dfmdock_amd/hbonds.py - its typing tables, its
per-pair tests on hand-built pairs and against an independent formulation (arccos and sqrt), its host finishes - the creator's host
preparation in dfm_poseprep.h (tests/hbond_prep_main.cpp under the address and undefined-behaviour sanitizers), the C ABI's layout and the
plumbing through the pair drivers and the command line with the device call stubbed."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_pair
from conftest import ROOT

D, A, CAT, AN, SC = 1, 2, 4, 8, 16
Z3 = np.zeros(3, np.float32)
Z13 = np.zeros((1, 3), np.float32)

# what the issue's tables say, residue by residue of the file below: (residue number, atom) -> (role, antecedent)
BACKBONE = {"N": "CA", "O": "C", "OXT": "C"}
RESIDUES = [  # (name, the side-chain atoms written after N CA C O)
    ("ALA", ["CB"]), ("PRO", ["CB", "CG", "CD"]), ("ARG", ["CB", "CG", "CD", "NE", "CZ", "NH1", "NH2"]), ("ASN", ["CB", "CG", "OD1", "ND2"]),
    ("GLN", ["CB", "CG", "CD", "OE1", "NE2"]), ("ASP", ["CB", "CG", "OD1", "OD2"]), ("GLU", ["CB", "CG", "CD", "OE1", "OE2"]),
    ("HIS", ["CB", "CG", "ND1", "CD2", "CE1", "NE2"]), ("LYS", ["CB", "CG", "CD", "CE", "NZ"]), ("SER", ["CB", "OG"]),
    ("THR", ["CB", "OG1", "CG2"]), ("TYR", ["CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ", "OH"]),
    ("TRP", ["CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2"]), ("CYS", ["CB", "SG"]), ("MET", ["CB", "CG", "SD", "CE"]),
    ("MSE", ["CB", "CG", "SE", "CE"]), ("ARG", ["CB", "CG", "CD", "NE", "NH1", "NH2"]),      # 17: an ARG without CZ
    ("GLY", ["OXT"]),
]
SIDE = {("ARG", "NE"): (D | CAT | SC, "CZ"), ("ARG", "NH1"): (D | CAT | SC, "CZ"), ("ARG", "NH2"): (D | CAT | SC, "CZ"),
        ("ASN", "OD1"): (A | SC, "CG"), ("ASN", "ND2"): (D | SC, "CG"), ("GLN", "OE1"): (A | SC, "CD"), ("GLN", "NE2"): (D | SC, "CD"),
        ("ASP", "OD1"): (A | AN | SC, "CG"), ("ASP", "OD2"): (A | AN | SC, "CG"), ("GLU", "OE1"): (A | AN | SC, "CD"),
        ("GLU", "OE2"): (A | AN | SC, "CD"), ("HIS", "ND1"): (D | A | CAT | SC, "CG"), ("HIS", "NE2"): (D | A | CAT | SC, "CE1"),
        ("LYS", "NZ"): (D | CAT | SC, "CE"), ("SER", "OG"): (D | A | SC, "CB"), ("THR", "OG1"): (D | A | SC, "CB"),
        ("TYR", "OH"): (D | A | SC, "CZ"), ("TRP", "NE1"): (D | SC, "CD1")}


def typing_pdb(path):
    """One chain with every residue type that has side-chain roles, a PRO, the chain start, an OXT, an ARG without CZ, an MSE, one
    hydrogen and one HETATM; every atom at its own coordinate (serial, residue, 0.5).  Returns {(residue number, atom): coordinate}."""
    lines, where, serial = [], {}, 0
    for r, (name, side) in enumerate(RESIDUES, 1):
        for atom in ["N", "CA", "C", "O"] + side:
            serial += 1
            xyz = (float(serial), float(r), 0.5)
            where[(r, atom)] = xyz
            el = "SE" if atom == "SE" else atom[0]
            lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (serial, " " + atom if len(atom) < 4 else atom, name, r, *xyz, 1.0, 0.0, el))
    lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (serial + 1, " H", "ALA", 1, 0.0, 0.0, 0.0, 1.0, 0.0, "H"))
    lines.append("HETATM%5d %-4s %3s A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (serial + 2, " O", "HOH", 99, 0.0, 0.0, 0.0, 1.0, 0.0, "O"))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\nEND\n")
    return where


def test_typing_tables(tmp_path):
    from dfmdock_amd import hbonds as HB
    from dfmdock_amd import pdbio, sterics as ST
    where = typing_pdb(tmp_path / "t.pdb")
    atoms = pdbio.read_pdb(tmp_path / "t.pdb")
    pa = HB.polar_atoms(atoms)
    heavy = ST.heavy_atoms(atoms)
    assert (HB.DONOR, HB.ACCEPTOR, HB.CATION, HB.ANION, HB.SIDECHAIN) == (D, A, CAT, AN, SC)
    want = {}
    for r, (name, side) in enumerate(RESIDUES, 1):
        table_name = "MET" if name == "MSE" else name
        for atom in ["N", "CA", "C", "O"] + side:
            if atom == "N":
                role = (0 if name == "PRO" else D) | (CAT if r == 1 else 0)
                back = "CA"
            elif atom in ("O", "OXT"):
                role = A | (AN if "OXT" in side else 0)
                back = "C"
            elif (table_name, atom) in SIDE:
                role, back = SIDE[(table_name, atom)]
            else:
                continue
            if role and (r, back) in where:
                want[(r, atom)] = (role, where[(r, back)])
    got = {}
    for n in range(len(pa["role"])):
        a = atoms[int(heavy[pa["index"][n]])]
        assert np.array_equal(pa["xyz"][n], np.float32(a["coord"]))
        got[(a["res_id"], a["name"])] = (int(pa["role"][n]), tuple(float(v) for v in pa["ante"][n]))
        assert pa["keys"][pa["res"][n]][1] == a["res_id"]
    assert got == want
    # spot checks, written out: the chain start, PRO, the terminus, HIS, the neither-nor atoms, MSE
    assert got[(1, "N")][0] == D | CAT and (2, "N") not in got and got[(2, "O")][0] == A and got[(3, "N")][0] == D
    assert got[(18, "O")][0] == A | AN and got[(18, "OXT")][0] == A | AN and got[(18, "OXT")][1] == where[(18, "C")]
    assert got[(8, "ND1")] == (D | A | CAT | SC, where[(8, "CG")]) and got[(8, "NE2")] == (D | A | CAT | SC, where[(8, "CE1")])
    assert got[(13, "NE1")] == (D | SC, where[(13, "CD1")]) and got[(9, "NZ")] == (D | CAT | SC, where[(9, "CE")])
    assert not any(k in got for k in ((14, "SG"), (15, "SD"), (16, "SE"), (16, "SD")))
    assert [k for k in got if k[0] == 16] == [(16, "N"), (16, "O")]            # MSE is typed as MET: the backbone only
    assert pa["untyped"] == 3 and not any(k[0] == 17 and k[1] in ("NE", "NH1", "NH2") for k in got)      # the ARG without CZ
    assert pa["n_res"] == 18 and pa["res"].dtype == np.int32 and pa["role"].dtype == np.uint8 and pa["xyz"].dtype == np.float32
    assert pa["res"].tolist() == [k[0] - 1 for k in got]                        # residue_of_atoms numbering over the heavy atoms
    assert len(heavy) == len(atoms) - 2 and "neither" in HB.__doc__ and "CYS SG and MET SD" in HB.__doc__
    # a restricted heavy index is honoured: without the CA atoms no backbone N has its antecedent
    no_ca = np.array([i for i in heavy if atoms[int(i)]["name"] != "CA"])
    p2 = HB.polar_atoms(atoms, no_ca)
    assert p2["untyped"] == 3 + 17 and not (p2["role"] & D).astype(bool)[[atoms[int(no_ca[i])]["name"] == "N" for i in p2["index"]]].any()


def chain(xyz, ante, role, res=None, n_res=None):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    res = np.zeros(len(xyz), np.int32) if res is None else np.asarray(res, np.int32)
    return {"xyz": xyz, "ante": np.asarray(ante, np.float32).reshape(-1, 3), "role": np.asarray(role, np.uint8).reshape(-1), "res": res,
            "n_res": int(res.max()) + 1 if n_res is None else n_res}


def one(X, XA, rx, Y=(0, 0, 0), YA=(-1.25, 0, 0), ry=A, **kw):
    """One ligand atom X (antecedent XA, role rx) against one receptor atom Y under the identity pose about the origin: R = I and tr = 0
    leave every coordinate as it is."""
    from dfmdock_amd import hbonds as HB
    return HB.hbonds(chain(Y, YA, ry), chain(X, XA, rx), Z3, Z13, Z13, per_atom=True, **kw)


def test_hand_built_pairs():
    """The receptor acceptor at the origin with its antecedent on -x; the ligand donor on +x: both angles are 180 degrees unless the case
    says otherwise.  Every coordinate is representable."""
    f32 = np.float32
    n = lambda o: (int(o["n_hbond"][0]), o["hb_kind"][0].tolist())
    below = np.nextafter(f32(3.5), f32(0))
    assert n(one((3.5, 0, 0), (4.5, 0, 0), D)) == (0, [0, 0, 0])                 # r2 == cutoff^2: strict
    o = one((below, 0, 0), (4.5, 0, 0), D)
    assert n(o) == (1, [1, 0, 0]) and o["rec_hb"].tolist() == [[1]] and o["lig_hb"].tolist() == [[1]] and o["n_salt"][0] == 0
    assert n(one((below, 0, 0), (4.5, 0, 0), D, hb_cutoff=float(below))) == (0, [0, 0, 0])      # the cutoff is the float32, widened
    # the angle at X: exactly 90 degrees (du == 0) is a bond, 89 is not
    assert n(one((3, 0, 0), (3, 1, 0), D)) == (1, [1, 0, 0])
    u = lambda deg: (3.0 - np.cos(np.radians(deg)), np.sin(np.radians(deg)), 0.0)      # X + the unit vector at `deg` from X -> Y
    assert n(one((3, 0, 0), u(89), D)) == (0, [0, 0, 0]) and n(one((3, 0, 0), u(91), D)) == (1, [1, 0, 0])
    # the angle at Y likewise
    assert n(one((3, 0, 0), (4, 0, 0), D, YA=(0, -1, 0))) == (1, [1, 0, 0])
    assert n(one((3, 0, 0), (4, 0, 0), D, YA=(np.cos(np.radians(89)), np.sin(np.radians(89)), 0))) == (0, [0, 0, 0])
    # min_angle 120: 119 is no bond, 121 is, at either atom
    assert n(one((3, 0, 0), u(119), D, min_angle=120)) == (0, [0, 0, 0]) and n(one((3, 0, 0), u(121), D, min_angle=120)) == (1, [1, 0, 0])
    v = lambda deg: (np.cos(np.radians(deg)), np.sin(np.radians(deg)), 0.0)
    assert n(one((3, 0, 0), (4, 0, 0), D, YA=v(119), min_angle=120)) == (0, [0, 0, 0])
    assert n(one((3, 0, 0), (4, 0, 0), D, YA=v(121), min_angle=120)) == (1, [1, 0, 0])
    # roles: donor - donor and acceptor - acceptor never, either direction does, side chains are counted
    assert n(one((3, 0, 0), (4, 0, 0), D, ry=D)) == (0, [0, 0, 0]) and n(one((3, 0, 0), (4, 0, 0), A, ry=A)) == (0, [0, 0, 0])
    assert n(one((3, 0, 0), (4, 0, 0), A, ry=D)) == (1, [1, 0, 0]) and n(one((3, 0, 0), (4, 0, 0), A | SC, ry=D)) == (1, [0, 1, 0])
    assert n(one((3, 0, 0), (4, 0, 0), CAT | AN | SC, ry=D | A)) == (0, [0, 0, 0])
    # SER OG with THR OG1: complementary in both directions, one bond
    assert n(one((3, 0, 0), (4, 0, 0), D | A | SC, ry=D | A | SC)) == (1, [0, 0, 1])
    # a coincident antecedent: uu == 0 gives du == 0, which passes du <= 0 and 0 >= c2 * 0 at any min_angle
    assert n(one((3, 0, 0), (3, 0, 0), D)) == (1, [1, 0, 0]) and n(one((3, 0, 0), (3, 0, 0), D, min_angle=150)) == (1, [1, 0, 0])
    assert n(one((3, 0, 0), (4, 0, 0), D, YA=(0, 0, 0), min_angle=150)) == (1, [1, 0, 0])
    # a hydrogen bond and a salt-bridge pair at once: both are counted (ARG NH1 with ASP OD1)
    o = one((3, 0, 0), (4, 0, 0), D | CAT | SC, ry=A | AN | SC)
    assert n(o) == (1, [0, 0, 1]) and o["n_salt"][0] == 1 and o["n_salt_atoms"][0] == 1 and o["rec_sb"].tolist() == [[1]]
    # the salt cutoff: strict, and independent of the angles and of the hydrogen-bond cutoff
    assert one((4, 0, 0), (3, 0, 0), CAT, ry=AN)["n_salt_atoms"][0] == 0
    o = one((np.nextafter(f32(4), f32(0)), 0, 0), (3, 0, 0), CAT, ry=AN)
    assert o["n_salt_atoms"][0] == 1 and o["n_salt"][0] == 1 and o["n_hbond"][0] == 0
    # a pose with a non-finite transform gets zeros
    from dfmdock_amd import hbonds as HB
    rec, lig = chain((0, 0, 0), (-1.25, 0, 0), A | AN), chain((3, 0, 0), (4, 0, 0), D | CAT)
    rot = np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [0, 0, 0]])
    tr = np.float32([[0, 0, 0], [0, 0, 0], [0, np.inf, 0], [0, 0, 0]])
    o = HB.hbonds(rec, lig, Z3, rot, tr, per_atom=True)
    assert o["n_hbond"].tolist() == [1, 0, 0, 1] and o["n_salt"].tolist() == [1, 0, 0, 1] and o["lig_sb"][:, 0].tolist() == [1, 0, 0, 1]
    assert all(v.dtype == np.int32 for v in o.values()) and o["hb_kind"].shape == (4, 3) and o["rec_hb"].shape == (4, 1)


def test_salt_bridges_are_residue_pairs():
    from dfmdock_amd import hbonds as HB
    arg = chain([(0, 0, 0), (0, 2, 0)], [(-1, 1, 0), (-1, 1, 0)], [D | CAT | SC] * 2, [0, 0], 3)                 # NH1, NH2 -> CZ
    asp = chain([(2.5, 0, 0), (2.5, 2, 0)], [(3.25, 1, 0), (3.25, 1, 0)], [A | AN | SC] * 2, [1, 1], 2)          # OD1, OD2 -> CG
    o = HB.hbonds(arg, asp, Z3, Z13, Z13, per_atom=True)
    assert o["n_salt"].tolist() == [1] and o["n_salt_atoms"].tolist() == [4] and o["rec_sb"].tolist() == [[2, 2]] and o["lig_sb"].tolist() == [[2, 2]]
    assert np.array_equal(HB.residue_bonds(o["rec_sb"], arg["res"], 3), [[4, 0, 0]]) and np.array_equal(HB.residue_bonds(o["lig_sb"][0], asp["res"], 2), [0, 4])
    two = chain(np.concatenate([asp["xyz"], [(1.5, 1, 2.5)]]), np.concatenate([asp["ante"], [(1.5, 1, 3.5)]]), [A | AN | SC] * 3, [1, 1, 0], 2)
    o = HB.hbonds(arg, two, Z3, Z13, Z13)
    assert o["n_salt"].tolist() == [2] and o["n_salt_atoms"].tolist() == [6]
    # the same atoms the other way round: the ligand holds the cations
    o = HB.hbonds(two, arg, Z3, Z13, Z13)
    assert o["n_salt"].tolist() == [2] and o["n_salt_atoms"].tolist() == [6]


def lump(rng, n, n_res, center=(0, 0, 0), spread=4.0):
    """n typed atoms about `center`, all five role bits drawn, antecedents 1.2 to 1.6 A away in a random direction."""
    xyz = (spread * rng.standard_normal((n, 3)) + np.float32(center)).astype(np.float32)
    d = rng.standard_normal((n, 3))
    ante = (xyz + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.2, 1.6, (n, 1))).astype(np.float32)
    return chain(xyz, ante, rng.integers(1, 32, n), rng.integers(0, n_res, n), n_res)


def poses(rng, P, s_rot=0.4, s_tr=1.5):
    return (s_rot * rng.standard_normal((P, 3))).astype(np.float32), (s_tr * rng.standard_normal((P, 3))).astype(np.float32)


def independent(rec, lig, center, rot, tr, hb_cutoff, min_angle, salt_cutoff, eps=1e-9):
    """Distances from sqrt, angles from arccos of normalised vectors: (hydrogen bond, salt pair, border) bool [P,Nl,Nr]; border: a
    distance within eps of a cutoff it is tested against, or an angle within eps rad of min_angle."""
    from dfmdock_amd import sterics as ST
    Y, YA = rec["xyz"].astype(np.float64), rec["ante"].astype(np.float64)
    rl, rr = lig["role"].astype(int)[:, None], rec["role"].astype(int)[None, :]
    compl = (((rl & D) > 0) & ((rr & A) > 0)) | (((rl & A) > 0) & ((rr & D) > 0))
    ionic = (((rl & CAT) > 0) & ((rr & AN) > 0)) | (((rl & AN) > 0) & ((rr & CAT) > 0))
    hc, sc, amin = float(np.float32(hb_cutoff)), float(np.float32(salt_cutoff)), np.radians(min_angle)
    hb, sb, border = [], [], []
    for p in range(len(rot)):
        X, XA = ST.pose_atoms(lig["xyz"], center, rot[p], tr[p]), ST.pose_atoms(lig["ante"], center, rot[p], tr[p])
        dv = Y[None, :, :] - X[:, None, :]
        dist = np.sqrt((dv ** 2).sum(-1))
        unit = dv / dist[..., None]
        u = (XA - X) / np.linalg.norm(XA - X, axis=1, keepdims=True)
        w = (YA - Y) / np.linalg.norm(YA - Y, axis=1, keepdims=True)
        ang_x = np.arccos(np.clip((u[:, None, :] * unit).sum(-1), -1, 1))
        ang_y = np.arccos(np.clip(-(w[None, :, :] * unit).sum(-1), -1, 1))
        hb.append(compl & (dist < hc) & (ang_x >= amin) & (ang_y >= amin))
        sb.append(ionic & (dist < sc))
        near = compl & (dist < hc + eps)
        border.append((compl & (np.abs(dist - hc) < eps)) | (ionic & (np.abs(dist - sc) < eps))
                      | (near & ((np.abs(ang_x - amin) < eps) | (np.abs(ang_y - amin) < eps))))
    return np.stack(hb), np.stack(sb), np.stack(border)


@pytest.mark.parametrize("min_angle, hb_cutoff, salt_cutoff", [(90.0, 3.5, 4.0), (120.0, 3.5, 4.0), (105.5, 8.0, 8.0)])
def test_definition_against_an_independent_formulation(min_angle, hb_cutoff, salt_cutoff):
    """Seed 11: the independent formulation alone leaves no pair within 1e-9 of a threshold here (the cap is 0.1 %)."""
    from dfmdock_amd import hbonds as HB
    rng = np.random.default_rng(11)
    rec, lig = lump(rng, 140, 17), lump(rng, 90, 11, center=(3, 0, 0))
    cen = lig["xyz"].astype(np.float64).mean(0).astype(np.float32)
    rot, tr = poses(rng, 6)
    hb, sb, border = independent(rec, lig, cen, rot, tr, hb_cutoff, min_angle, salt_cutoff)
    assert border.sum() <= 0.001 * border.size and hb.sum() > 20 and sb.sum() > 20
    got = HB.hbonds(rec, lig, cen, rot, tr, hb_cutoff, min_angle, salt_cutoff, per_atom=True)
    side = ((lig["role"].astype(int)[:, None] >> 4) & 1) + ((rec["role"].astype(int)[None, :] >> 4) & 1)
    for p in range(len(rot)):
        if border[p].any():      # left out: a pair the two formulations may round apart
            continue
        assert np.array_equal(got["lig_hb"][p], hb[p].sum(1)) and np.array_equal(got["rec_hb"][p], hb[p].sum(0)), p
        assert np.array_equal(got["lig_sb"][p], sb[p].sum(1)) and np.array_equal(got["rec_sb"][p], sb[p].sum(0)), p
        assert got["n_hbond"][p] == hb[p].sum() and got["n_salt_atoms"][p] == sb[p].sum()
        assert got["hb_kind"][p].tolist() == [int((hb[p] & (side == k)).sum()) for k in range(3)]
        j, i = np.nonzero(sb[p])
        assert got["n_salt"][p] == len(set(zip(rec["res"][i].tolist(), lig["res"][j].tolist())))
    # the call's own consistency
    assert np.array_equal(got["hb_kind"].sum(1), got["n_hbond"]) and np.array_equal(got["lig_hb"].sum(1), got["n_hbond"])
    assert np.array_equal(got["rec_hb"].sum(1), got["n_hbond"]) and np.array_equal(got["lig_sb"].sum(1), got["n_salt_atoms"])
    assert (got["n_salt"] <= got["n_salt_atoms"]).all()


def test_shortcut_changes_nothing():
    from dfmdock_amd import hbonds as HB
    rng = np.random.default_rng(4)
    rec, lig = lump(rng, 200, 20, spread=6.0), lump(rng, 120, 12, center=(6, 0, 0), spread=5.0)
    rot, tr = poses(rng, 5, 0.5, 4.0)
    tr[4] = (80.0, 0, 0)      # far away: the shortcut drops every atom
    for kw in ({}, {"min_angle": 130.0, "hb_cutoff": 5.0, "salt_cutoff": 3.0}):
        a = HB.hbonds(rec, lig, Z3, rot, tr, per_atom=True, shortcut=True, **kw)
        b = HB.hbonds(rec, lig, Z3, rot, tr, per_atom=True, shortcut=False, **kw)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
        assert a["n_hbond"][:4].sum() > 0 and a["n_salt"][:4].sum() > 0 and a["n_hbond"][4] == 0 and not a["lig_sb"][4].any()


def backbone_polar(bb, seq):
    """The polar atoms of a backbone [n,3,3] with the O that pdbio.full_backbone places: N of every non-PRO residue is a donor with
    antecedent CA, O an acceptor with antecedent C; no side-chain roles.  Atom order: the N atoms, then the O atoms."""
    from dfmdock_amd import pdbio
    a = pdbio.full_backbone(bb)      # N, CA, C, O, CB
    n = a.shape[0]
    keep = np.array([s != "P" for s in seq])
    return {"xyz": np.concatenate([a[keep, 0], a[:, 3]]), "ante": np.concatenate([a[keep, 1], a[:, 2]]),
            "role": np.concatenate([np.full(keep.sum(), D, np.uint8), np.full(n, A, np.uint8)]),
            "res": np.concatenate([np.nonzero(keep)[0], np.arange(n)]).astype(np.int32), "n_res": n}


def db5_definition():
    """The DB5 recipe of tests/test_gpu_sterics.py on the backbones' polar atoms: per complex (id, rec, lig, center, rot, tr, the
    definition's result with per-atom counts), 16 poses each from one default_rng(0) stream in db5_ids() order, defaults throughout."""
    from conftest import db5_complex, db5_ids
    from test_gpu_sterics import ca_center, db5_poses
    from dfmdock_amd import hbonds as HB
    rng = np.random.default_rng(0)
    runs = []
    for cid in db5_ids():
        c = db5_complex(cid)
        rot, tr = db5_poses(rng)
        rec, lig, cen = backbone_polar(c["rec_pos"], c["rec_seq"]), backbone_polar(c["lig_pos"], c["lig_seq"]), ca_center(c["lig_pos"])
        runs.append((cid, rec, lig, cen, rot, tr, HB.hbonds(rec, lig, cen, rot, tr, per_atom=True)))
    return runs


def test_db5_recipe():
    """What the definition gives on the 24 DB5 backbones: 384 poses, 1 593 role-compatible pairs below 3.5 A, 549 hydrogen bonds, 175
    poses without one, 48 bonds over the 24 identity poses (2SIC and 2SNI: 9 each), and no pair within 1e-4 A of the cutoff or within
    1e-6 of cos = 0 - so the device has no pair to round the other way."""
    from dfmdock_amd import sterics as ST
    runs = db5_definition()
    poses_, pairs, near_cut, near_cos = 0, 0, 0, 0
    for cid, rec, lig, cen, rot, tr, o in runs:
        Y, YA = rec["xyz"].astype(np.float64), rec["ante"].astype(np.float64)
        for p in range(len(rot)):
            X, XA = ST.pose_atoms(lig["xyz"], cen, rot[p], tr[p]), ST.pose_atoms(lig["ante"], cen, rot[p], tr[p])
            a, b, d = ST.near_pairs(rec["xyz"], X, 3.6)
            ok = (lig["role"][a] ^ rec["role"][b]) == (D | A)
            a, b, d = a[ok], b[ok], d[ok]
            pairs += int((d < 3.5).sum())
            near_cut += int((np.abs(d - 3.5) < 1e-4).sum())
            dv = (Y[b] - X[a]) / d[:, None]
            u, w = XA[a] - X[a], YA[b] - Y[b]
            cx = (u * dv).sum(1) / np.linalg.norm(u, axis=1)
            cy = -(w * dv).sum(1) / np.linalg.norm(w, axis=1)
            near_cos += int(((np.abs(cx) < 1e-6) | (np.abs(cy) < 1e-6))[d < 3.5].sum())
        poses_ += len(rot)
    n = np.concatenate([o["n_hbond"] for *_, o in runs])
    ident = {cid: int(o["n_hbond"][0]) for cid, *_, o in runs}
    print("poses", poses_, "pairs", pairs, "bonds", int(n.sum()), "poses without one", int((n == 0).sum()), "identity", ident)
    assert (poses_, pairs, int(n.sum()), int((n == 0).sum())) == (384, 1593, 549, 175)
    assert sum(ident.values()) == 48 and ident["2SIC"] == 9 and ident["2SNI"] == 9 and near_cut == 0 and near_cos == 0
    assert all(int(o["n_salt_atoms"].sum()) == 0 and np.array_equal(o["hb_kind"][:, 0], o["n_hbond"]) for *_, o in runs)


def test_unsatisfied_and_the_host_finishes(tmp_path):
    from dfmdock_amd import hbonds as HB
    role = np.uint8([D, A, D | A, CAT, D | SC, A | AN, D])
    exposed = np.int32([10, 10, 8, 10, 0, 3, 10])
    buried = np.int32([[10, 5, 8, 10, 0, 2, 10],       # pose 0
                       [9, 10, 4, 10, 0, 3, 10]])     # pose 1
    hb = np.int32([[0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0]])
    u = HB.unsatisfied(role, exposed, buried, hb)
    # fully buried without a bond: atom 0 (donor), atom 2 (both); atom 3 is no donor or acceptor, atom 4 has no exposed point, atom 6 has a bond
    assert u["mask"].tolist() == [[True, False, True, False, False, False, False], [False, True, False, False, False, True, True]]
    assert u["n_unsat"].tolist() == [2, 3] and u["n_unsat_donor"].tolist() == [1, 1] and u["n_unsat_acceptor"].tolist() == [0, 2]
    assert u["n_unsat_both"].tolist() == [1, 0] and u["n_unsat"].dtype == np.int32
    h = HB.unsatisfied(role, exposed, buried, hb, percent=50)      # buried * 100 >= 50 * exposed, in integers: 5 of 10 and 4 of 8 count, 2 of 3 does
    assert h["mask"].tolist() == [[True, True, True, False, False, True, False], [True, True, True, False, False, True, True]]
    assert HB.unsatisfied(role, exposed, buried, hb, percent=51)["mask"][0].tolist() == [True, False, True, False, False, True, False]
    for bad in (0, 101, 50.5):
        with pytest.raises(ValueError):
            HB.unsatisfied(role, exposed, buried, hb, percent=bad)
    with pytest.raises(ValueError):
        HB.unsatisfied(role, exposed[:-1], buried, hb)
    assert np.array_equal(HB.residue_bonds(np.int32([[1, 2, 0, 4], [0, 0, 1, 1]]), np.int32([2, 0, 2, 1]), 4), [[2, 4, 1, 0], [0, 1, 1, 0]])
    rk, lk = [("A", 7, " ", "ARG"), ("A", 8, "B", "GLY")], [("B", 1, " ", "ASP"), ("B", 2, " ", "SER"), ("B", 3, " ", "ALA")]
    HB.write_hbond_residues(tmp_path / "r.txt", rk, [2, 0], [4, 0], lk, [1, 1, 0], [4, 0, 0])
    assert (tmp_path / "r.txt").read_text().splitlines()[1:] == ["R A:7 ARG 2 4", "L B:1 ASP 1 4", "L B:2 SER 1 0"]


def test_every_value_error_of_the_checkers():
    from dfmdock_amd import hbonds as HB
    rng = np.random.default_rng(2)
    rec, lig = lump(rng, 30, 5), lump(rng, 20, 4)
    rot, tr = poses(rng, 2)
    assert HB.min_cos2(90) == 0.0 and HB.min_cos2(90.0) == 0.0 and HB.min_cos2(120) == np.cos(np.radians(120.0)) ** 2 and 0 < HB.min_cos2(179.9) < 1
    assert HB.check_cutoffs(3.5, 4.0) == (3.5, 4.0) and HB.check_cutoffs(3.3, 8)[0] == float(np.float32(3.3))
    for kw in ({"hb_cutoff": 0}, {"hb_cutoff": 8.5}, {"hb_cutoff": np.nan}, {"salt_cutoff": -1}, {"salt_cutoff": 8.01}, {"min_angle": 89.9},
               {"min_angle": 180}, {"min_angle": np.nan}):
        with pytest.raises(ValueError):
            HB.hbonds(rec, lig, Z3, rot, tr, **kw)

    def mod(c, key, i, v):
        q = dict(c, **{key: c[key].copy()})
        q[key][i] = v
        return q
    for bad in (mod(rec, "role", 3, 32), mod(rec, "role", 0, 255), mod(rec, "res", 2, 5), mod(rec, "res", 2, -1), mod(rec, "xyz", (1, 1), np.nan),
                mod(rec, "ante", (29, 2), np.inf), dict(rec, n_res=0), dict(rec, n_res=4097), dict(rec, ante=rec["ante"][:-1]),
                dict(rec, role=rec["role"][:-1]), dict(rec, xyz=rec["xyz"][:0], ante=rec["ante"][:0], role=rec["role"][:0], res=rec["res"][:0])):
        with pytest.raises(ValueError):
            HB.hbonds(bad, lig, Z3, rot, tr)
        with pytest.raises(ValueError):
            HB.hbonds(lig, bad, Z3, rot, tr)
    with pytest.raises(ValueError):
        HB.hbonds(rec, lig, Z3, rot, tr[:1])
    with pytest.raises(ValueError):
        HB.hbonds(rec, lig, Z3, np.zeros((65537, 3), np.float32), np.zeros((65537, 3), np.float32))


def test_struct_layout_and_exports(tmp_path):
    """dfm_hbond_out as gcc lays it out against the ctypes mirror; the new symbols are exported and listed; argument checks run before any
    device work and reach `status`."""
    from dfmdock_amd import _lib
    c_name, cls = "dfm_hbond_out", _lib.HbondOutC
    body = f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[c_name]) == C.sizeof(cls) == 64
    for f, _ in cls._fields_:
        assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_hbond_create", "dfm_hbond_destroy", "dfm_hbond_info", "dfm_pose_hbonds", "dfm_pose_hbonds_chunked", "dfm_hbond_last_timing",
              "dfm_hbond_last_phases"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and (getattr(lib, s).argtypes or s == "dfm_hbond_destroy")
    from test_abi_cpu import header_symbols
    assert sorted(_lib.EXPORTS) == header_symbols()
    status = C.c_int(7)
    none = [None] * 4
    assert lib.dfm_hbond_create(None, 1, *none, 1, 1, *none, 1, None, 3.5, 0.0, 4.0, C.byref(status)) is None
    assert status.value == -1 and b"m is NULL" in lib.dfm_last_error()
    assert lib.dfm_hbond_create(None, 1, *none, 1, 1, *none, 1, None, 3.5, 0.0, 4.0, None) is None      # status may be NULL
    assert lib.dfm_pose_hbonds(None, 1, None, None, None) == -1 and b"h is NULL" in lib.dfm_last_error()
    assert lib.dfm_hbond_last_timing(None, None) == -1 and lib.dfm_hbond_info(None, None, None, None, None, None, None) == -1
    assert lib.dfm_hbond_last_phases(None, None, None) == -1


def test_the_kernels_are_in_the_shipped_code_object():
    """The three kernels of kernels_hbond.hip are in the code object (so the scratch / LDS / op_sel audits of test_abi_cpu.py run over
    them), use no scratch, k_hbond holds its two staged float4 arrays in LDS, and the file is built without contraction."""
    import re
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(os.path.join(tools, "llvm-readelf")), "the ROCm llvm tools that built the library read its notes"
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_hbond.hip")).read()
    names = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))
    assert names == {"k_hbond_pose", "k_hbond", "k_hbond_finish"}
    mk = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "Makefile")).read()
    assert re.search(r"^kernels_hbond\.o:.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(STRICT\) ", mk, re.M) and "kernels_hbond.o" in re.search(r"^OBJS\s*:=.*", mk, re.M).group(0)
    td = tempfile.mkdtemp()
    try:
        lib = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, lib)
        subprocess.run([os.path.join(tools, "llvm-objdump"), "--offloading", lib], cwd=td, check=True, capture_output=True)
        found = {}
        for f in sorted(os.listdir(td)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", os.path.join(td, f)], capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                for n in names:
                    if re.search(r"\d+" + n + r"E", name):
                        found[n] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in ("private_segment_fixed_size", "group_segment_fixed_size"))
        assert found == {"k_hbond_pose": (0, 0), "k_hbond": (0, 2048), "k_hbond_finish": (0, 0)}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    d = tmp_path_factory.mktemp("hbond_prep")
    exe = str(d / "hbond_prep")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "hbond_prep_main.cpp"), "-o", exe])

    def run(rec, lig, center=(0, 0, 0), hb_cutoff=3.5, c2=0.0, salt_cutoff=4.0, budget=64 << 20, n_res=None):
        path = str(d / "in.bin")
        n = (rec["xyz"].shape[0], lig["xyz"].shape[0]) + (n_res or (rec["n_res"], lig["n_res"]))
        with open(path, "wb") as f:
            f.write(struct.pack("<iiii", *n) + np.float32([hb_cutoff, salt_cutoff]).tobytes() + struct.pack("<d", c2) + np.float32(center).tobytes()
                    + struct.pack("<q", budget))
            for c in (rec, lig):
                f.write(np.ascontiguousarray(c["xyz"], np.float32).tobytes() + np.ascontiguousarray(c["ante"], np.float32).tobytes()
                        + np.ascontiguousarray(c["role"], np.uint8).tobytes() + np.ascontiguousarray(c["res"], np.int32).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.stderr == "", r.stderr      # a sanitizer report
        return r.returncode, {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    return run


def test_host_preparation_under_the_sanitizers(prep):
    """The bits and the antecedents follow their atoms through both sorts, the charged residues are numbered in residue order, the chunk
    follows the bitmap, and every limit has its message."""
    i64 = lambda out, k: np.array([int(v) for v in out[k]], np.int64)
    f32 = lambda out, k: np.array([float(v) for v in out[k]], np.float32)
    rng = np.random.default_rng(8)
    for Nl, n_res in ((1, 1), (63, 31), (64, 32), (65, 33), (130, 65)):
        rec, lig = lump(rng, 150, n_res), lump(rng, Nl, max(1, Nl // 3), center=(3, 0, 0))
        rc, out = prep(rec, lig, lig["xyz"].mean(0), salt_cutoff=4.5)
        assert rc == 0 and float(out["edge"][0]) == 4.5, out
        order, index = i64(out, "order"), i64(out, "lig_index")
        assert np.array_equal(np.sort(order), np.arange(150)) and np.array_equal(np.sort(index), np.arange(Nl))
        assert np.array_equal(f32(out, "rec_x"), rec["xyz"][order, 0]) and np.array_equal(f32(out, "rec_ante_x"), rec["ante"][order, 0])
        assert np.array_equal(f32(out, "lig_ante_x"), lig["ante"][index, 0])
        for c, bits, comp, perm in ((rec, i64(out, "rec_bits"), i64(out, "rec_compact"), order), (lig, i64(out, "lig_bits"), i64(out, "lig_compact"), index)):
            charged = (c["role"] & (CAT | AN)) != 0
            which = np.unique(c["res"][charged])
            want = np.full(c["n_res"], -1)
            want[which] = np.arange(which.size)
            assert np.array_equal(comp, want)
            assert np.array_equal(bits & 31, c["role"][perm]) and np.array_equal((bits >> 8)[charged[perm]], want[c["res"][perm]][charged[perm]])
            assert not (bits >> 8)[~charged[perm]].any()
        Rc, Lc = (int(v) for v in out["charged"])
        assert (Rc, Lc) == ((i64(out, "rec_compact") >= 0).sum(), (i64(out, "lig_compact") >= 0).sum()) and int(out["words"][0]) == (Rc + 31) // 32
        assert [int(v) for v in out["chunk"]] == [min(32768, max(1, (64 << 20) // (max(Lc, 1) * max((Rc + 31) // 32, 1) * 4)))] * 2
    # a chain without a charged residue is legal
    rec, lig = lump(rng, 40, 6), lump(rng, 30, 5)
    lig["role"] &= np.uint8(D | A | SC)
    lig["role"][lig["role"] == 0] = D
    rc, out = prep(rec, lig)
    assert rc == 0 and int(out["charged"][1]) == 0 and set(out["lig_compact"]) == {"-1"} and [int(v) for v in out["chunk"]][0] == 32768
    # the budget: 4096 x 4096 charged residues are 2 MiB of bitmap per pose
    big = lump(rng, 4096, 4096)
    big["res"], big["role"] = np.arange(4096, dtype=np.int32), np.full(4096, CAT | AN, np.uint8)
    for budget, want in ((64 << 20, 32), (2 << 20, 1), (1, 1), ((2 << 20) * 5 + 7, 5)):
        rc, out = prep(big, big, budget=budget)
        assert rc == 0 and [int(v) for v in out["chunk"]] == [32, want] and out["charged"] == ["4096", "4096"]
    # the limits, in the creator's order
    err = lambda *a, **k: " ".join(prep(*a, **k)[1].get("error", ["<none>"]))

    def mod(c, key, i, v):
        q = dict(c, **{key: c[key].copy()})
        q[key][i] = v
        return q
    rec, lig = lump(rng, 30, 14), lump(rng, 45, 9)
    assert err(mod(rec, "xyz", (3, 1), np.nan), lig) == "rec_atoms: atom 3 is not finite"
    assert err(rec, lig, n_res=(0, 9)) == "rec: need 1 <= residues <= 4096" and err(rec, lig, n_res=(4097, 9)) == "rec: need 1 <= residues <= 4096"
    assert err(rec, lig, n_res=(14, 4097)) == "lig: need 1 <= residues <= 4096"
    assert err(mod(rec, "ante", (7, 2), np.inf), lig) == "rec_ante: atom 7 is not finite"
    assert err(mod(rec, "role", 5, 32), lig) == "rec_role: atom 5 has role 32 outside the five bits"
    assert err(rec, mod(lig, "role", 44, 255)) == "lig_role: atom 44 has role 255 outside the five bits"
    assert err(mod(rec, "res", 5, 14), lig) == "rec_res: atom 5 has residue 14 outside [0, 14)"
    assert err(rec, mod(lig, "res", 0, -1)) == "lig_res: atom 0 has residue -1 outside [0, 9)"
    for cut in (0.0, 8.5, np.nan, -3.0):
        assert err(rec, lig, hb_cutoff=cut) == "hb_cutoff must be in (0, 8]" and err(rec, lig, salt_cutoff=cut) == "salt_cutoff must be in (0, 8]"
    for c2 in (-0.1, 1.0, np.nan):
        assert err(rec, lig, c2=c2).startswith("min_cos2 must be in [0, 1)")
    assert prep(rec, lig, hb_cutoff=8.0, salt_cutoff=8.0, c2=0.999)[0] == 0


def _pair(tmp_path):
    from dfmdock_amd import cli
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    return cli.load_pair(rec_pdb, lig_pdb, feat)[:2], (rec_pdb, lig_pdb, feat)


def test_driver_inputs_and_the_shared_finish(tmp_path, monkeypatch):
    """hbond_inputs on the written backbone files, and _finish with the engine stubbed: the five counts describe the kept pose, hbond_data
    holds every trajectory, every model gains the counts, n_unsat comes with the surface only, and without the option nothing is added."""
    from dfmdock_amd import driver, hbonds as HB
    (rec, lig), _ = _pair(tmp_path)
    rp, lp, cen = driver.hbond_inputs(rec, lig, 0)
    assert np.array_equal(cen, driver.sterics_inputs(rec, lig, 0)[2]) and rp["untyped"] == lp["untyped"] == 0
    n_pro = sum(k[3] == "PRO" for k in rp["keys"])
    assert len(rp["role"]) == 2 * rp["n_res"] - n_pro and not (rp["role"] & SC).any() and (rp["role"][rp["role"] & CAT > 0] == D | CAT).sum() <= 1
    HB.check_chain(rp, "rec"), HB.check_chain(lp, "lig")
    assert driver._check_hbonds(False, 3.5, 90, 4.0) is None and driver._check_hbonds(True, 3.25, 100, 5) == (3.25, 100.0, 5.0)
    for bad in ((9.0, 90, 4.0), (3.5, 80, 4.0), (3.5, 90, 0.0)):
        with pytest.raises(ValueError):
            driver._check_hbonds(True, *bad)
    n = 5
    energy = np.float32([-1.0, -5.0, -2.0, -3.0, -4.0])
    cols = {"energy": energy, "rot_update": 0.01 * np.arange(3 * n, dtype=np.float32).reshape(n, 3), "tr_update": np.arange(3 * n, dtype=np.float32).reshape(n, 3)}
    kind = np.arange(3 * n).reshape(n, 3)
    seen, calls = {}, []

    def ensemble_hbonds(model, rec_, lig_, rot, tr, hb_cutoff, min_angle, salt_cutoff, per_atom=False):
        seen["args"] = (np.asarray(rot).shape, hb_cutoff, min_angle, salt_cutoff, per_atom)
        hd = {"n_hbond": kind.sum(1), "hb_kind": kind, "n_salt": np.arange(n) + 2, "n_salt_atoms": np.arange(n) + 3, "untyped": (0, 0),
              "rec_polar": {"role": np.uint8([D, A]), "index": np.array([0, 3])}, "lig_polar": {"role": np.uint8([D | A]), "index": np.array([1])}}
        if per_atom:
            hd.update(rec_hb=np.zeros((n, 2), np.int32), lig_hb=(np.arange(n)[:, None] % 2).astype(np.int32))
        return hd

    def ensemble_surface(model, rec_, lig_, rot, tr, probe, points, per_atom=False):
        calls.append(per_atom)
        bd = {"bsa": np.arange(n) * 100.0, "bsa_rec": np.arange(n) * 50.0, "bsa_lig": np.arange(n) * 50.0, "probe": probe, "sphere_points": points}
        if per_atom:
            bd.update(rec_exposed=np.int32([4, 0, 0, 6]), lig_exposed=np.int32([0, 5]), rec_buried=np.int32([[4, 0, 0, 5]] * n),
                      lig_buried=np.int32([[0, 5]] * n))
        return bd
    monkeypatch.setattr(driver, "ensemble_hbonds", ensemble_hbonds)
    monkeypatch.setattr(driver, "ensemble_surface", ensemble_surface)
    monkeypatch.setattr(driver, "cluster_trajectories", lambda *a, **k: {"center": np.array([1, 3]), "size": np.array([3, 2]), "cluster_of": np.array([1, 0, 0, 1, 0])})

    class Gx:
        lig_pos0 = np.asarray(lig["bb_coords"], np.float32)

        def close(self):
            pass
    model = type("M", (), {"hp": type("Hp", (), {"family": 0})})()
    def fin(clu=None, **opts):
        run = driver._Run(model, Gx(), rec, lig, cols, "fp32", opts)
        run.key = energy
        return driver._finish(run, (np.argmin, "energy"), lambda k: {}, clu)
    r = fin()
    assert not any(k in r for k in ("n_hbond", "hbond_data", "index", "n_salt")) and "args" not in seen
    r = fin(hbonds=driver._check_hbonds(True, 3.5, 90.0, 4.0), clu=(2, 4.0, "energy"))
    want = lambda k: {"n_hbond": int(kind[k].sum()), "hb_bb_bb": int(kind[k, 0]), "hb_bb_sc": int(kind[k, 1]), "hb_sc_sc": int(kind[k, 2]), "n_salt": k + 2}
    assert seen["args"] == ((n, 3), 3.5, 90.0, 4.0, False) and r["index"] == 1 and {k: r[k] for k in want(1)} == want(1) and "n_unsat" not in r
    assert set(r["trajectories"]) == {"energy", "rot_update", "tr_update"} and r["hbond_data"]["n_salt_atoms"].tolist() == list(range(3, 3 + n))
    assert [m["index"] for m in r["models"]] == [1, 3] and all({k: m[k] for k in want(0)} == want(m["index"]) for m in r["models"])
    json.dumps({k: r[k] for k in want(1)})
    # with the surface in the same run: one per-atom surface call, and n_unsat = receptor atom 0 (fully buried, no bond) plus the ligand's
    # atom in the poses where it has no bond; the receptor's acceptor buries 5 of 6 points only
    r = fin(hbonds=driver._check_hbonds(True, 3.5, 90.0, 4.0), surface=driver._check_surface(True, None, 1.4, 128), clu=(2, 4.0, "energy"))
    assert calls == [True] and seen["args"][4] is True and r["hbond_data"]["n_unsat"].tolist() == [2, 1, 2, 1, 2] and r["n_unsat"] == 1 and r["bsa"] == 100.0
    assert [m["n_unsat"] for m in r["models"]] == [1, 1]


def test_cli_flags_parse_default_off_and_reach_the_driver(tmp_path, monkeypatch, capsys):
    from dfmdock_amd import cli, driver
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert not a.hbonds and a.hbond_residues is None and cli.hbonds_kwargs(a) == {}
        assert cli.hbonds_kwargs(cli.parse_args([cmd] + base + ["--hbonds"])) == dict(hbonds=True, hbond_cutoff=3.5, hbond_angle=90.0, salt_cutoff=4.0)
        assert cli.hbonds_kwargs(cli.parse_args([cmd] + base + ["--hbonds", "--hbond-cutoff", "3.2", "--hbond-angle", "110", "--salt-cutoff", "4.5"])) == \
            dict(hbonds=True, hbond_cutoff=3.2, hbond_angle=110.0, salt_cutoff=4.5)
        assert cli.parse_args([cmd] + base + ["--hbond-residues", "x.txt"]).hbonds
        for bad in (["--hbond-cutoff", "3"], ["--salt-cutoff", "4"], ["--hbond-angle", "100"], ["--hbonds", "--hbond-cutoff", "9"],
                    ["--hbonds", "--hbond-cutoff", "nan"], ["--hbonds", "--salt-cutoff", "0"], ["--hbonds", "--hbond-angle", "89"],
                    ["--hbonds", "--hbond-angle", "180"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c", "--hbonds"])
    (rec, lig), (rec_pdb, lig_pdb, feat) = _pair(tmp_path)
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))
    counts = {"n_hbond": 7, "hb_bb_bb": 3, "hb_bb_sc": 2, "hb_sc_sc": 2, "n_salt": 1}
    poses_ = {"rot_update": np.float32([[0, 0, 0], [0.1, 0, 0], [0, 0.2, 0]]), "tr_update": np.float32([[1, 1, 1], [2, 2, 2], [3, 3, 3]])}

    def pair(model, rec, lig, rec_x, lig_x, **kw):
        seen.update(kw)
        res = {"energy": -1.5, "precision": "mfma16", "rot_update": poses_["rot_update"][0], "tr_update": poses_["tr_update"][0], "selfcheck": None,
               "t_begin": 0.1, "index": 0, "trajectories": {"energy": np.zeros(1)}}
        if kw.get("hbonds"):
            res.update(counts, index=4, hbond_data=dict(poses_, untyped=(0, 3) if kw["salt_cutoff"] == 5.0 else (0, 0)))
            if kw.get("bsa"):
                res.update(n_unsat=5, bsa=1.0, bsa_rec=0.5, bsa_lig=0.5, probe=1.4, sphere_points=128)
            if kw.get("top_k"):
                res.update(models=[dict(counts, rank=1, index=2, energy=-1.0, cluster_size=2)])
        return res
    rk, lk = driver.hbond_inputs(rec, lig, 0)[0]["keys"], driver.hbond_inputs(rec, lig, 0)[1]["keys"]

    def residue_hbonds(model, rec, lig, rot, tr, hb_cutoff, min_angle, salt_cutoff):
        seen.setdefault("residue_calls", []).append((np.asarray(rot).tolist(), np.asarray(tr).tolist(), hb_cutoff, min_angle, salt_cutoff))
        hb = [np.zeros(len(rk), np.int64), np.zeros(len(lk), np.int64)]
        hb[0][3], hb[1][0] = 2, 2
        return (rk, lk), hb, [np.zeros(len(rk), np.int64), np.zeros(len(lk), np.int64)]
    monkeypatch.setattr(driver, "dock_pair", pair)
    monkeypatch.setattr(driver, "refine_pair", pair)
    monkeypatch.setattr(driver, "residue_hbonds", residue_hbonds)
    for cmd in ("dock", "refine"):
        args = [cmd, rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb")]
        seen.clear()
        assert cli.main(args) == 0
        plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert not any(k in plain for k in counts) and not any(k.startswith(("hbond", "salt")) for k in seen)
        assert cli.main(args + ["--hbonds"]) == 0
        io = capsys.readouterr()
        line = json.loads(io.out.strip().splitlines()[-1])
        assert {k: line[k] for k in counts} == counts and line["index"] == 4 and "n_unsat" not in line and "hbond_untyped" not in line and io.err == ""
        assert {k: v for k, v in line.items() if k in plain and k != "index"} == {k: v for k, v in plain.items() if k != "index"}
        assert (seen["hbonds"], seen["hbond_cutoff"], seen["hbond_angle"], seen["salt_cutoff"]) == (True, 3.5, 90.0, 4.0)
        # with --bsa: n_unsat; untyped atoms are said once on stderr; --hbond-residues writes the kept model's table
        out_txt = tmp_path / f"{cmd}_res.txt"
        assert cli.main(args + ["--hbond-residues", str(out_txt), "--bsa", "--salt-cutoff", "5"]) == 0
        io = capsys.readouterr()
        line = json.loads(io.out.strip().splitlines()[-1])
        assert line["n_unsat"] == 5 and line["hbond_untyped"] == [0, 3] and io.err.count("polar atoms have no antecedent") == 1
        assert seen["residue_calls"] == [([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 3.5, 90.0, 5.0)] and os.path.samefile(line["hbond_residues"], out_txt)
        fmt = lambda side, k: f"{side} {k[0]}:{k[1]} {k[3]} 2 0"
        assert out_txt.read_text().splitlines()[1:] == [fmt("R", rk[3]), fmt("L", lk[0])]
    # dock --top-k: every model's table next to the kept one's
    seen.clear()
    out_txt = tmp_path / "top.txt"
    assert cli.main(["dock", rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb"), "--hbonds", "--top-k", "1",
                     "--hbond-residues", str(out_txt)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {k: line["models"][0][k] for k in counts} == counts and [c[1] for c in seen["residue_calls"]] == [[1.0, 1.0, 1.0], [3.0, 3.0, 3.0]]
    assert (tmp_path / "top_1.txt").read_text() == out_txt.read_text()
