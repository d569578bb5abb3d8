"""The float64 definition of the all-atom clash / contact screen (dfmdock_amd/sterics.py), its host finishes and the command-line
plumbing, on the CPU.  The GPU call is held against this definition in tests/test_gpu_sterics.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_pair
from conftest import ROOT

Z3 = np.zeros((1, 3), np.float32)


def one(rec, lig, center=(0, 0, 0), rot=Z3, tr=Z3, **kw):
    from dfmdock_amd import sterics as ST
    return ST.sterics(np.asarray(rec, np.float32), np.asarray(lig, np.float32), np.asarray(center, np.float32), rot, tr, per_atom=True, **kw)


def test_known_answers_around_the_cutoffs():
    # two ligand atoms at 2.999 and 3.001 A of one receptor atom: one clash, two contacts
    o = one([[0, 0, 0]], [[2.999, 0, 0], [0, 3.001, 0]])
    assert o["n_clash"].tolist() == [1] and o["n_contact"].tolist() == [2]
    assert o["lig_clash"].tolist() == [[1, 0]] and o["lig_contact"].tolist() == [[1, 1]]
    assert o["min_dist"][0] == float(np.float32(2.999)) and o["n_clash"].dtype == np.int32 and o["min_dist"].dtype == np.float64
    # exactly 3.0 is not a clash, exactly 5.0 not a contact (strict)
    o = one([[0, 0, 0]], [[3.0, 0, 0], [0, 0, 5.0]])
    assert o["n_clash"].tolist() == [0] and o["n_contact"].tolist() == [1] and o["min_dist"][0] == 3.0
    # nothing within the contact cutoff: +inf
    o = one([[0, 0, 0]], [[6.0, 0, 0]])
    assert o["n_contact"].tolist() == [0] and o["min_dist"][0] == np.inf
    # the identity transform about any centre
    o = one([[0, 0, 0]], [[2.5, 0, 0]], center=(7, -3, 2))
    assert o["n_clash"].tolist() == [1] and o["min_dist"][0] == 2.5
    # 90 degrees about z, about the off-origin centre (1, 1, 0): (2, 1, 0) -> (1, 2, 0); the receptor atom at (1, 4.5, 0) is 2.5 A away
    rot = np.array([[0, 0, np.pi / 2]], np.float32)
    o = one([[1, 4.5, 0]], [[2, 1, 0]], center=(1, 1, 0), rot=rot)
    assert o["n_clash"].tolist() == [1] and abs(o["min_dist"][0] - 2.5) < 1e-6
    assert one([[1, 4.5, 0]], [[2, 1, 0]], center=(1, 1, 0))["n_contact"].tolist() == [1]      # unrotated: sqrt(1 + 12.25) = 3.64
    # ... plus a translation
    o = one([[1, 4.5, 0]], [[2, 1, 0]], center=(1, 1, 0), rot=rot, tr=np.array([[0, 0, 4.0]], np.float32))
    assert o["n_clash"].tolist() == [0] and abs(o["min_dist"][0] - np.sqrt(2.5 ** 2 + 16)) < 1e-6
    # the small-angle branch (|rot| < 1e-6): a rotation by 5e-7 rad moves (1000, 0, 0) by 5e-4 A in y
    from dfmdock_amd import sterics as ST
    x = ST.pose_atoms(np.array([[1000.0, 0, 0]], np.float32), np.zeros(3), np.array([0, 0, 5e-7], np.float32), np.zeros(3))
    assert abs(x[0, 1] - 5e-4) < 1e-9 and abs(x[0, 0] - 1000.0) < 1e-6
    o = one([[1000.0, 2.9999, 0]], [[1000.0, 0, 0]], rot=np.array([[0, 0, 5e-7]], np.float32))
    assert o["n_clash"].tolist() == [1] and abs(o["min_dist"][0] - (float(np.float32(2.9999)) - 5e-4)) < 1e-6
    # cutoffs: contact == clash is allowed, contact < clash is not
    o = one([[0, 0, 0]], [[2.0, 0, 0], [3.5, 0, 0]], clash_cutoff=3.0, contact_cutoff=3.0)
    assert o["n_clash"].tolist() == o["n_contact"].tolist() == [1]
    for bad in (dict(clash_cutoff=5.0, contact_cutoff=3.0), dict(clash_cutoff=0.0), dict(contact_cutoff=float("nan"))):
        with pytest.raises(ValueError):
            one([[0, 0, 0]], [[1, 0, 0]], **bad)


def test_nan_poses_disturb_no_other_pose():
    rng = np.random.default_rng(0)
    rec, lig = (4.0 * rng.random((20, 3))).astype(np.float32), (4.0 * rng.random((15, 3))).astype(np.float32)
    rot, tr = (0.3 * rng.standard_normal((5, 3))).astype(np.float32), rng.standard_normal((5, 3)).astype(np.float32)
    clean = one(rec, lig, lig.mean(0), rot, tr)
    assert (clean["n_contact"] > 0).all()
    r2, t2 = rot.copy(), tr.copy()
    r2[1, 0], t2[3, 2] = np.nan, np.nan
    dirty = one(rec, lig, lig.mean(0), r2, t2)
    for p in (1, 3):
        assert dirty["n_clash"][p] == 0 and dirty["n_contact"][p] == 0 and dirty["min_dist"][p] == np.inf and not dirty["lig_contact"][p].any()
    for p in (0, 2, 4):
        for k in clean:
            assert np.array_equal(clean[k][p], dirty[k][p]), (k, p)


def test_definition_equals_a_triple_loop_on_a_toy():
    from dfmdock_amd import pdbio
    rng = np.random.default_rng(1)
    rec, lig = (5.0 * rng.random((7, 3))).astype(np.float32), (5.0 * rng.random((5, 3))).astype(np.float32)
    cen = lig.astype(np.float64).mean(0).astype(np.float32)
    rot, tr = (0.8 * rng.standard_normal((6, 3))).astype(np.float32), (2.0 * rng.standard_normal((6, 3))).astype(np.float32)
    o = one(rec, lig, cen, rot, tr)
    seen = 0
    for p in range(6):
        R = pdbio.axis_angle_to_matrix(rot[p])
        nc = nt = 0
        best = np.inf
        for a in range(5):
            x = R @ (lig[a].astype(np.float64) - cen.astype(np.float64)) + cen.astype(np.float64) + tr[p].astype(np.float64)
            ac = at = 0
            for b in range(7):
                dx, dy, dz = x - rec[b].astype(np.float64)
                d = np.sqrt((dx * dx + dy * dy) + dz * dz)
                assert abs(d - 3.0) > 1e-6 and abs(d - 5.0) > 1e-6      # no pair near enough to a cutoff for the matmul's rounding to matter
                ac, at = ac + (d < 3.0), at + (d < 5.0)
                best = min(best, d) if d < 5.0 else best
            assert o["lig_clash"][p, a] == ac and o["lig_contact"][p, a] == at
            nc, nt = nc + ac, nt + at
        assert o["n_clash"][p] == nc and o["n_contact"][p] == nt and abs(o["min_dist"][p] - best) < 1e-12
        seen += nt
    assert seen > 20


def test_the_bounding_box_shortcut_changes_nothing(monkeypatch):
    """near_pairs drops atoms beyond reach + 1 A of the other chain's box before taking distances, and works in blocks of pairs."""
    from dfmdock_amd import sterics as ST
    rng = np.random.default_rng(2)
    rec, lig = (30.0 * rng.random((400, 3))).astype(np.float32), (30.0 * rng.random((300, 3)) + 12.0).astype(np.float32)
    a, b, d = ST.near_pairs(rec, lig.astype(np.float64), 5.0)
    full = np.sqrt(((lig[:, None].astype(np.float64) - rec[None].astype(np.float64)) ** 2).sum(-1))
    wa, wb = np.nonzero(full < 5.0)
    assert len(a) > 50 and np.array_equal(a, wa) and np.array_equal(b, wb) and np.allclose(d, full[wa, wb], rtol=0, atol=1e-12)
    monkeypatch.setattr(ST, "_PAIR_BUDGET", 1000)
    a2, b2, d2 = ST.near_pairs(rec, lig.astype(np.float64), 5.0)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(d, d2)


def test_capri_flags():
    from dfmdock_amd import sterics as ST
    n = np.array([0, 1, 2, 1, 0, 40, 1, 2], np.int32)
    flags, thr, mean, std = ST.capri_flags(n)
    assert mean == n.mean() and std == n.std() and thr == n.mean() + 2 * n.std()      # population std, ddof 0
    assert flags.tolist() == [False] * 5 + [True, False, False] and flags.dtype == bool
    # exactly at the threshold is not flagged: counts 0, 0, 0, 0, 4 -> mean 0.8, std 1.6, thr 4.0
    flags, thr, _, _ = ST.capri_flags([0, 0, 0, 0, 4])
    assert thr == 0.8 + 2 * 1.6 and not flags.any()
    # the member mask: mean and std over the members, every pose judged
    m = np.array([1, 1, 1, 1, 1, 0, 1, 1], bool)
    flags, thr, mean, std = ST.capri_flags(n, m)
    assert mean == n[m].mean() and std == n[m].std() and flags.tolist() == [False] * 5 + [True, False, False] and thr < 3
    # fewer than two members: nothing flagged
    for mem in (np.zeros(8, bool), np.arange(8) == 5):
        flags, thr, mean, std = ST.capri_flags(n, mem)
        assert not flags.any() and thr == np.inf
    assert not ST.capri_flags([100])[0].any()
    with pytest.raises(ValueError):
        ST.capri_flags(n, np.ones(3, bool))


PDB = """\
ATOM      1  N   ALA A   1       0.000   0.000   0.000  1.00  0.00           N
ATOM      2  CA  ALA A   1       1.458   0.000   0.000  1.00  0.00           C
ATOM      3  H   ALA A   1      -0.500   0.800   0.000  1.00  0.00           H
ATOM      4  C   ALA A   1       2.000   1.400   0.000  1.00  0.00
ATOM      5 1HB  ALA A   1       1.800  -0.500   0.900  1.00  0.00
ATOM      6  HB2 ALA A   1       1.800  -0.500  -0.900  1.00  0.00
ATOM      7  CB  ALA A   1       1.900  -0.800   0.000  1.00  0.00
ATOM      8  D1  ALA A   1       3.000   3.000   3.000  1.00  0.00           D
HETATM    9  O   HOH A   2       5.000   5.000   5.000  1.00  0.00           O
ATOM     10  N   GLY A   2       3.300   1.500   0.000  1.00  0.00           N
ATOM     11  CA  GLY A   2       3.900   2.800   0.000  1.00  0.00           C
ATOM     12  C   GLY A   2       5.400   2.700   0.000  1.00  0.00           C
ATOM     13  HG  GLY A   2       5.400   2.700   1.000  1.00  0.00          HG
END
"""


def test_heavy_atoms_and_residues(tmp_path):
    from dfmdock_amd import pdbio
    from dfmdock_amd import sterics as ST
    path = tmp_path / "x.pdb"
    path.write_text(PDB)
    atoms = pdbio.read_pdb(str(path))
    assert len(atoms) == 13
    idx = ST.heavy_atoms(atoms)
    # H by element, H by name with an empty element column (1HB, HB2), D, HETATM are out; mercury (element HG) is a heavy atom
    assert [atoms[i]["name"] for i in idx] == ["N", "CA", "C", "CB", "N", "CA", "C", "HG"]
    keys, res = ST.residue_of_atoms(atoms, idx)
    assert keys == [("A", 1, " ", "ALA"), ("A", 2, " ", "GLY")] and res.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert ST.residue_counts(np.array([1, 0, 2, 0, 0, 5, 0, 1]), res, 2).tolist() == [3, 6]
    assert ST.residue_counts(np.arange(16).reshape(2, 8), res, 2).tolist() == [[6, 22], [38, 54]]
    # heavy_atoms indexes the chain dict the drivers hold (HETATM already dropped there)
    chain = pdbio.backbone_from_atoms(atoms)
    assert [chain["atoms"][i]["name"] for i in ST.heavy_atoms(chain["atoms"])] == ["N", "CA", "C", "CB", "N", "CA", "C", "HG"]
    out = tmp_path / "res.txt"
    ST.write_clash_residues(str(out), keys, [3, 0], [6, 0])
    assert out.read_text().splitlines()[1:] == ["A:1 ALA 3 6"]


def test_the_pose_is_apply_pose_all_atom_bit_for_bit():
    from dfmdock_amd import pdbio
    from dfmdock_amd import sterics as ST
    rng = np.random.default_rng(3)
    aa = (20.0 * rng.random((57, 3))).round(3)
    bb = (20.0 * rng.random((11, 3, 3))).round(3)
    for rot, tr in ((np.array([0.3, -0.8, 0.5], np.float32), np.array([4.0, -2.5, 9.25], np.float32)),
                    (np.array([2e-7, 0, -3e-7], np.float32), np.zeros(3, np.float32)), (np.zeros(3, np.float32), np.ones(3, np.float32))):
        want = pdbio.apply_pose_all_atom(aa, bb, rot, tr, center="ca")
        assert ST.pose_atoms(aa, bb[:, 1].mean(axis=0), rot, tr).tobytes() == want.tobytes()
        want = pdbio.apply_pose_all_atom(aa, bb, rot, tr, center="all_atoms")
        assert ST.pose_atoms(aa, aa.mean(axis=0), rot, tr).tobytes() == want.tobytes()


def test_driver_inputs_and_selection_helpers(tmp_path):
    from dfmdock_amd import cli, driver
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, _, _ = cli.load_pair(rec_pdb, lig_pdb, feat)
    ra, la, cen = driver.sterics_inputs(rec, lig, 0)
    assert ra.dtype == la.dtype == cen.dtype == np.float32 and ra.shape == (len(rec["atoms"]), 3) and la.shape == (len(lig["atoms"]), 3)
    assert np.array_equal(cen, np.asarray(lig["bb_coords"], np.float64)[:, 1].mean(0).astype(np.float32))
    assert np.array_equal(driver.sterics_inputs(rec, lig, 1)[2], np.asarray(lig["aa_coords"], np.float64).mean(0).astype(np.float32))
    e = np.array([3.0, -1.0, 0.5, -4.0, 2.0])
    bad = np.array([0, 0, 0, 1, 0], bool)
    assert driver._kept(np.argmin, None, e) == 3 and driver._kept(np.argmin, bad, e) == 1
    key = driver._nan_key(e, bad)
    assert np.isnan(key[3]) and np.array_equal(key[~bad], e[~bad]) and driver._nan_key(e, None) is e and driver._nan_key(None, bad) is None
    assert driver._check_sterics(False, False, 3.0, 5.0) is None and driver._check_sterics(False, True, 3.0, 5.0) == (True, 3.0, 5.0)
    with pytest.raises(ValueError):
        driver._check_sterics(True, False, 6.0, 5.0)
    sd = {"n_clash": np.array([2, 90]), "n_contact": np.array([30, 400]), "min_dist": np.array([2.5, np.inf]), "flags": np.array([False, True]),
          "threshold": 80.0, "ensemble_mean": 46.0, "ensemble_std": 44.0, "clash_cutoff": 3.0, "contact_cutoff": 5.0, "filtered": True, "fallback": False}
    r = driver._sterics_result(sd, 0)
    assert r["index"] == 0 and r["sterics"] == {"n_clash": 2, "n_contact": 30, "min_dist": 2.5, "flagged": False, "threshold": 80.0, "ensemble_mean": 46.0,
                                                 "ensemble_std": 44.0, "clash_cutoff": 3.0, "contact_cutoff": 5.0, "filtered": True, "fallback": False}
    assert driver._pose_sterics(sd, 1) == {"n_clash": 90, "n_contact": 400, "min_dist": None, "flagged": True}
    json.dumps(r["sterics"])
    assert driver._remarks(sd, 1) == ["dfmdock_amd sterics n_clash 90 n_contact 400 (heavy-atom pairs below 3 / 5 A)"] and driver._remarks(None, 0) is None
    assert driver._sterics_result(None, 0) == {}


def test_cli_flags_parse_default_off_and_reach_the_driver(tmp_path, monkeypatch, capsys):
    from dfmdock_amd import cli, driver, pdbio
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert not a.clash_screen and not a.clash_filter and a.clash_residues is None and cli.sterics_kwargs(a) == {}
        a = cli.parse_args([cmd] + base + ["--clash-screen"])
        assert cli.sterics_kwargs(a) == dict(clash_screen=True, clash_filter=False, clash_cutoff=3.0, contact_cutoff=5.0)
        a = cli.parse_args([cmd] + base + ["--clash-filter", "--clash-cutoff", "2.5", "--contact-cutoff", "4"])
        assert cli.sterics_kwargs(a) == dict(clash_screen=True, clash_filter=True, clash_cutoff=2.5, contact_cutoff=4.0)
        assert cli.parse_args([cmd] + base + ["--clash-residues", "x.txt"]).clash_screen
        for bad in (["--clash-cutoff", "2.5"], ["--clash-screen", "--clash-cutoff", "6"], ["--clash-screen", "--contact-cutoff", "nan"],
                    ["--clash-screen", "--clash-cutoff", "0"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c", "--clash-screen"])      # sweep is left alone: the DB5 files hold backbones only
    # cmd_pair (dock) with the engine stubbed: what reaches dock_pair, what the line and the residue file hold
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))
    st = {"n_clash": 3, "n_contact": 41, "min_dist": 2.25, "flagged": False, "threshold": 9.5, "ensemble_mean": 3.5, "ensemble_std": 3.0,
          "clash_cutoff": 3.0, "contact_cutoff": 5.0, "filtered": True, "fallback": False}

    def dock_pair(model, rec, lig, rec_x, lig_x, **kw):
        seen.update(kw)
        res = {"energy": -1.5, "precision": "mfma16", "rot_update": np.zeros(3, np.float32), "tr_update": np.ones(3, np.float32), "selfcheck": None}
        if kw.get("clash_screen"):
            res.update(sterics=st, index=4)
        return res

    def residue_sterics(model, rec, lig, rot, tr, cc, ct):
        seen["residue_call"] = (np.asarray(rot).tolist(), np.asarray(tr).tolist(), cc, ct)
        keys = [tuple(k) for k in lig["residues"]]
        n = np.zeros(len(keys), np.int64)
        n[2] = 7
        return keys, n // 7 * 3, n
    monkeypatch.setattr(driver, "dock_pair", dock_pair)
    monkeypatch.setattr(driver, "residue_sterics", residue_sterics)
    args = ["dock", rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb")]
    assert cli.main(args) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "sterics" not in plain and "index" not in plain and not any(k.startswith(("clash", "contact")) for k in seen)
    seen.clear()
    assert cli.main(args + ["--clash-filter", "--clash-residues", str(tmp_path / "res.txt")]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["clash_screen"] is True and seen["clash_filter"] is True and (seen["clash_cutoff"], seen["contact_cutoff"]) == (3.0, 5.0)
    assert line["sterics"] == st and line["index"] == 4 and {k: v for k, v in line.items() if k in plain} == plain
    assert seen["residue_call"] == ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 3.0, 5.0) and os.path.samefile(line["clash_residues"], tmp_path / "res.txt")
    k = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))["residues"][2]
    assert (tmp_path / "res.txt").read_text().splitlines()[1:] == [f"{k[0]}:{k[1]} {k[3]} 3 7"]


def test_remarks_are_optional_and_ignored_by_the_reader(tmp_path):
    from dfmdock_amd import pdbio
    atoms = pdbio.read_pdb(_write(tmp_path / "x.pdb", PDB))
    rec, lig = atoms[:4], atoms[4:8]
    xyz = np.array([a["coord"] for a in lig])
    pdbio.write_complex_pdb(str(tmp_path / "a.pdb"), rec, lig, xyz)
    pdbio.write_complex_pdb(str(tmp_path / "b.pdb"), rec, lig, xyz, remarks=["dfmdock_amd sterics n_clash 1 n_contact 2"])
    a, b = (tmp_path / "a.pdb").read_text(), (tmp_path / "b.pdb").read_text()
    assert b == "REMARK dfmdock_amd sterics n_clash 1 n_contact 2\n" + a and pdbio.read_pdb(str(tmp_path / "b.pdb")) == pdbio.read_pdb(str(tmp_path / "a.pdb"))


def _write(path, text):
    path.write_text(text)
    return str(path)


def test_struct_layout_and_exports(tmp_path):
    """dfm_sterics_params / dfm_sterics_out as gcc lays them out against the ctypes mirrors; the new symbols are exported and listed."""
    from dfmdock_amd import _lib
    body = ""
    for c_name, cls in (("dfm_sterics_params", _lib.StericsParamsC), ("dfm_sterics_out", _lib.StericsOutC)):
        body += f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(
            f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    for c_name, cls in (("dfm_sterics_params", _lib.StericsParamsC), ("dfm_sterics_out", _lib.StericsOutC)):
        assert int(got[c_name]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_atoms_create", "dfm_atoms_destroy", "dfm_atoms_info", "dfm_pose_sterics", "dfm_pose_sterics_chunked", "dfm_sterics_last_timing",
              "dfm_sterics_exit_counts"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    from test_abi_cpu import header_symbols
    assert sorted(_lib.EXPORTS) == header_symbols()
    # argument checks run before any device work
    assert lib.dfm_atoms_create(None, 1, None, 1, None, None, None) is None and b"m is NULL" in lib.dfm_last_error()
    assert lib.dfm_pose_sterics(None, 1, None, None, None) == -1 and lib.dfm_sterics_last_timing(None, None) == -1


def test_the_audits_see_the_new_kernels():
    """Both kernels of kernels_sterics.hip are in the shipped code object (so the scratch / LDS / op_sel audits of test_abi_cpu.py run over
    them) and use no scratch."""
    import re
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_sterics.hip")).read()
    names = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))
    assert names == {"k_sterics_pose", "k_sterics"}
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
            for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", notes, re.S):
                for n in names:
                    if re.search(r"\d+" + n + r"E", m.group(1)):
                        found[n] = int(m.group(2))
        assert found == {n: 0 for n in names}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)
