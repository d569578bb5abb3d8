"""CPU side of the buried-surface-area call: the float64 definition dfmdock_amd/surface.py on known answers, its host finishes, the
ctypes layouts and the command-line plumbing with the engine stubbed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_pair
from conftest import ROOT, db5_complex, db5_ids

Z3 = np.zeros((1, 3), np.float32)


def one(rec, rr, lig, lr, K=128, **kw):
    from dfmdock_amd import surface as SF
    return SF.bsa(np.asarray(rec, np.float32), np.asarray(rr, np.float32), np.asarray(lig, np.float32), np.asarray(lr, np.float32),
                  np.zeros(3, np.float32), Z3, Z3, K=K, **kw)


def test_sphere_points():
    from dfmdock_amd import surface as SF
    for K in (64, 128, 192, 256):
        u = SF.sphere_points(K)
        assert u.shape == (K, 3) and u.dtype == np.float32
        assert np.abs(np.sqrt((u.astype(np.float64) ** 2).sum(1)) - 1.0).max() < 2e-7      # float32 rounding of three components
        k = np.arange(K)
        assert np.array_equal(u[:, 2], (1.0 - (2.0 * k + 1.0) / K).astype(np.float32))
    assert not np.array_equal(SF.sphere_points(64), SF.sphere_points(128)[:64])
    for K in (0, 32, 100, 320, -64):
        with pytest.raises(ValueError):
            SF.sphere_points(K)


def test_two_equal_spheres_bury_the_cap_fraction():
    """Two spheres of R = 1.7 + 1.4 = 3.1 at distance d: each loses the cap beyond the mid-plane, the fraction (1 - d / (2R)) / 2 of its
    points.  Over d = 0.3 .. 6.0 along x, y and z the lattice's count stays within 4 points of f K (measured: 2.48, 2.97, 3.06 points
    for K = 64, 128, 256; the bound is the next whole point)."""
    R = float(np.float32(1.7)) + float(np.float32(1.4))
    for K in (64, 128, 256):
        worst = 0.0
        for axis in range(3):
            for d in np.arange(3, 61) / 10.0:
                lig = np.zeros((1, 3), np.float32)
                lig[0, axis] = d
                r = one(np.zeros((1, 3)), [1.7], lig, [1.7], K=K)
                f = (1.0 - float(lig[0, axis]) / (2.0 * R)) / 2.0
                assert r["rec_exposed"][0] == K and r["lig_exposed"][0] == K
                worst = max(worst, abs(r["rec_buried"][0, 0] - f * K), abs(r["lig_buried"][0, 0] - f * K))
        print(f"K {K}: largest |count - f K| = {worst:.2f} points")
        assert worst <= 4.0


def test_small_cases():
    R = float(np.float32(1.7)) + float(np.float32(1.4))
    for d in (2 * R, 2 * R + 0.5, 40.0):      # d >= 2R buries nothing
        r = one([[0, 0, 0]], [1.7], [[d, 0, 0]], [1.7])
        assert r["bsa"][0] == 0.0 and not r["class_points"].any() and not r["lig_buried"].any() and not r["rec_buried"].any()
    # a ligand atom at a receptor atom's centre loses all its exposed points, and so does the receptor atom
    r = one([[1, 2, 3]], [1.7], [[1, 2, 3]], [1.52])
    assert r["lig_buried"][0, 0] == 128 and r["lig_points"][0] == 128
    assert r["rec_buried"][0, 0] == 0      # the smaller ligand sphere lies inside the receptor's: it holds none of its points
    # an atom with no exposed point buries nothing of its own
    rec = np.array([[0, 0, 0], [0.1, 0, 0]], np.float32)
    r = one(rec, [1.0, 1.9], [[2.0, 0, 0]], [1.7])
    assert r["rec_exposed"][0] == 0 and r["rec_buried"][0, 0] == 0 and r["rec_buried"][0, 1] > 0
    # a non-finite transform gives zeros
    from dfmdock_amd import surface as SF
    rot = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    tr = np.array([[0, 0, 0], [0, 0, 0], [np.inf, 0, 0]], np.float32)
    r = SF.bsa(rec, [1.7, 1.7], [[2.0, 0, 0]], [1.7], np.zeros(3, np.float32), rot, tr)
    assert r["bsa"][0] > 0 and r["bsa"][1] == 0 and r["bsa"][2] == 0 and not r["lig_buried"][1:].any() and not r["class_points"][1:].any()


def brute(rec, rr, lig, lr, center, rot, tr, probe, K):
    """Triple loops over atoms, points and atoms, scalar arithmetic only."""
    from dfmdock_amd import pdbio
    from dfmdock_amd import surface as SF
    from dfmdock_amd import sterics as ST
    u = SF.sphere_points(K).astype(np.float64)
    rec = np.asarray(rec, np.float32).astype(np.float64)
    lig32 = np.asarray(lig, np.float32)
    Rr = np.asarray(rr, np.float32).astype(np.float64) + float(np.float32(probe))
    Rl = np.asarray(lr, np.float32).astype(np.float64) + float(np.float32(probe))
    dist = lambda q, c: float(np.sqrt((q[0] - c[0]) * (q[0] - c[0]) + (q[1] - c[1]) * (q[1] - c[1]) + (q[2] - c[2]) * (q[2] - c[2])))

    def exposed(x, R):
        out = np.ones((len(x), K), bool)
        for i in range(len(x)):
            for k in range(K):
                q = [x[i][c] + R[i] * u[k][c] for c in range(3)]
                for j in range(len(x)):
                    if j != i and dist(q, x[j]) < R[j]:
                        out[i, k] = False
        return out
    er, el = exposed(rec, Rr), exposed(lig32.astype(np.float64), Rl)
    P = len(rot)
    lb, rb = np.zeros((P, len(lig32)), np.int32), np.zeros((P, len(rec)), np.int32)
    for p in range(P):
        X = ST.pose_atoms(lig32, center, rot[p], tr[p])
        M = pdbio.axis_angle_to_matrix(np.asarray(rot[p], np.float32)).astype(np.float64)
        for a in range(len(X)):
            for k in range(K):
                w = [(M[c, 0] * u[k, 0] + M[c, 1] * u[k, 1]) + M[c, 2] * u[k, 2] for c in range(3)]
                q = [X[a][c] + Rl[a] * w[c] for c in range(3)]
                if el[a, k] and any(dist(q, rec[b]) < Rr[b] for b in range(len(rec))):
                    lb[p, a] += 1
        for b in range(len(rec)):
            for k in range(K):
                q = [rec[b][c] + Rr[b] * u[k][c] for c in range(3)]
                if er[b, k] and any(dist(q, X[a]) < Rl[a] for a in range(len(X))):
                    rb[p, b] += 1
    return er.sum(1), el.sum(1), lb, rb


def test_definition_equals_a_triple_loop_on_a_toy():
    from dfmdock_amd import surface as SF
    rng = np.random.default_rng(1)
    rec, lig = (4.0 * rng.random((7, 3))).astype(np.float32), (4.0 * rng.random((5, 3)) + np.array([3.0, 0, 0])).astype(np.float32)
    rr = np.array([1.7, 1.55, 1.52, 1.8, 1.7, 1.9, 1.55], np.float32)
    lr = np.array([1.52, 1.7, 1.8, 1.55, 1.7], np.float32)
    rot = (0.6 * rng.standard_normal((3, 3))).astype(np.float32)
    tr = (1.0 * rng.standard_normal((3, 3))).astype(np.float32)
    cen = lig.mean(0)
    got = SF.bsa(rec, rr, lig, lr, cen, rot, tr, K=64)
    er, el, lb, rb = brute(rec, rr, lig, lr, cen, rot, tr, 1.4, 64)
    assert np.array_equal(got["rec_exposed"], er) and np.array_equal(got["lig_exposed"], el)
    assert np.array_equal(got["lig_buried"], lb) and np.array_equal(got["rec_buried"], rb) and lb.sum() > 50 and rb.sum() > 50
    assert np.array_equal(got["lig_points"], lb.sum(1)) and np.array_equal(got["rec_points"], rb.sum(1))


def test_the_bounding_box_shortcut_changes_nothing():
    """Candidates from sterics.near_pairs against every atom pair, on CA and CB of a DB5 complex (one pose, K = 64)."""
    from dfmdock_amd import pdbio
    from dfmdock_amd import surface as SF
    c = db5_complex(db5_ids()[0])
    pick = lambda bb: pdbio.full_backbone(bb).reshape(-1, 5, 3)[:, [1, 4]].reshape(-1, 3).astype(np.float32)
    rec, lig = pick(c["rec_pos"]), pick(c["lig_pos"])
    rr, lr = np.full(len(rec), 1.7, np.float32), np.full(len(lig), 1.7, np.float32)
    cen = lig.mean(0)
    rot, tr = np.array([[0.05, -0.1, 0.02]], np.float32), np.array([[0.5, -1.0, 0.25]], np.float32)
    st = {}
    a = SF.bsa(rec, rr, lig, lr, cen, rot, tr, K=64, stats=st)
    b = SF.bsa(rec, rr, lig, lr, cen, rot, tr, K=64, shortcut=False)
    assert st["near_pairs"] < 0.05 * len(rec) * len(lig) and a["lig_points"][0] > 50 and a["rec_points"][0] > 50
    for k in ("rec_exposed", "lig_exposed", "lig_buried", "rec_buried", "class_points", "bsa"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_bsa_is_the_class_sum_in_the_stated_order():
    from dfmdock_amd import surface as SF
    rng = np.random.default_rng(4)
    rec, lig = (6.0 * rng.random((40, 3))).astype(np.float32), (6.0 * rng.random((30, 3)) + 3.0).astype(np.float32)
    radii = np.array([1.52, 1.55, 1.7, 1.8, 1.9], np.float32)
    rr, lr = radii[rng.integers(0, 5, 40)], radii[rng.integers(0, 4, 30)]
    r = SF.bsa(rec, rr, lig, lr, lig.mean(0), Z3, Z3)
    assert np.array_equal(r["class_radius"], np.unique(np.concatenate([rr, lr]))) and r["bsa"][0] > 0
    s = 0.0
    for chain in range(2):
        for c, v in enumerate(r["class_radius"]):
            R = float(v) + float(np.float32(1.4))
            s = s + float(r["class_points"][0, chain, c]) * (4.0 * np.pi * R * R / 128)
    assert s == r["bsa"][0]
    br, bl = SF.side_areas(r["class_points"], r["class_radius"], 1.4, 128)
    assert abs(br[0] + bl[0] - s) < 1e-9 and br[0] > 0 and bl[0] > 0
    cls = np.searchsorted(r["class_radius"], rr)
    assert np.array_equal(r["class_points"][0, 0], np.bincount(cls, weights=r["rec_buried"][0], minlength=16).astype(np.int32))
    with pytest.raises(ValueError):
        SF.bsa(rec[:17], (1.0 + 0.01 * np.arange(17)).astype(np.float32), lig, lr, lig.mean(0), Z3, Z3)
    SF.radius_classes((1.0 + 0.01 * np.arange(16)).astype(np.float32), np.float32([1.0, 1.15]))      # 16 distinct values are fine
    for bad in (dict(probe=0.0), dict(probe=float("nan")), dict(K=96)):
        with pytest.raises(ValueError):
            SF.bsa(rec, rr, lig, lr, lig.mean(0), Z3, Z3, **bad)
    with pytest.raises(ValueError):
        SF.bsa(rec, -rr, lig, lr, lig.mean(0), Z3, Z3)


PDB = """\
ATOM      1  N   ALA A   1       0.000   0.000   0.000  1.00  0.00           N
ATOM      2  CA  ALA A   1       1.458   0.000   0.000  1.00  0.00           C
ATOM      3  C   ALA A   1       2.000   1.400   0.000  1.00  0.00
ATOM      4  O   ALA A   1       1.900  -0.800   0.000  1.00  0.00
ATOM      5  SG  CYS A   2       3.300   1.500   0.000  1.00  0.00           S
ATOM      6 SE   CYS A   2       3.900   2.800   0.000  1.00  0.00          SE
ATOM      7  P   CYS A   2       5.400   2.700   0.000  1.00  0.00           P
ATOM      8 ZN    ZN A   3       5.400   2.700   1.000  1.00  0.00          ZN
ATOM      9  OXT  ZN A   3       6.400   2.700   1.000  1.00  0.00
END
"""


def test_host_finishes(tmp_path):
    from dfmdock_amd import pdbio
    from dfmdock_amd import sterics as ST
    from dfmdock_amd import surface as SF
    path = tmp_path / "x.pdb"
    path.write_text(PDB)
    atoms = pdbio.read_pdb(str(path))
    assert [SF.element_radius(a) for a in atoms] == [1.55, 1.70, 1.70, 1.52, 1.80, 1.90, 1.80, 1.80, 1.52]      # C and O from the name
    rad = SF.atom_radii(atoms)
    assert rad.dtype == np.float32 and np.array_equal(SF.atom_radii(atoms, [0, 3]), np.float32([1.55, 1.52]))
    keys, res = ST.residue_of_atoms(atoms)
    assert res.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2]
    buried = np.array([3, 0, 2, 5, 0, 0, 4, 0, 1])
    area = SF.residue_bsa(buried, rad, res, 3, 1.4, 128)
    A = lambda v: 4.0 * np.pi * (float(np.float32(v)) + float(np.float32(1.4))) ** 2 / 128
    assert np.allclose(area, [3 * A(1.55) + 2 * A(1.70) + 5 * A(1.52), 4 * A(1.80), 1 * A(1.52)], rtol=1e-13, atol=0)
    assert SF.residue_bsa(np.stack([buried, 2 * buried]), rad, res, 3).shape == (2, 3)
    out = tmp_path / "iface.txt"
    SF.write_interface_residues(str(out), (keys, keys[:2]), (area, [0.0, 12.345]))
    lines = out.read_text().splitlines()
    assert lines[0].startswith("#") and lines[1:] == [f"rec A:1 ALA {area[0]:.2f}", f"rec A:2 CYS {area[1]:.2f}", f"rec A:3 ZN {area[2]:.2f}",
                                                      "lig A:2 CYS 12.35"]
    assert SF.min_bsa_flags([0.0, 799.9, 800.0, 1500.0, np.nan], 800.0).tolist() == [True, True, False, False, False]


def test_driver_helpers(tmp_path):
    from dfmdock_amd import cli, driver
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, _, _ = cli.load_pair(rec_pdb, lig_pdb, feat)
    ra, rr, la, lr, cen = driver.surface_inputs(rec, lig, 0)
    ra0, la0, cen0 = driver.sterics_inputs(rec, lig, 0)
    assert np.array_equal(ra, ra0) and np.array_equal(la, la0) and np.array_equal(cen, cen0)
    assert rr.dtype == lr.dtype == np.float32 and rr.shape == (len(ra),) and lr.shape == (len(la),) and set(rr.tolist()) <= {np.float32(v).item() for v in (1.7, 1.55, 1.52, 1.8)}
    assert driver._check_surface(False, None, 1.4, 128) is None
    assert driver._check_surface(True, None, 1.4, 128) == (None, float(np.float32(1.4)), 128)
    assert driver._check_surface(False, 900, 1.4, 64)[0] == 900.0
    for bad in ((True, None, 0.0, 128), (True, None, 1.4, 100), (True, float("nan"), 1.4, 128)):
        with pytest.raises(ValueError):
            driver._check_surface(*bad)
    bd = {"bsa": np.array([1200.5, 300.0]), "bsa_rec": np.array([610.25, 140.0]), "bsa_lig": np.array([590.25, 160.0]), "probe": 1.4, "sphere_points": 128}
    r = driver._surface_result(bd, 1, (500.0, 1.4, 128))
    assert (r["bsa"], r["bsa_rec"], r["bsa_lig"], r["index"], r["min_bsa"]) == (300.0, 140.0, 160.0, 1, 500.0)
    assert "min_bsa" not in driver._surface_result(bd, 0, (None, 1.4, 128)) and driver._surface_result(None, 0, None) == {}
    json.dumps(driver._pose_bsa(bd, 0))


def test_cli_flags_parse_default_off_and_reach_the_driver(tmp_path, monkeypatch, capsys):
    from dfmdock_amd import cli, driver, pdbio
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert not a.bsa and a.min_bsa is None and a.interface_residues is None and cli.surface_kwargs(a) == {}
        assert cli.surface_kwargs(cli.parse_args([cmd] + base + ["--bsa"])) == dict(bsa=True, min_bsa=None, probe=1.4, sphere_points=128)
        a = cli.parse_args([cmd] + base + ["--min-bsa", "800", "--probe", "1.2", "--sphere-points", "256"])
        assert cli.surface_kwargs(a) == dict(bsa=True, min_bsa=800.0, probe=1.2, sphere_points=256)
        assert cli.parse_args([cmd] + base + ["--interface-residues", "x.txt"]).bsa
        for bad in (["--probe", "1.2"], ["--sphere-points", "64"], ["--bsa", "--sphere-points", "100"], ["--bsa", "--probe", "0"],
                    ["--min-bsa", "nan"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c", "--bsa"])
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))

    def dock_pair(model, rec, lig, rec_x, lig_x, **kw):
        seen.update(kw)
        res = {"energy": -1.5, "precision": "mfma16", "rot_update": np.zeros(3, np.float32), "tr_update": np.ones(3, np.float32), "selfcheck": None}
        if kw.get("bsa"):
            res.update(bsa=1234.5, bsa_rec=600.25, bsa_lig=634.25, probe=1.4, sphere_points=128, index=4)
            if kw.get("top_k"):
                res.update(models=[{"rank": 1, "index": 4, "energy": -1.5, "cluster_size": 3, "bsa": 1234.5, "bsa_rec": 600.25, "bsa_lig": 634.25}],
                           bsa_dropped=2)
        return res

    def residue_surface(model, rec, lig, rot, tr, probe, K):
        seen["residue_call"] = (np.asarray(rot).tolist(), np.asarray(tr).tolist(), probe, K)
        kr, kl = [tuple(k) for k in rec["residues"]], [tuple(k) for k in lig["residues"]]
        ar, al = np.zeros(len(kr)), np.zeros(len(kl))
        ar[1], al[2] = 40.5, 17.25
        return [kr, kl], [ar, al]

    def forbidden(*a, **k):
        raise AssertionError("a dock run without the surface flags called the surface code")
    monkeypatch.setattr(driver, "dock_pair", dock_pair)
    monkeypatch.setattr(driver, "residue_surface", forbidden)
    monkeypatch.setattr(driver, "ensemble_surface", forbidden)
    args = ["dock", rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb")]
    assert cli.main(args) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any(k.startswith(("bsa", "min_bsa", "probe", "sphere", "interface", "index")) for k in plain)
    assert not any(k in seen for k in ("bsa", "min_bsa", "probe", "sphere_points"))
    seen.clear()
    monkeypatch.setattr(driver, "residue_surface", residue_surface)
    assert cli.main(args + ["--min-bsa", "900", "--top-k", "3", "--interface-residues", str(tmp_path / "iface.txt")]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["bsa"] is True and seen["min_bsa"] == 900.0 and (seen["probe"], seen["sphere_points"]) == (1.4, 128)
    assert (line["bsa"], line["bsa_rec"], line["bsa_lig"], line["min_bsa"], line["bsa_dropped"], line["index"]) == (1234.5, 600.25, 634.25, 900.0, 2, 4)
    assert line["models"][0]["bsa"] == 1234.5 and {k: v for k, v in line.items() if k in plain} == plain
    assert seen["residue_call"] == ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 1.4, 128) and os.path.samefile(line["interface_residues"], tmp_path / "iface.txt")
    kr = pdbio.backbone_from_atoms(pdbio.read_pdb(rec_pdb))["residues"][1]
    kl = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))["residues"][2]
    assert (tmp_path / "iface.txt").read_text().splitlines()[1:] == [f"rec {kr[0]}:{kr[1]} {kr[3]} 40.50", f"lig {kl[0]}:{kl[1]} {kl[3]} 17.25"]


def test_struct_layout_and_exports(tmp_path):
    """dfm_surface_params / dfm_bsa_out as gcc lays them out against the ctypes mirrors; the new symbols are exported and listed."""
    from dfmdock_amd import _lib
    pairs = (("dfm_surface_params", _lib.SurfaceParamsC), ("dfm_bsa_out", _lib.BsaOutC))
    body = ""
    for c_name, cls in pairs:
        body += f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(
            f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    for c_name, cls in pairs:
        assert int(got[c_name]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_surface_create", "dfm_surface_destroy", "dfm_surface_info", "dfm_pose_bsa", "dfm_pose_bsa_chunked", "dfm_bsa_last_timing"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    # argument checks run before any device work
    assert lib.dfm_surface_create(None, 1, None, None, 1, None, None, None, None) is None and b"m is NULL" in lib.dfm_last_error()
    assert lib.dfm_pose_bsa(None, 1, None, None, None) == -1 and lib.dfm_bsa_last_timing(None, None) == -1
    assert lib.dfm_surface_info(None, *([None] * 9)) == -1


def test_the_audits_see_the_new_kernels():
    """The three kernels of kernels_surface.hip are in the shipped code object (so the scratch / LDS / op_sel audits of test_abi_cpu.py run
    over them), use no scratch, and the main kernel holds static LDS; the file is built without contraction."""
    import re
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_surface.hip")).read()
    names = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))
    assert names == {"k_surface_pose", "k_surface", "k_surface_finish"}
    mk = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "Makefile")).read()
    assert re.search(r"kernels_surface\.o: kernels_surface\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(COMMON\) \$\(STRICT\)", mk)
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
                    if re.search(r"\d+" + n + r"(E|P|N|\b)", name):
                        found[n] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                                    int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)))
        print(found)
        assert set(found) == names and all(v[0] == 0 for v in found.values()) and found["k_surface"][1] >= 16384
    finally:
        shutil.rmtree(td, ignore_errors=True)
