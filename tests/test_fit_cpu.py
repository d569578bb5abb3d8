"""The rigid pose fit and the rescoring door without a GPU: the float64 definition dfmdock_amd/fit.py, the decoy readers
pdbio.read_models / match_model, the `rescore` parser and the argument checks of dfm_pose_fit (which run before any device work)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fit_harness as fh
from conftest import ROOT


def rotmat(rot):
    from dfmdock_amd.pdbio import axis_angle_to_matrix
    return axis_angle_to_matrix(rot)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", (0, 1))
@pytest.mark.parametrize("R", (0, 40))
def test_fit_recovers_seeded_poses(family, R):
    """(rot, tr) applied with cluster.rebuild_backbone about that family's centre come back, as rotation matrices and translations, to
    the accuracy the fp32 coordinates leave (1.5e-5 A per coordinate over lever arms of tens of A)."""
    from dfmdock_amd.cluster import rebuild_backbone
    from dfmdock_amd.fit import fit_poses
    cs = fh.case(100 + family, 6, 70, R, family)
    lig_pos = rebuild_backbone(cs["lig_ref"], cs["rot"], cs["tr"], family)
    if not R:      # the decoys are rebuild_backbone's own poses (the harness rotates about the centre rounded to fp32: the same to 1 ulp)
        assert np.abs(lig_pos - cs["lig_pos"]).max() < 4e-5
        cs["lig_pos"] = lig_pos
    rot, tr, rmsd, rec_rmsd = fit_poses(cs["lig_ref"], cs["lig_pos"], cs["center"], cs["rec_ref"], cs["rec_pos"])
    assert (rmsd < 1e-4).all() and ((rec_rmsd is None) if not R else (rec_rmsd < 1e-4).all())
    for p in range(6):
        np.testing.assert_allclose(rotmat(rot[p]), rotmat(cs["rot"][p]), atol=2e-6)
        np.testing.assert_allclose(tr[p], cs["tr"][p], atol=1e-4)
        assert 0.0 <= np.linalg.norm(rot[p]) <= np.pi
    back = rebuild_backbone(cs["lig_ref"], rot, tr, family)
    assert np.abs(back.astype(np.float64) - lig_pos).max() < 1e-4


def test_fit_agrees_with_the_three_fits_of_metrics():
    """On the same points fit_poses is metrics.find_rigid_alignment: the receptor fit, the ligand fit carried through it, and the explicit
    residuals of compute_metrics' RMSDs."""
    from dfmdock_amd import metrics as MT
    from dfmdock_amd.fit import fit_poses
    cs = fh.case(9, 3, 33, 21)
    rot, tr, rmsd, rec_rmsd = fit_poses(cs["lig_ref"], cs["lig_pos"], cs["center"], cs["rec_ref"], cs["rec_pos"])
    c = cs["center"].astype(np.float64)
    for p in range(3):
        y, y_ref = cs["rec_pos"][p].astype(np.float64).reshape(-1, 3), cs["rec_ref"].astype(np.float64).reshape(-1, 3)
        x, x0 = cs["lig_pos"][p].astype(np.float64).reshape(-1, 3), cs["lig_ref"].astype(np.float64).reshape(-1, 3)
        Q, s = MT.find_rigid_alignment(y, y_ref)
        assert rec_rmsd[p] == MT._rmsd(y @ Q.T + s, y_ref)
        Rm, t = MT.find_rigid_alignment(x0, x @ Q.T + s)
        assert rmsd[p] == MT._rmsd(x0 @ Rm.T + t, x @ Q.T + s)
        np.testing.assert_allclose(rotmat(rot[p]), Rm, atol=1e-12)
        np.testing.assert_allclose(tr[p], t + Rm @ c - c, atol=1e-12)
    # all atoms of the complex as one chain: c_rmsd's fit of a decoy that is a rigid image of the whole complex is exact too
    whole_ref = np.concatenate([cs["rec_ref"], cs["lig_ref"]])
    whole = np.concatenate([cs["rec_pos"][0], cs["lig_pos"][0]])
    _, _, r_lig_frame, _ = fit_poses(whole_ref, whole[None], cs["center"])
    m = MT.compute_metrics((cs["rec_pos"][0], cs["lig_pos"][0]), (cs["rec_ref"], cs["lig_ref"]))
    assert r_lig_frame[0] == pytest.approx(m["c_rmsd"], abs=1e-9)


def test_identity_and_nan_poses():
    from dfmdock_amd.fit import fit_poses, matrix_to_axis_angle
    cs = fh.case(4, 3, 20, 12)
    lig = np.stack([cs["lig_ref"], cs["lig_pos"][1], cs["lig_ref"]])
    rec = np.stack([cs["rec_ref"], cs["rec_pos"][1], cs["rec_ref"]])
    rot, tr, rmsd, rec_rmsd = fit_poses(cs["lig_ref"], lig[:1], cs["center"])
    assert not rot.any() and not tr.any() and rmsd[0] == 0.0 and rec_rmsd is None
    assert not matrix_to_axis_angle(np.eye(3)).any()
    lig[2, 5, 1, 0] = np.nan
    rot, tr, rmsd, rec_rmsd = fit_poses(cs["lig_ref"], lig, cs["center"], cs["rec_ref"], rec)
    assert np.isnan(rot[2]).all() and np.isnan(tr[2]).all() and np.isnan(rmsd[2]) and np.isnan(rec_rmsd[2])
    assert np.isfinite(rot[:2]).all() and np.isfinite(tr[:2]).all() and (rmsd[:2] < 1e-4).all() and (rec_rmsd[:2] < 1e-4).all()
    rec[1, 0, 0, 0] = np.inf
    assert np.isnan(fit_poses(cs["lig_ref"], lig, cs["center"], cs["rec_ref"], rec)[0][1]).all()
    with pytest.raises(ValueError):
        fit_poses(cs["lig_ref"], lig, cs["center"], cs["rec_ref"], None)
    # a half turn: the angle is pi, whichever of the two axes comes out
    half = matrix_to_axis_angle(np.diag([-1.0, -1.0, 1.0]))
    assert np.linalg.norm(half) == pytest.approx(np.pi, abs=1e-12) and abs(half[2]) == pytest.approx(np.pi, abs=1e-12)


# ---- reading decoys ---------------------------------------------------------------------------------------------------------------------
def small_pair(tmp_path, R=7, L=5, seed=2):
    """A seeded pair written as rec.pdb (chain A) / lig.pdb (chain B) and parsed back, so that its coordinates are what a file holds."""
    from dfmdock_amd import pdbio
    rng = np.random.default_rng(seed)
    rec_bb, lig_bb = np.round(fh.chain(rng, R, np.zeros(3), 12.0), 3), np.round(fh.chain(rng, L, np.array([15.0, 0.0, 0.0]), 8.0), 3)
    seqs = ("ACDEFGH" * 3)[:R], ("KLMNPQR" * 3)[:L]
    out = []
    for name, bb, seq, first in (("rec.pdb", rec_bb, seqs[0], True), ("lig.pdb", lig_bb, seqs[1], False)):
        p = str(tmp_path / name)
        pdbio.write_backbone_pdb(p, pdbio.full_backbone(bb), seq, delim=len(seq) - 1 if first else -1, mode="w")
        out.append(pdbio.backbone_from_atoms(pdbio.read_pdb(p)))
    return out[0], out[1]


def test_read_models_and_match_model(tmp_path):
    from dfmdock_amd import pdbio
    rec, lig = small_pair(tmp_path)
    rot, tr = fh.random_poses(np.random.default_rng(1), 3, 10.0)
    moved = [pdbio.apply_pose_all_atom(lig["aa_coords"], lig["bb_coords"], rot[p], tr[p]) for p in range(3)]
    # one model per file (write_complex_pdb has no MODEL record): read_pdb's atoms
    one = str(tmp_path / "one.pdb")
    pdbio.write_complex_pdb(one, rec["atoms"], lig["atoms"], moved[0])
    models = pdbio.read_models(one)
    assert len(models) == 1 and models[0] == pdbio.read_pdb(one)
    lb, rb = pdbio.match_model(models[0], rec, lig, source=one)
    want = pdbio.backbone_from_atoms([dict(a, coord=tuple(np.round(c, 3))) for a, c in zip(lig["atoms"], moved[0])])["bb_coords"]
    np.testing.assert_allclose(lb, want, atol=1e-9)
    np.testing.assert_array_equal(rb, rec["bb_coords"])
    # several models in one file, the second ligand-only, the third with a moved receptor
    g_rot, g_tr = fh.random_poses(np.random.default_rng(2), 1, 10.0)
    rec_moved = [dict(a, coord=tuple(c)) for a, c in zip(rec["atoms"], pdbio.apply_pose_all_atom(rec["aa_coords"], rec["bb_coords"], g_rot[0], g_tr[0]))]
    multi = str(tmp_path / "multi.pdb")
    with open(multi, "w") as f:
        for i, (ra, xyz) in enumerate(((rec["atoms"], moved[0]), ([], moved[1]), (rec_moved, moved[2]))):
            part = str(tmp_path / "part.pdb")
            pdbio.write_complex_pdb(part, ra, lig["atoms"], xyz)
            f.write(f"MODEL     {i + 1:4d}\n" + open(part).read().replace("END\n", "") + "ENDMDL\n")
        f.write("END\n")
    models = pdbio.read_models(multi)
    assert len(models) == 3 and [len(m) for m in models] == [len(rec["atoms"]) + len(lig["atoms"]), len(lig["atoms"]), len(rec["atoms"]) + len(lig["atoms"])]
    assert pdbio.read_pdb(multi) == models[0]      # read_pdb still reads the first model only
    got = [pdbio.match_model(m, rec, lig, source=multi, model=i + 1) for i, m in enumerate(models)]
    assert got[1][1] is None and got[0][1] is not None
    np.testing.assert_allclose(got[2][1], pdbio.apply_pose_all_atom(rec["bb_coords"].reshape(-1, 3), rec["bb_coords"], g_rot[0], g_tr[0]).reshape(-1, 3, 3),
                               atol=6e-4)
    # the frames of write_trajectory_pdb (MODEL records, no ENDMDL; one numbering over both chains): the pair as that file names it
    traj = str(tmp_path / "traj.pdb")
    frames = np.stack([lig["bb_coords"] + d for d in (0.0, 1.0, 2.5)]).astype(np.float32)
    pdbio.write_trajectory_pdb(traj, [rec["bb_coords"].astype(np.float32)] * 3, frames, rec["seq"], lig["seq"])
    tm = pdbio.read_models(traj)
    assert len(tm) == 3
    trec, tlig = (pdbio.backbone_from_atoms([a for a in tm[0] if a["chain"] == ch]) for ch in "AB")
    for i in range(3):
        lb, rb = pdbio.match_model(tm[i], trec, tlig, source=traj, model=i)
        np.testing.assert_allclose(lb, frames[i], atol=6e-4)
        np.testing.assert_allclose(rb, rec["bb_coords"], atol=6e-4)


def test_match_model_errors_name_file_model_and_residue(tmp_path):
    from dfmdock_amd import pdbio
    rec, lig = small_pair(tmp_path)
    full = str(tmp_path / "full.pdb")
    pdbio.write_complex_pdb(full, rec["atoms"], lig["atoms"], lig["aa_coords"])
    atoms = pdbio.read_models(full)[0]
    third = lig["residues"][2]
    label = f"{third[3]} {third[0]}{third[1]}"
    missing = [a for a in atoms if (a["chain"], a["res_id"]) != (third[0], third[1])]
    with pytest.raises(ValueError, match=rf"decoys\.pdb, model 4: ligand residue {label} is missing"):
        pdbio.match_model(missing, rec, lig, source="decoys.pdb", model=4)
    no_ca = [a for a in atoms if not ((a["chain"], a["res_id"]) == (third[0], third[1]) and a["name"] == "CA")]
    with pytest.raises(ValueError, match=rf"model 1: ligand residue {label} is missing an N, CA or C atom"):
        pdbio.match_model(no_ca, rec, lig, source="decoys.pdb")
    is3 = lambda a: (a["chain"], a["res_id"]) == (third[0], third[1])
    reordered = [a for a in atoms if a["chain"] == "A"] + [a for a in atoms if is3(a)] + [a for a in atoms if a["chain"] == "B" and not is3(a)]
    with pytest.raises(ValueError, match=r"x\.pdb, model 2: ligand residue .* is out of place"):
        pdbio.match_model(reordered, rec, lig, source="x.pdb", model=2)
    rec_gap = [a for a in atoms if (a["chain"], a["res_id"]) != (rec["residues"][1][0], rec["residues"][1][1])]
    with pytest.raises(ValueError, match=r"model 1: receptor residue .* is missing"):
        pdbio.match_model(rec_gap, rec, lig, source="x.pdb")
    # a shared chain id: the inputs alone cannot tell the sides apart
    lig_a = pdbio.backbone_from_atoms([dict(a, chain="A") for a in lig["atoms"]])
    with pytest.raises(ValueError, match="share the chain id.*--decoy-chains"):
        pdbio.match_model(atoms, rec, lig_a)
    lb, rb = pdbio.match_model(atoms, rec, lig_a, rec_chains="A", lig_chains="B")
    np.testing.assert_array_equal(lb, lig["bb_coords"])
    np.testing.assert_array_equal(rb, rec["bb_coords"])
    with pytest.raises(ValueError, match="one chain per chain"):
        pdbio.match_model(atoms, rec, lig_a, rec_chains="AC", lig_chains="B")


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_rescore_parser(tmp_path, capsys, monkeypatch):
    from dfmdock_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["rescore", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    dock = cli.build_parser()._subparsers._group_actions[0].choices["dock"].format_help()
    analysis_flags = set()
    for a in cli.ANALYSES:
        import argparse
        p = argparse.ArgumentParser()
        a.add(p)
        analysis_flags |= {s for act in p._actions for s in act.option_strings if s.startswith("--") and s != "--help"}
    assert len(analysis_flags) > 30
    for flag in sorted(analysis_flags | {"--decoys", "--coords", "--poses", "--decoy-chains", "--fit-tolerance", "--score-t", "--scores", "--top-k",
                                         "--cluster-radius", "--cluster-rule", "--refine-t", "--refine-samples", "--native", "--out", "--json"}):
        assert flag in text, flag
        assert flag in dock or flag in ("--decoys", "--coords", "--poses", "--decoy-chains", "--fit-tolerance", "--score-t", "--scores"), flag
    assert "rescore" in cli.build_parser().format_help()
    # an argument error comes before any model is loaded
    monkeypatch.setattr(cli, "load_model", lambda args: pytest.fail("the model was loaded before the arguments were checked"))
    poses = str(tmp_path / "p.npz")
    np.savez(poses, rot_update=np.zeros((2, 3), np.float32), tr_update=np.zeros((2, 3), np.float32))
    base = ["rescore", "r.pdb", "l.pdb", "--ckpt", "c", "--features", "f.npz"]
    for bad, msg in ((["--poses", poses, "--coords", poses], "not allowed with"), ([], "one of the arguments"),
                     (["--poses", poses, "--decoy-chains", "A", "B"], "--decoy-chains names"), (["--poses", str(tmp_path / "none.npz")], "no such file"),
                     (["--poses", poses, "--refine-t", "0.1"], "needs --top-k"), (["--poses", poses, "--fit-tolerance", "-1"], "--fit-tolerance"),
                     (["--poses", poses, "--rank", "pairpot"], "pair"), (["--poses", poses, "--consensus-top", "0.5"], "needs --consensus")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, (bad, msg)
    args = cli.parse_args(base + ["--poses", poses, "--clash-screen", "--bsa", "--top-k", "3"])
    assert args.cmd == "rescore" and args.fit_tolerance == 0.1 and args.score_t is None and args.top_k == 3 and args.clash_screen and args.bsa


def test_decoy_files_of_the_command_line(tmp_path):
    """cli.load_decoys: PDB models (a ligand-only model travels with the input receptor), --coords and --poses, with one name per decoy."""
    import argparse
    from dfmdock_amd import cli, pdbio
    rec, lig = small_pair(tmp_path)
    a, b = str(tmp_path / "a.pdb"), str(tmp_path / "b.pdb")
    pdbio.write_complex_pdb(a, rec["atoms"], lig["atoms"], lig["aa_coords"] + 1.0)
    pdbio.write_complex_pdb(b, [], lig["atoms"], lig["aa_coords"] + 2.0)
    ns = lambda **kw: argparse.Namespace(**dict(dict(decoys=None, coords=None, poses=None, decoy_chains=None), **kw))
    dec, names = cli.load_decoys(ns(decoys=[a, b]), rec, lig)
    assert names == [(a, 1), (b, 1)] and dec["lig_pos"].shape == (2, 5, 3, 3) and dec["rec_pos"].shape == (2, 7, 3, 3)
    np.testing.assert_allclose(dec["lig_pos"][1], lig["bb_coords"] + 2.0, atol=1e-5)
    np.testing.assert_array_equal(dec["rec_pos"][1], rec["bb_coords"].astype(np.float32))
    dec, names = cli.load_decoys(ns(decoys=[b]), rec, lig)
    assert "rec_pos" not in dec and len(names) == 1
    coords = str(tmp_path / "c.npz")
    np.savez(coords, lig_pos=np.zeros((4, 5, 3, 3), np.float32))
    dec, names = cli.load_decoys(ns(coords=coords), rec, lig)
    assert dec["lig_pos"].shape == (4, 5, 3, 3) and "rec_pos" not in dec and names[3] == (coords, 4)
    np.savez(coords, lig_pos=np.zeros((4, 6, 3, 3), np.float32))
    with pytest.raises(ValueError, match="the ligand PDB has 5 residues"):
        cli.load_decoys(ns(coords=coords), rec, lig)


def test_rescore_reports_decoy_mistakes_in_one_line(tmp_path, capsys, monkeypatch):
    """A decoy file that does not match the pair, or an array file without its arrays: `rescore: <message>` on stderr and status 1,
    no traceback, and the driver is never called."""
    import types
    from dfmdock_amd import cli, driver, pdbio
    rec, lig = small_pair(tmp_path)
    monkeypatch.setattr(cli, "load_model", lambda args: (types.SimpleNamespace(hp=types.SimpleNamespace(lm_embed_dim=1301)), None))
    monkeypatch.setattr(cli, "load_pair", lambda *a: (rec, lig, None, None))
    monkeypatch.setattr(driver, "rescore_pair", lambda *a, **k: pytest.fail("the driver ran on decoys that could not be read"))
    third = lig["residues"][2]
    gap = str(tmp_path / "gap.pdb")
    pdbio.write_complex_pdb(gap, rec["atoms"], [a for a in lig["atoms"] if a["res_id"] != third[1]],
                            [c for a, c in zip(lig["atoms"], lig["aa_coords"]) if a["res_id"] != third[1]])
    empty = str(tmp_path / "empty.npz")
    np.savez(empty, other=np.zeros(3))
    base = ["rescore", "r.pdb", "l.pdb", "--ckpt", "c", "--features", "f.npz"]
    for src, msg in ((["--decoys", gap], f"rescore: {gap}, model 1: ligand residue {third[3]} {third[0]}{third[1]} is missing"),
                     (["--coords", empty], f"rescore: {empty}: need lig_pos"), (["--poses", empty], f"rescore: {empty}: need rot_update")):
        assert cli.main(base + src) == 1
        err = capsys.readouterr().err
        assert msg in err and "Traceback" not in err, err


def test_sterics_screen_adds_its_mask_to_the_drivers(monkeypatch):
    """driver._sterics_screen with a stubbed screen: without a mask of the driver's the screen's stands as it always did; with one
    (rescore_pair's rejected decoys) the two add up, neither replaces the other; and when together they would remove every pose the
    filter falls back - `fallback` true, the driver's mask alone."""
    import types
    from dfmdock_amd import driver
    T, F = True, False
    screen = {}
    monkeypatch.setattr(driver, "_screen", lambda model, rec, lig, cols, opts: ({"fallback": False, "filtered": True}, screen["bad"]))
    run = lambda bad: types.SimpleNamespace(model=None, rec=None, lig=None, cols=None, opts={"sterics": (True, 3.0, 5.0)}, data={}, bad=bad)
    flags, rejected = np.array([F, T, F, F]), np.array([T, F, F, F])
    for mine, theirs, want, fallback in ((None, flags, flags, False), (None, None, None, False), (rejected, None, rejected, False),
                                         (rejected, flags, np.array([T, T, F, F]), False), (rejected, ~rejected, rejected, True)):
        screen["bad"] = theirs
        r = run(None if mine is None else mine.copy())
        driver._sterics_screen(r)
        assert (r.bad is None) if want is None else np.array_equal(r.bad, want), (mine, theirs)
        assert r.data["sterics"]["fallback"] is fallback
    assert np.array_equal(rejected, [T, F, F, F])      # the driver's own mask is never written into


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_fit_abi_and_argument_errors(tmp_path):
    """dfm_fit_out as gcc lays it out; the new symbols are exported and listed; every argument error of dfm_pose_fit returns -1 with its
    message before any device work (no GPU is needed: the model handle is never followed)."""
    from dfmdock_amd import _lib
    from test_abi_cpu import header_symbols
    c_name, cls = "dfm_fit_out", _lib.FitOutC
    body = f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[c_name]) == C.sizeof(cls) == 32
    for f, _ in cls._fields_:
        assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_pose_fit", "dfm_pose_fit_chunked", "dfm_fit_last_timing"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and getattr(lib, s).argtypes
    assert sorted(_lib.EXPORTS) == header_symbols()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)      # a model handle nobody follows: every check below returns first
    x = np.zeros(9 * 4, np.float32)
    fp = x.ctypes.data_as(_lib.F32P)
    rmsd = np.zeros(4)
    dp = rmsd.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.FitOutC(fp, fp, dp, None)
    full = _lib.FitOutC(fp, fp, dp, dp)
    ok = dict(m=fake, P=1, L=1, lig_ref=fp, lig_pos=fp, R=0, rec_ref=None, rec_pos=None, center=fp, out=C.byref(out))
    cases = [(dict(m=None), "m is NULL"), (dict(lig_ref=None), "lig_ref is NULL"), (dict(lig_pos=None), "lig_pos is NULL"),
             (dict(center=None), "center is NULL"), (dict(out=None), "out, out->rot, out->tr or out->rmsd is NULL"),
             (dict(out=C.byref(_lib.FitOutC(None, fp, dp, None))), "out->rot"), (dict(P=0), "need P >= 1"), (dict(L=0), "need L >= 1"),
             (dict(rec_ref=fp, R=1), "rec_ref and rec_pos must be given together"), (dict(rec_pos=fp, R=1), "rec_ref and rec_pos must be given together"),
             (dict(rec_ref=fp, rec_pos=fp, R=0, out=C.byref(full)), "need R >= 1 with a receptor"),
             (dict(rec_ref=fp, rec_pos=fp, R=1), "out->rec_rmsd_or_null is NULL with a receptor")]
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.dfm_pose_fit(a["m"], a["P"], a["L"], a["lig_ref"], a["lig_pos"], a["R"], a["rec_ref"], a["rec_pos"], a["center"], a["out"])
        assert rc == -1 and msg.encode() in lib.dfm_last_error(), (change.keys(), lib.dfm_last_error())
    rc = lib.dfm_pose_fit_chunked(fake, 1, 1, fp, fp, 0, None, None, fp, -1, C.byref(out))
    assert rc == -1 and b"chunk_poses must be >= 0" in lib.dfm_last_error()
    assert lib.dfm_fit_last_timing(None, None) == -1


def test_the_fit_kernels_are_in_the_shipped_code_object():
    """k_fit_reduce, k_fit_solve and k_fit_resid are gfx950 kernels of the library (so the audits of test_abi_cpu.py run over them) and use
    no scratch: no dynamically indexed private array survived."""
    import re
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
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
                k = re.search(r"\d+(k_fit_\w+?)E", m.group(1))
                if k:
                    found[k.group(1)] = int(m.group(2))
        assert found == {"k_fit_reduce": 0, "k_fit_solve": 0, "k_fit_resid": 0}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)
