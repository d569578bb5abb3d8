"""`rescore` end to end on 7CEI with the seeded checkpoint (tests/cli_fixtures.py): the eight poses of one `dock` run go back in as PDB
models, as coordinates and as poses, and come out with the energies Complex.score gives by hand, the backbones they went in with, and the
analysis entries dock_pair computes for the same (rot_update, tr_update) columns.

PDB text rounds every coordinate to 1e-3 A (half a unit: 5e-4 A per coordinate, 8.7e-4 A per atom): 2e-3 A bounds the fit's rmsd and the
distance of any recovered backbone atom from where it started, also after a rigid motion of the whole model and its second rounding.
"""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, STEPS, SEED = 8, 6, 3
TEXT = 2e-3


class Setup:
    pass


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    """The pair, the checkpoint, one dock run with the analyses on, and its poses written three ways."""
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    from dfmdock_amd import cli, driver, engine, pdbio
    from dfmdock_amd.cluster import rebuild_backbone
    from dfmdock_amd.weights import load_lightning_checkpoint, pack_blob
    s = Setup()
    s.tmp = str(tmp_path_factory.mktemp("rescore"))
    cx, rs, ls = golden_7cei()
    s.rec_pdb, s.lig_pdb, s.feat = write_pair(s.tmp, cx, rs, ls)
    s.ck = os.path.join(s.tmp, "model_0.ckpt")
    write_ckpt(s.ck, seed=0)
    engine.set_device(0)
    sd, hp = load_lightning_checkpoint(s.ck)
    s.model = engine.Model(pack_blob(sd, hp), hp)
    s.rec, s.lig, s.rec_x, s.lig_x = cli.load_pair(s.rec_pdb, s.lig_pdb, s.feat)
    s.native = cli.load_native((s.rec_pdb, s.lig_pdb))
    s.dock = driver.dock_pair(s.model, s.rec, s.lig, s.rec_x, s.lig_x, num_samples=N, num_steps=STEPS, seed=SEED, max_batch=8, selfcheck=False,
                              out_pdb=os.path.join(s.tmp, "dock.pdb"), clash_screen=True, bsa=True, hbonds=True, top_k=3, native=s.native)
    s.rot, s.tr = s.dock["trajectories"]["rot_update"], s.dock["trajectories"]["tr_update"]
    s.lig0 = np.asarray(s.lig["bb_coords"], np.float32)
    s.backbones = rebuild_backbone(s.lig0, s.rot, s.tr, 0)
    s.poses = os.path.join(s.tmp, "poses.npz")
    np.savez(s.poses, rot_update=s.rot, tr_update=s.tr)
    s.coords = os.path.join(s.tmp, "coords.npz")
    np.savez(s.coords, lig_pos=s.backbones)
    s.aa = [pdbio.apply_pose_all_atom(s.lig["aa_coords"], s.lig["bb_coords"], s.rot[p], s.tr[p]) for p in range(N)]
    s.pdbs = []
    for p in range(N):
        s.pdbs.append(os.path.join(s.tmp, f"decoy_{p}.pdb"))
        pdbio.write_complex_pdb(s.pdbs[-1], s.rec["atoms"], s.lig["atoms"], s.aa[p])
    s.base = [s.rec_pdb, s.lig_pdb, "--ckpt", s.ck, "--features", s.feat, "--seed", str(SEED), "--max-batch", "8", "--no-selfcheck", "--num-steps", str(STEPS)]
    yield s
    s.model.close()


def rescore(S, capsys, extra, expect=0):
    """`rescore` in this process: (exit status, the result line or None, stderr)."""
    from dfmdock_amd import cli
    capsys.readouterr()
    rc = cli.main(["rescore"] + S.base + extra)
    cap = capsys.readouterr()
    assert rc == expect, cap.err
    return json.loads(cap.out.strip().splitlines()[-1]) if rc == 0 else None, cap.err


def by_hand(S, rot, tr, t=1e-3, seed=SEED):
    from dfmdock_amd import engine
    from dfmdock_amd.cluster import rebuild_backbone
    gx = engine.Complex(S.model, S.rec_x, S.lig_x, S.rec["bb_coords"], S.lig["bb_coords"])
    try:
        return gx.score(rebuild_backbone(gx.lig_pos0, rot, tr, 0), t, seed=seed, energy=True, **engine.precision_kwargs("mfma16"))["energy"]
    finally:
        gx.close()


def scores(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_poses_go_through_as_they_are(S, capsys):
    """--poses: the energy column is Complex.score on the rebuilt backbones with the same t, seed and precision; nothing is fitted."""
    from dfmdock_amd import driver
    out = os.path.join(S.tmp, "poses_out.pdb")
    line, _ = rescore(S, capsys, ["--poses", S.poses, "--out", out, "--json", os.path.join(S.tmp, "poses.json"), "--scores", os.path.join(S.tmp, "poses.csv")])
    want = by_hand(S, S.rot, S.tr)
    got = np.array(json.load(open(os.path.join(S.tmp, "poses.json")))["energies"], np.float32)
    np.testing.assert_array_equal(got, want)
    k = int(np.argmin(want))
    assert line["index"] == k and line["energy"] == float(want[k]) and line["num_decoys"] == N and line["t"] == 1e-3
    assert line["fit"] == {"rmsd": 0.0, "rec_rmsd": None, "tolerance": 0.1, "n_rejected": 0}
    assert line["rot_update"] == [float(v) for v in S.rot[k]] and line["tr_update"] == [float(v) for v in S.tr[k]]
    rows = scores(os.path.join(S.tmp, "poses.csv"))
    assert len(rows) == N and [int(r["model"]) for r in rows] == list(range(1, N + 1)) and all(r["rejected"] == "0" for r in rows)
    assert sorted(int(r["rank"]) for r in rows) == list(range(1, N + 1)) and rows[k]["rank"] == "1"
    assert [float(r["energy"]) for r in rows] == [float(e) for e in want]
    # the driver by itself, another time of the evaluation
    res = driver.rescore_pair(S.model, S.rec, S.lig, S.rec_x, S.lig_x, {"rot_update": S.rot, "tr_update": S.tr}, t=0.05, seed=SEED, selfcheck=False,
                              out_pdb=None, max_batch=8)
    np.testing.assert_array_equal(res["trajectories"]["energy"], by_hand(S, S.rot, S.tr, 0.05))
    assert res["t"] == 0.05 and not res["fit_data"]["rejected"].any()
    # more decoys than max_batch: the chunk that starts at decoy p0 is the call made by hand with seed + p0
    res = driver.rescore_pair(S.model, S.rec, S.lig, S.rec_x, S.lig_x, {"rot_update": S.rot, "tr_update": S.tr}, seed=SEED, selfcheck=False,
                              out_pdb=None, max_batch=3)
    chunks = [by_hand(S, S.rot[p0:p0 + 3], S.tr[p0:p0 + 3], seed=SEED + p0) for p0 in range(0, N, 3)]
    np.testing.assert_array_equal(res["trajectories"]["energy"], np.concatenate(chunks))


def test_pdb_text_and_coordinates_round_trip(S, capsys):
    """From PDB text and from --coords: every fit within 2e-3 A, no decoy rejected, the recovered backbones within 2e-3 A of the originals;
    and the same after every model, receptor included, went through a seeded rigid motion of its own."""
    from dfmdock_amd import cli, driver, pdbio
    from dfmdock_amd.cluster import rebuild_backbone
    import argparse
    import fit_harness as fh
    ns = lambda **kw: argparse.Namespace(**dict(dict(decoys=None, coords=None, poses=None, decoy_chains=None), **kw))
    g_rot, g_tr = fh.random_poses(np.random.default_rng(5), N, 30.0)
    moved = []
    for p in range(N):
        every = np.concatenate([S.rec["aa_coords"], S.aa[p]])
        every = pdbio.apply_pose_all_atom(every, S.rec["bb_coords"], g_rot[p], g_tr[p])
        rec_atoms = [dict(a, coord=tuple(c)) for a, c in zip(S.rec["atoms"], every[:len(S.rec["atoms"])])]
        moved.append(os.path.join(S.tmp, f"moved_{p}.pdb"))
        pdbio.write_complex_pdb(moved[-1], rec_atoms, S.lig["atoms"], every[len(S.rec["atoms"]):])
    rec_bb = np.asarray(S.rec["bb_coords"], np.float32)
    fits = {}
    for name, source in (("pdb", ns(decoys=S.pdbs)), ("coords", ns(coords=S.coords)), ("moved", ns(decoys=moved))):
        dec, names = cli.load_decoys(source, S.rec, S.lig)
        assert len(names) == N and ("rec_pos" in dec) == (name != "coords")
        rot, tr, rmsd, rec_rmsd = driver.fit_decoys(S.model, S.lig0, dec, rec_bb)
        back = rebuild_backbone(S.lig0, rot, tr, 0).astype(np.float64)
        dev = float(np.sqrt(((back - S.backbones.astype(np.float64)) ** 2).sum(-1)).max())
        print(name, "fit rmsd max", rmsd.max(), "rec", None if rec_rmsd is None else rec_rmsd.max(), "backbone deviation", dev)
        assert (rmsd < TEXT).all() and (rec_rmsd is None or (rec_rmsd < TEXT).all()) and dev < TEXT
        fits[name] = (rot, tr)
    for p in range(N):      # fp32 backbones, no text rounding: the same rotation (the sampler's own angle may exceed pi, the fit's never does)
        np.testing.assert_allclose(pdbio.axis_angle_to_matrix(fits["coords"][0][p]), pdbio.axis_angle_to_matrix(S.rot[p]), atol=1e-6)
        assert np.linalg.norm(fits["coords"][0][p]) <= np.pi + 1e-6
    assert np.abs(fits["coords"][1] - S.tr).max() < 1e-4
    out = os.path.join(S.tmp, "moved_out.pdb")
    line, _ = rescore(S, capsys, ["--decoys"] + moved + ["--out", out, "--scores", os.path.join(S.tmp, "moved.csv")])
    plain, _ = rescore(S, capsys, ["--decoys"] + S.pdbs + ["--out", os.path.join(S.tmp, "pdb_out.pdb")])
    for ln in (line, plain):
        assert ln["fit"]["n_rejected"] == 0 and ln["fit"]["rmsd"] < TEXT and ln["fit"]["rec_rmsd"] < TEXT and ln["num_decoys"] == N
    assert line["source"] == moved[line["index"]] and line["model"] == 1
    rows = scores(os.path.join(S.tmp, "moved.csv"))
    assert [r["source"] for r in rows] == moved and all(float(r["fit_rmsd"]) < TEXT and float(r["rec_rmsd"]) < TEXT and r["rejected"] == "0" for r in rows)
    # the written complex holds the kept decoy's ligand where it started, in the INPUT's frame
    k = line["index"]
    written = np.array([a["coord"] for a in pdbio.read_pdb(out)[len(S.rec["atoms"]):]])
    assert np.sqrt(((written - S.aa[k]) ** 2).sum(-1)).max() < 2 * TEXT


def test_analyses_models_and_refinement(S, capsys):
    """--clash-screen --bsa --hbonds --top-k 3 --native --refine-t 0.1: the analysis entries of the line are dock_pair's for the same
    columns, every model gains a refined energy."""
    from dfmdock_amd import driver
    out = os.path.join(S.tmp, "an.pdb")
    line, _ = rescore(S, capsys, ["--poses", S.poses, "--out", out, "--clash-screen", "--bsa", "--hbonds", "--top-k", "3", "--native", S.rec_pdb, S.lig_pdb,
                                  "--refine-t", "0.1", "--refine-samples", "2"])
    d, k = S.dock, line["index"]
    js = lambda x: json.loads(json.dumps(x, default=float))
    assert line["sterics"] == js(driver._sterics_result(d["sterics_data"], k)["sterics"])
    for key, v in {**driver._pose_bsa(d["bsa_data"], k), **driver._pose_hbonds(d["hbond_data"], k)}.items():
        assert line[key] == v, key
    assert (line["probe"], line["sphere_points"]) == (d["probe"], d["sphere_points"])
    assert line["metrics"] == js(driver.native_metrics(S.model, S.native, S.rec["bb_coords"], S.backbones[k:k + 1])[0])
    assert 1 <= len(line["models"]) <= 3 and line["models"][0]["index"] == k and line["refine_t"] == 0.1
    for m in line["models"]:
        c = m["index"]
        assert m["sterics"] == js(driver._pose_sterics(d["sterics_data"], c)) and np.isfinite(m["refined_energy"]) and os.path.exists(m["path"])
        for key, v in {**driver._pose_bsa(d["bsa_data"], c), **driver._pose_hbonds(d["hbond_data"], c)}.items():
            assert m[key] == v, key
        assert m["metrics"] == js(driver.native_metrics(S.model, S.native, S.rec["bb_coords"], S.backbones[c:c + 1])[0]) and "refined_metrics" in m
    if d["index"] == k:      # the sampler's own final energy kept the same pose: the whole entries agree, not only their formulas
        assert line["sterics"] == js(d["sterics"]) and line["bsa"] == d["bsa"] and line["n_hbond"] == d["n_hbond"]


def deformed(S, p, name):
    """Decoy p with one ligand residue displaced by 2 A: no rigid image of the input."""
    from dfmdock_amd import pdbio
    aa = S.aa[p].copy()
    res = S.lig["residues"][10]
    sel = [i for i, a in enumerate(S.lig["atoms"]) if (a["chain"], a["res_id"]) == (res[0], res[1])]
    aa[sel] += np.array([1.2, 0.0, 1.6])
    path = os.path.join(S.tmp, name)
    pdbio.write_complex_pdb(path, S.rec["atoms"], S.lig["atoms"], aa)
    return path


def test_rejection(S, capsys):
    """The decoy that would be kept, deformed: it is rejected, listed with rejected = 1 and no energy, and another one is kept, also
    with --clash-filter in the same run (how the two masks add up: tests/test_fit_cpu.py).  All decoys deformed: a non-zero exit and
    a message."""
    best = int(np.argmin(by_hand(S, S.rot, S.tr)))
    files = list(S.pdbs)
    files[best] = deformed(S, best, "bent.pdb")
    line, _ = rescore(S, capsys, ["--decoys"] + files + ["--out", os.path.join(S.tmp, "rej.pdb"), "--scores", os.path.join(S.tmp, "rej.csv"), "--top-k", "8",
                                  "--clash-filter"])
    rows = scores(os.path.join(S.tmp, "rej.csv"))
    assert line["fit"]["n_rejected"] == 1 and line["index"] != best and line["num_decoys"] == N
    assert rows[best]["rejected"] == "1" and rows[best]["energy"] == "" and rows[best]["rank"] == "" and float(rows[best]["fit_rmsd"]) > 0.1
    assert sum(r["rejected"] == "1" for r in rows) == 1 and all(m["index"] != best for m in line["models"])
    flagged = line["sterics"]["filtered"] and not line["sterics"]["fallback"]
    assert not line["sterics"]["flagged"] or not flagged
    p = subprocess.run([sys.executable, "-m", "dfmdock_amd", "rescore"] + S.base + ["--decoys", deformed(S, 0, "bent0.pdb"), deformed(S, 1, "bent1.pdb"),
                                                                                  "--out", os.path.join(S.tmp, "none.pdb")],
                       cwd=S.tmp, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert p.returncode != 0 and "every one of the 2 decoys is rejected" in p.stderr and not os.path.exists(os.path.join(S.tmp, "none.pdb"))
