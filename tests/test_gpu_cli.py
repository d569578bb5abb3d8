"""`python -m dfmdock_amd` end to end on the GPU: a seeded checkpoint written by the test, 7CEI as two PDB files +
a features file (the reference's own backbone, sequence and ESM block: tests/golden/cx_7CEI.npz), and a DB5-style directory.

  dock   <- src/inference_single.py:1-12 / inference() (src/inference_base.py:601-670): output.pdb + {"energy": ...}
  sweep  <- src/inference_mlsb.py:188-262: reference-schema CSV + success-rate table + the self-check lines
"""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_ckpt, write_db5_pt, write_pair
from conftest import ROOT, complex_for

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def test_dock_7cei_end_to_end(tmp_path):
    from dfmdock_amd import cli, driver, engine, pdbio
    from dfmdock_amd.weights import load_lightning_checkpoint, pack_blob
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    p = _run(["dock", rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--num-samples", "9", "--max-batch", "4", "--seed", "5",
              "--json", str(tmp_path / "res.json")], cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert "selfcheck pair" in p.stderr and " OK" in p.stderr and line["selfcheck_ok"] is True and line["precision"] == "mfma16"
    out = tmp_path / "output.pdb"                      # inference() writes output.pdb into the working directory
    assert out.exists() and os.path.samefile(line["output"], out)
    # the same call in process: same energy, same pose
    engine.set_device(0)
    sd, hp = load_lightning_checkpoint(ck)
    model = engine.Model(pack_blob(sd, hp), hp)
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    ref = driver.dock_pair(model, rec, lig, rec_x, lig_x, num_samples=9, num_steps=40, seed=5, max_batch=4, out_pdb=None)
    assert line["energy"] == ref["energy"]
    np.testing.assert_array_equal(np.float32(line["rot_update"]), ref["rot_update"])
    atoms = pdbio.read_pdb(str(out))
    n_rec = len(rec["atoms"])
    assert len(atoms) == n_rec + len(lig["atoms"])
    np.testing.assert_allclose(np.array([a["coord"] for a in atoms[:n_rec]]), rec["aa_coords"], atol=6e-4)      # the receptor as read
    np.testing.assert_allclose(np.array([a["coord"] for a in atoms[n_rec:]]), ref["lig_aa_coords"], atol=6e-4)  # the ligand at the best pose
    moved = np.array([a["coord"] for a in atoms[n_rec:]])
    d0 = np.linalg.norm(lig["aa_coords"][0] - lig["aa_coords"][-1])
    assert abs(np.linalg.norm(moved[0] - moved[-1]) - d0) < 2e-3                                                 # rigid
    res = json.load(open(tmp_path / "res.json"))
    assert res["selfcheck"]["ok"] and res["selfcheck"]["dev_f"] < 1e-2
    # the selfcheck command on the same inputs
    q = _run(["selfcheck", rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat], cwd=str(tmp_path))
    assert q.returncode == 0 and json.loads(q.stdout.strip().splitlines()[-1])["ok"], q.stdout + q.stderr
    model.close()


def test_every_flag_at_once(tmp_path):
    """dock and refine with every analysis flag and every output file in one run each, on the 24 + 16 residue synthetic pair and a
    family-1 checkpoint (the distogram head): the line holds every analysis, every named file is written, and the line equals the
    drivers called in process with the same keywords."""
    from dfmdock_amd import cli, driver, engine, pairpot, restraints as RS
    from dfmdock_amd.weights import HParams, load_lightning_checkpoint, pack_blob
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), complex_for("fwd2_syn_24_16"), "A" * 24, "G" * 16)
    ck = str(tmp_path / "pair.ckpt")
    write_ckpt(ck, hp=HParams(family=1, mask_dist=20.0), seed=1)
    rng = np.random.default_rng(3)
    pot = str(tmp_path / "pot.npz")
    pairpot.save(pot, np.linspace(0.0, 15.0, 31).astype(np.float32), rng.uniform(-1.0, 1.0, (3, 3, 30)).astype(np.float32), ["@C", "@N", "*"])
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    name = lambda k: f"{k[0]}:{k[1]}{k[2].strip()}"
    groups = RS.native_contact_groups(rec["bb_coords"], lig["bb_coords"], 3, seed=0)
    assert len(groups) == 3
    (tmp_path / "r.txt").write_text("".join(f"{name(rec['residues'][g.pairs[0][0]])}  {name(lig['residues'][g.pairs[0][1]])}  8.0\n" for g in groups))
    files = {"--contact-map": "cmap.npz", "--write-restraints": "cons.txt", "--distogram-map": "dmap.npz", "--distogram-restraints": "dist.txt",
             "--clash-residues": "clash.txt", "--interface-residues": "iface.txt", "--energy-residues": "energy.txt", "--pairpot-residues": "pp.txt",
             "--pair-counts": "counts.npz", "--contact-residues": "contacts.txt", "--hbond-residues": "hb.txt", "--json": "res.json", "--out": "out.pdb"}
    flags = ["--consensus", "--consensus-top", "0.75", "--restraint-top", "5", "--restraint-upper", "9.0", "--distogram", "--distogram-t", "0.002",
             "--clash-screen", "--clash-filter", "--clash-cutoff", "2.5", "--contact-cutoff", "5.5", "--bsa", "--min-bsa", "1.0", "--probe", "1.4",
             "--sphere-points", "128", "--interface-energy", "--ie-weights", "0.2", "1.0", "0.4", "--ie-cutoff", "9.0", "--pair-potential", pot,
             "--affinity", "--affinity-cutoff", "6.0", "--hbonds", "--hbond-cutoff", "3.4", "--hbond-angle", "95", "--salt-cutoff", "4.5",
             "--native", rec_pdb, lig_pdb]
    base = ["--ckpt", ck, "--features", feat, "--num-samples", "6", "--num-steps", "8", "--max-batch", "4", "--seed", "5"]
    kw = dict(consensus=True, consensus_top=0.75, distogram=True, distogram_t=0.002, distogram_maps=True, clash_screen=True, clash_filter=True,
              clash_cutoff=2.5, contact_cutoff=5.5, bsa=True, min_bsa=1.0, probe=1.4, sphere_points=128, interface_energy=True,
              ie_weights=[0.2, 1.0, 0.4], ie_cutoff=9.0, pair_potential=pot, affinity=True, affinity_cutoff=6.0, hbonds=True, hbond_cutoff=3.4,
              hbond_angle=95.0, salt_cutoff=4.5, native=cli.load_native([rec_pdb, lig_pdb]), num_samples=6, num_steps=8, max_batch=4, seed=5, out_pdb=None)
    objects = ["consensus", "sterics", "interface_energy", "pair_potential", "affinity", "bsa", "bsa_rec", "bsa_lig", "probe", "sphere_points", "min_bsa",
               "n_hbond", "hb_bb_bb", "hb_bb_sc", "hb_sc_sc", "n_salt", "n_unsat", "metrics"]
    written = ["contact_map", "restraints_written", "restraints_written_n", "distogram_map", "distogram_restraints", "distogram_restraints_n",
               "clash_residues", "interface_residues", "energy_residues", "pairpot_residues", "pair_counts", "contact_residues", "hbond_residues"]
    engine.set_device(0)
    sd, hp = load_lightning_checkpoint(ck)
    model = engine.Model(pack_blob(sd, hp), hp)
    plain = lambda v: json.loads(json.dumps(v))
    for cmd, own, own_kw, own_keys in (
            ("dock", ["--top-k", "2", "--refine-t", "0.1", "--refine-samples", "2", "--restraints", str(tmp_path / "r.txt")],
             dict(top_k=2, refine_t=0.1, refine_samples=2, restraints=groups),
             ["models", "cluster_radius", "cluster_rule", "refine_t", "refine_samples", "restraints", "restraints_satisfied", "restraint_energy", "restraint_rank",
              "bsa_dropped"]),
            ("refine", [], {}, ["t_begin", "perturb", "start_metrics"])):
        d = tmp_path / cmd
        d.mkdir()
        p = _run([cmd, rec_pdb, lig_pdb] + base + own + flags + [a for f, n in files.items() for a in (f, str(d / n))], cwd=str(d))
        assert p.returncode == 0, p.stdout + p.stderr
        line = json.loads(p.stdout.strip().splitlines()[-1])
        print(cmd, sorted(line))
        assert set(line) == set(["energy", "output", "num_samples", "precision", "rot_update", "tr_update", "selfcheck_ok", "index", "dist_nll",
                                 "dist_nll_near", "exp_contacts", "dist_rank", "distogram_t"] + objects + written + own_keys), sorted(line)
        for n in files.values():
            assert (d / n).exists(), n
        ref = (driver.dock_pair if cmd == "dock" else driver.refine_pair)(model, rec, lig, rec_x, lig_x, **kw, **own_kw)
        assert line["energy"] == ref["energy"] and line["index"] == ref["index"]
        np.testing.assert_array_equal(np.float32(line["rot_update"]), ref["rot_update"])
        for k in objects:
            assert line[k] == plain(ref[k]), k
        assert {k: line[k] for k in ("dist_nll", "dist_nll_near", "exp_contacts")} == plain({k: ref["distogram"][k] for k in ("dist_nll", "dist_nll_near", "exp_contacts")})
        assert line["dist_rank"] == ref["distogram"]["rank"] and line["distogram_t"] == 0.002
        if cmd == "dock":
            assert len(line["models"]) == len(ref["models"]) >= 1 and (d / "out_1.pdb").exists() and (d / "hb_1.txt").exists()
            for m, r in zip(line["models"], ref["models"]):
                assert {k: v for k, v in m.items() if k != "path"} == plain(r)
            assert line["restraints"] == 3 and line["restraints_satisfied"] == ref["restraints_satisfied"] and line["bsa_dropped"] == ref["bsa_dropped"]
        else:
            assert line["start_metrics"] == plain(ref["start_metrics"]) and line["t_begin"] == 0.1
    model.close()


def test_sweep_db5_directory(tmp_path):
    cx, rs, ls = golden_7cei()
    d = tmp_path / "db5"
    d.mkdir()
    write_db5_pt(str(d / "7CEI.pt"), "7CEI", cx, rs, ls)
    small = complex_for("fwd_syn_24_16")
    write_db5_pt(str(d / "SYN1.pt"), "SYN1", small, "A" * 24, "G" * 16)
    (d / "test.txt").write_text("7CEI\nSYN1\n1N2C\n")
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    p = _run(["sweep", "--db5", str(d), "--ckpt", ck, "--num-samples", "6", "--num-steps", "8", "--out-csv", str(tmp_path / "r.csv"),
              "--summary", str(tmp_path / "s.json")], cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "1N2C.pt is listed but missing" in p.stderr and p.stderr.count("selfcheck ") >= 2
    assert "success rate over 2 complexes" in p.stdout and "DockQ >= 0.23" in p.stdout
    rows = list(csv.DictReader(open(tmp_path / "r.csv")))
    assert len(rows) == 12 and list(rows[0]) == ["id", "index", "c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ", "energy", "num_clashes"]
    s = json.load(open(tmp_path / "s.json"))
    assert set(s["complexes"]) == {"7CEI", "SYN1"} and len(s["selfcheck"]) == 2 and all(c["selfcheck"]["ok"] for c in s["selfcheck"])
    assert 0 <= s["success"]["acceptable"]["top1"] <= s["success"]["acceptable"]["best_of_n"] <= 1
