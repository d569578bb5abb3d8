"""Pose clustering on the GPU (dfm_pose_rmsd, dfm_pose_cluster) against the float64 definition in dfmdock_amd/cluster.py, and the
clustering options of dock_pair / run_set / the command line end to end.

Gates: RMSD within 1e-4 A + 2e-4 * rmsd of float64; the matrix bitwise symmetric and bitwise permuted with the poses; clusters EXACTLY the
definition's, on radii that no float64 pair lies within 1e-2 A of; the rebuilt backbone within 1e-2 A of the sampler's own lig_pos.
"""
import csv
import json
import os
import subprocess
import sys
import textwrap
import threading

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_ckpt, write_db5_pt, write_pair
from conftest import ROOT, complex_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def _rigid(lig, B, rng, spread=4.0):
    """B rigid moves of a real ligand: a random rotation about its CA centroid and an N(0, spread^2) shift."""
    from dfmdock_amd.pdbio import axis_angle_to_matrix
    lig = np.asarray(lig, np.float64)
    c = lig[:, 1].mean(0)
    out = np.empty((B,) + lig.shape, np.float32)
    for b in range(B):
        aa = rng.standard_normal(3)
        aa *= rng.uniform(0, 0.6) / np.linalg.norm(aa)
        out[b] = (lig - c) @ axis_angle_to_matrix(aa).T + c + spread * rng.standard_normal(3)
    return out


def _ligand(L, seed=0):
    """A real ligand backbone (7CEI) cut or tiled to L residues."""
    lig = np.asarray(golden_7cei()[0]["lig_pos"], np.float32)
    reps = -(-L // lig.shape[0])
    tiled = np.concatenate([lig + np.float32(30.0 * k) for k in range(reps)], 0)
    return tiled[:L]


def _safe_radius(r64, candidates):
    """The first radius no float64 pair lies within 1e-2 A of (asserted: the exact comparison depends on it)."""
    off = r64[np.triu_indices(r64.shape[0], 1)]
    for rad in candidates:
        if off.size == 0 or np.abs(off - rad).min() > 1e-2:
            return rad
    raise AssertionError("no radius keeps 1e-2 A away from every pair")


@pytest.mark.parametrize("B,L", [(1, 16), (2, 300), (31, 1000), (33, 57), (257, 300), (4099, 16)])
def test_rmsd_vs_float64(B, L, model):
    from dfmdock_amd.cluster import pose_rmsd
    rng = np.random.default_rng(B + L)
    rigid = _rigid(_ligand(L), B, rng)
    noisy = (rng.normal(0, 20, (B, L, 3, 3)) + rng.normal(0, 0.5, (1, L, 3, 3))).astype(np.float32)      # non-rigid
    worst = 0.0
    for x in (rigid, noisy):
        got = model.pose_rmsd(x)
        want = pose_rmsd(x)
        err = np.abs(got - want)
        worst = max(worst, float((err / (1e-4 + 2e-4 * want)).max()))
        assert (err <= 1e-4 + 2e-4 * want).all(), float(err.max())
        assert (got == got.T).all() and (np.diag(got) == 0).all()
    if B >= 2:
        sub = np.sort(rng.choice(L, size=max(1, L // 3), replace=False))
        got = model.pose_rmsd(rigid, residues=sub)
        want = pose_rmsd(rigid, residues=sub)
        assert (np.abs(got - want) <= 1e-4 + 2e-4 * want).all()
    print(f"B={B} L={L}: worst error / gate {worst:.3f}")


def test_rmsd_bitwise_symmetric_permuted_and_batch_free(model):
    rng = np.random.default_rng(7)
    x = _rigid(_ligand(120), 300, rng)
    r = model.pose_rmsd(x)
    assert np.array_equal(r, r.T)
    perm = rng.permutation(300)
    rp = model.pose_rmsd(x[perm])
    assert np.array_equal(rp, r[np.ix_(perm, perm)])      # the same bits wherever a pair's tile falls
    sub = model.pose_rmsd(x[:65])                           # and whatever B is
    assert np.array_equal(sub, r[:65, :65])
    assert np.array_equal(model.pose_rmsd(x), r)


@pytest.mark.parametrize("rule", ["energy", "size"])
@pytest.mark.parametrize("B,L", [(33, 40), (257, 60), (1000, 20)])
def test_cluster_equals_the_definition(rule, B, L, model):
    from dfmdock_amd.cluster import cluster_adjacency, pose_rmsd
    rng = np.random.default_rng(B * 3 + L)
    lig = _ligand(L)
    # basins: a few rigid moves of the ligand, each pose shifted from its basin by a lattice vector in {-2..2}^3 A, so that two poses of a
    # basin are sqrt(n) A apart (integer n: clear gaps for the radius, and many exact ties in the neighbour counts)
    basins = _rigid(lig, 6, rng, spread=25.0)
    x = np.stack([basins[rng.integers(6)] + rng.integers(-2, 3, 3).astype(np.float64) for _ in range(B)]).astype(np.float32)
    key = rng.normal(size=B).astype(np.float32)
    key[rng.random(B) < 0.1] = np.nan
    key[rng.random(B) < 0.1] = 0.5
    sub = np.sort(rng.choice(L, size=L // 2, replace=False)).astype(np.int32)
    for residues in (None, sub):
        r64 = pose_rmsd(x, residues)
        rad = _safe_radius(r64, [2.1, 2.55, 1.55, 3.08, 1.2])
        for kw in ({}, {"key": key}, {"key": key, "max_clusters": 4}):
            want = cluster_adjacency(r64 <= rad, kw.get("key"), rule, kw.get("max_clusters"))
            got = model.pose_cluster(x, rad, rule=rule, residues=residues, **kw)
            assert got["n_clusters"] == want["n_clusters"]
            assert np.array_equal(got["center"], want["center"]) and np.array_equal(got["size"], want["size"])
            assert np.array_equal(got["cluster_of"], want["cluster_of"])
        assert want["n_clusters"] > 1


@pytest.mark.parametrize("rule", ["energy", "size"])
def test_a_non_finite_pose_opens_no_cluster(rule, model):
    """A pose with a NaN or an infinite coordinate among the compared residues is no pose's neighbour, itself included: keyed first or
    keyed last it opens no cluster and keeps cluster_of = -1, every cluster has a member, and when every pose is such a pose no cluster
    forms - with and without max_clusters, equal to the definition."""
    from dfmdock_amd.cluster import cluster_poses
    rng = np.random.default_rng(5)
    B, L = 70, 12
    basins = _rigid(_ligand(L), 4, rng, spread=25.0)
    x = np.stack([basins[rng.integers(4)] + rng.integers(-2, 3, 3).astype(np.float64) for _ in range(B)]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        for bad, value in ((0, np.nan), (B - 1, np.nan), (37, np.inf)):
            y = x.copy()
            y[bad, 5, 1, 2] = value
            first = np.where(np.arange(B) == bad, -1e9, rng.normal(size=B)).astype(np.float32)
            last = np.where(np.arange(B) == bad, 1e9, first).astype(np.float32)
            for key in (None, first, last):
                for kw in ({}, {"max_clusters": 3}):
                    want = cluster_poses(y, 2.55, key=key, rule=rule, **kw)
                    got = model.pose_cluster(y, 2.55, key=key, rule=rule, **kw)
                    for k in ("n_clusters", "center", "size", "cluster_of"):
                        assert np.array_equal(got[k], want[k]), (bad, k)
                    assert got["cluster_of"][bad] == -1 and bad not in got["center"] and (got["size"] >= 1).all()
                    if not kw:
                        assert got["size"].sum() == B - 1
            r = model.pose_rmsd(y)
            assert not np.isfinite(r[bad]).any() and not np.isfinite(r[:, bad]).any() and np.isfinite(np.delete(np.delete(r, bad, 0), bad, 1)).all()
            sub = [0, 1, 2, 3]      # the non-finite coordinate is in residue 5: not compared
            assert np.array_equal(model.pose_rmsd(y, residues=sub), model.pose_rmsd(x, residues=sub))
        y = x.copy()
        y[:, 0, 0, 0] = np.nan
        for kw in ({}, {"max_clusters": 3}):
            got = model.pose_cluster(y, 2.55, key=rng.normal(size=B).astype(np.float32), rule=rule, **kw)
            assert got["n_clusters"] == 0 and got["center"].size == 0 and got["size"].size == 0 and (got["cluster_of"] == -1).all()


def test_two_calls_are_bitwise_the_same(model):
    rng = np.random.default_rng(11)
    x = _rigid(_ligand(80), 700, rng)
    key = rng.normal(size=700).astype(np.float32)
    for rule in ("energy", "size"):
        a = model.pose_cluster(x, 3.0, key=key, rule=rule)
        b = model.pose_cluster(x, 3.0, key=key, rule=rule)
        for k in a:
            assert np.array_equal(a[k], b[k])


def test_65536_poses(model):
    """B = 65 536 (the limit; a 512 MB bitmask): tight blobs of unequal size, far apart, so the definition's clusters are the blobs.
    Counts and centres against the blob-level definition; a sampled subset of poses against their centre in float64."""
    from dfmdock_amd import engine
    from dfmdock_amd.cluster import pose_rmsd, rank_order
    B, L, G = 65536, 4, 48
    rng = np.random.default_rng(3)
    blob_of = np.sort(rng.integers(0, G, B))
    blob_of[:G] = np.arange(G)
    blob_of = np.sort(blob_of)
    base = rng.normal(0, 3, (L, 3, 3))
    x = (base[None] + 100.0 * np.stack([np.arange(G), np.zeros(G), np.zeros(G)], 1)[blob_of][:, None, None]
         + rng.normal(0, 0.2, (B, 1, 1, 3))).astype(np.float32)
    key = rng.normal(size=B).astype(np.float32)
    order = rank_order(key, B)
    first = {}
    for i in order:
        first.setdefault(int(blob_of[i]), int(i))
    blobs_by_key = sorted(first, key=lambda g: np.nonzero(order == first[g])[0][0])
    e = model.pose_cluster(x, 4.0, key=key, rule="energy")
    assert e["n_clusters"] == G
    assert list(e["center"]) == [first[g] for g in blobs_by_key]
    assert list(e["size"]) == [int((blob_of == g).sum()) for g in blobs_by_key]
    sizes = np.bincount(blob_of, minlength=G)
    s = model.pose_cluster(x, 4.0, key=key, rule="size", max_clusters=5)
    want = sorted(range(G), key=lambda g: (-sizes[g], np.nonzero(order == first[g])[0][0]))[:5]
    assert s["n_clusters"] == 5 and list(s["size"]) == [int(sizes[g]) for g in want]
    assert list(s["center"]) == [first[g] for g in want]
    assert (s["cluster_of"] == -1).sum() == B - sizes[want].sum()
    pick = rng.choice(B, 512, replace=False)
    cen = e["center"][e["cluster_of"][pick]]
    r = pose_rmsd(np.concatenate([x[pick], x[cen]]))[np.arange(512), 512 + np.arange(512)]
    assert (r <= 4.0).all() and (e["cluster_of"] >= 0).all()
    print("B=65536: k_pose_dist %.2f ms, clustering %.2f ms" % engine.pose_last_timing())


@pytest.mark.parametrize("family", [0, 1])
def test_rebuilt_backbone_matches_the_sampler(family, blob_pair):
    from conftest import pair_hparams
    from dfmdock_amd import engine
    from dfmdock_amd.cluster import rebuild_backbone
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    hp = pair_hparams() if family == 1 else None
    m = engine.Model(blob_pair if family == 1 else pack_blob(make_random_weights(0)), hp)
    cx = complex_for("rollout_7CEI")
    gx = engine.Complex(m, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    worst = 0.0
    for kw in ({}, {"use_clash_force": True}):
        r = gx.sample(B=16, num_steps=40, seed=2, mfma16=True, **kw)
        x = rebuild_backbone(gx.lig_pos0, r["rot_update"], r["tr_update"], family)
        d = np.linalg.norm(x.astype(np.float64) - r["lig_pos"], axis=-1).max()
        worst = max(worst, float(d))
    print(f"family {family}: worst rebuilt-vs-sampled atom deviation {worst:.2e} A over 40-step runs")
    assert worst < 1e-2
    gx.close()
    m.close()


def test_cluster_next_to_a_sampling_handle(model):
    """One clustering call on its own thread and stream while another handle samples: both results equal their solo runs bitwise."""
    from dfmdock_amd import engine
    cx = complex_for("c3_300_300")
    gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    rng = np.random.default_rng(5)
    x = _rigid(_ligand(300), 4096, rng)
    key = rng.normal(size=4096).astype(np.float32)
    solo_c = model.pose_cluster(x, 3.0, key=key, rule="size")
    solo_s = gx.sample(B=64, num_steps=8, seed=9, mfma16=True)
    out = {}

    def clus():
        out["c"] = [model.pose_cluster(x, 3.0, key=key, rule="size") for _ in range(3)]
    t = threading.Thread(target=clus)
    t.start()
    both_s = gx.sample(B=64, num_steps=8, seed=9, mfma16=True)
    t.join()
    for c in out["c"]:
        for k in solo_c:
            assert np.array_equal(c[k], solo_c[k])
    for k in ("lig_pos", "energy", "rot_update", "tr_update"):
        assert np.array_equal(both_s[k], solo_s[k])
    gx.close()


def test_bad_arguments(model):
    from dfmdock_amd import _lib as L
    import ctypes as C
    lib = L.lib()
    x = np.zeros((4, 5, 9), np.float32)
    o = np.zeros(4, np.int32)
    n = C.c_int32(0)
    f = lambda a: a.ctypes.data_as(L.F32P)
    i = lambda a: a.ctypes.data_as(L.I32P)

    def clu(B=4, Lg=5, res=None, n_res=0, radius=1.0, rule=0, maxc=4):
        return lib.dfm_pose_cluster(model._h, B, Lg, f(x), None if res is None else i(res), n_res, None, radius, rule, maxc,
                                    C.byref(n), i(o), i(o), i(o))
    assert clu() == 0
    for kw in (dict(B=0), dict(Lg=0), dict(res=np.array([0, 5], np.int32), n_res=2), dict(res=np.array([1, 1], np.int32), n_res=2),
               dict(res=np.array([-1], np.int32), n_res=1), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
               dict(radius=float("inf")), dict(rule=2), dict(rule=-1), dict(maxc=0), dict(B=65537)):
        assert clu(**kw) == -1, kw
    rm = np.zeros(16, np.float32)
    assert lib.dfm_pose_rmsd(model._h, 0, 5, f(x), None, 0, f(rm)) == -1
    assert lib.dfm_pose_rmsd(model._h, 4, 5, f(x), i(np.array([7], np.int32)), 1, f(rm)) == -1
    with pytest.raises(ValueError):
        model.pose_cluster(x, 1.0, rule="kmeans")


# ---------------------------------------------------------------------------------------------------------------------------------
def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def _coords(path):
    from dfmdock_amd import pdbio
    return np.array([a["coord"] for a in pdbio.read_pdb(str(path))])


def test_cli_dock_top_k(tmp_path):
    from dfmdock_amd import pdbio, restraints as RS
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    common = ["dock", rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--num-samples", "24", "--max-batch", "8", "--seed", "5"]
    plain = tmp_path / "plain"
    plain.mkdir()
    p0 = _run(common, cwd=str(plain))
    assert p0.returncode == 0, p0.stdout + p0.stderr
    p = _run(common + ["--top-k", "5", "--cluster-radius", "0.5"], cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    line0 = json.loads(p0.stdout.strip().splitlines()[-1])
    assert "models" not in line0 and set(line) - set(line0) == {"models", "cluster_radius", "cluster_rule"}
    assert line0["energy"] == line["energy"]
    assert (plain / "output.pdb").read_bytes() == (tmp_path / "output.pdb").read_bytes()      # output.pdb does not change
    assert not any(f.startswith("output_") for f in os.listdir(plain))
    ms = line["models"]
    assert [m["rank"] for m in ms] == [1, 2, 3, 4, 5] and all(os.path.exists(m["path"]) for m in ms)
    assert sum(m["cluster_size"] for m in ms) <= 24 and ms[0]["energy"] == line["energy"]
    assert [m["energy"] for m in ms] == sorted(m["energy"] for m in ms)      # leader clustering in energy order
    assert (tmp_path / "output_1.pdb").read_bytes() == (tmp_path / "output.pdb").read_bytes()      # model 1 is output.pdb, atom for atom
    assert not np.array_equal(_coords(tmp_path / "output_2.pdb"), _coords(tmp_path / "output.pdb"))
    # under restraints: model 1 is the pose restraint ranking kept
    rec = pdbio.backbone_from_atoms(pdbio.read_pdb(rec_pdb))
    lig = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))
    name = lambda k: f"{k[0]}:{k[1]}{k[2].strip()}"
    lines = [f"{name(rec['residues'][i])}  {name(lig['residues'][j])}  8.0"
             for g in RS.native_contact_groups(rec["bb_coords"], lig["bb_coords"], 4, seed=0) for (i, j) in g.pairs]
    (tmp_path / "r.txt").write_text("\n".join(lines) + "\n")
    rd = tmp_path / "restrained"
    rd.mkdir()
    q = _run(common + ["--restraints", str(tmp_path / "r.txt"), "--top-k", "3"], cwd=str(rd))
    assert q.returncode == 0, q.stdout + q.stderr
    ql = json.loads(q.stdout.strip().splitlines()[-1])
    assert ql["models"][0]["index"] == ql["index"]
    assert (rd / "output_1.pdb").read_bytes() == (rd / "output.pdb").read_bytes()


def _db5_dir(tmp_path):
    cx, rs, ls = golden_7cei()
    d = tmp_path / "db5"
    d.mkdir()
    write_db5_pt(str(d / "7CEI.pt"), "7CEI", cx, rs, ls)
    write_db5_pt(str(d / "SYN1.pt"), "SYN1", complex_for("fwd_syn_24_16"), "A" * 24, "G" * 16)
    (d / "test.txt").write_text("7CEI\nSYN1\n")
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    return d, ck


def test_cli_sweep_cluster_columns(tmp_path):
    from dfmdock_amd import driver, engine
    from dfmdock_amd.cluster import cluster_poses, rebuild_backbone
    from dfmdock_amd.db5 import load_db5_pt
    d, ck = _db5_dir(tmp_path)
    base = ["sweep", "--db5", str(d), "--ckpt", ck, "--num-samples", "16", "--num-steps", "8", "--max-batch", "8"]
    p0 = _run(base + ["--out-csv", str(tmp_path / "plain.csv"), "--summary", str(tmp_path / "plain.json")], cwd=str(tmp_path))
    assert p0.returncode == 0, p0.stdout + p0.stderr
    p = _run(base + ["--out-csv", str(tmp_path / "r.csv"), "--summary", str(tmp_path / "s.json"), "--cluster-radius", "4", "--top-k", "3"],
             cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    plain = list(csv.DictReader(open(tmp_path / "plain.csv")))
    rows = list(csv.DictReader(open(tmp_path / "r.csv")))
    assert list(plain[0]) == driver.CSV_FIELDS and list(rows[0]) == driver.CSV_FIELDS + ["cluster", "is_center"]
    for a, b in zip(plain, rows):
        assert all(a[k] == b[k] for k in driver.CSV_FIELDS)
    summ = json.load(open(tmp_path / "s.json"))
    assert "top3" not in json.load(open(tmp_path / "plain.json"))["success"]["acceptable"]
    for name, t in summ["success"].items():
        assert t["top1"] <= t["top3"] <= t["best_of_n"]
    assert "top3 DockQ" in p.stdout
    # the same run in process: its rows carry the same columns, which equal the definition on the backbone rebuilt from the records
    from dfmdock_amd.weights import load_lightning_checkpoint, pack_blob
    engine.set_device(0)
    sd, hp = load_lightning_checkpoint(ck)
    m = engine.Model(pack_blob(sd, hp), hp)
    cxs = []
    for cid in ("7CEI", "SYN1"):
        c = load_db5_pt(str(d / f"{cid}.pt"))
        c["id"] = c.get("id") or cid
        cxs.append(c)
    got, ranked = driver.run_set(m, cxs, num_samples=16, num_steps=8, max_batch=8, cluster_radius=4.0, top_k=3, log=lambda msg: None)
    m.close()
    by_csv = {(r["id"], r["index"]): (int(r["cluster"]), int(r["is_center"])) for r in rows}
    assert {(r["id"], r["index"]): (r["cluster"], r["is_center"]) for r in got} == by_csv
    rng = np.random.default_rng(0)
    rots = [rng.integers(0, 2 ** 31) for _ in cxs]
    for ci, c in enumerate(cxs):
        rec = ranked[ci][np.argsort(ranked[ci][:, 1])]
        lig0 = driver.input_pose(c, rots[ci], True)[1]
        want = cluster_poses(rebuild_backbone(lig0, rec[:, 4:7], rec[:, 7:10]), 4.0, key=rec[:, 2], max_clusters=3)
        assert [by_csv[(c["id"], str(t))][0] for t in range(16)] == list(want["cluster_of"])
        assert sorted(t for t in range(16) if by_csv[(c["id"], str(t))][1]) == sorted(want["center"])
        assert want["n_clusters"] >= 1


RUN_SET_WORKER = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, {root!r})
    import torch.distributed as dist
    from dfmdock_amd import distributed as D, driver, engine
    from dfmdock_amd.synthetic import make_complex
    from dfmdock_amd.weights import make_random_weights, pack_blob
    rank, local, world = D.dist_env()
    if world > 1:
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    cxs = []
    for k, (R, L) in enumerate({shapes!r}):
        c = make_complex(R, L, seed=20 + k)
        c.update(id=f"SYN{{k}}", rec_seq="A" * R, lig_seq="G" * L)
        cxs.append(c)
    rows, _ = driver.run_set(model, cxs, num_samples=12, num_steps=4, seed=3, out_csv=os.path.join({out!r}, "set.csv"), max_batch=4,
                             cluster_radius=6.0, top_k=4)
    json.dump([[r["id"], r["index"], r["cluster"], r["is_center"]] for r in rows], open(os.path.join({out!r}, f"rank{{rank}}.json"), "w"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
""")


@pytest.mark.parametrize("shapes", [[(30, 22), (70, 41), (41, 17), (25, 25)], [(70, 41)]], ids=["sharded", "split"])
def test_run_set_two_ranks_equal_one_rank(tmp_path, shapes):
    port = 29600 + (os.getpid() % 250) + len(shapes)
    results = {}
    for world in (1, 2):
        out = tmp_path / f"w{world}"
        out.mkdir()
        script = out / "worker.py"
        script.write_text(RUN_SET_WORKER.format(root=ROOT, out=str(out), shapes=shapes))
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs = [p.communicate(timeout=600)[0].decode() for p in procs]
        assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
        per_rank = [json.load(open(out / f"rank{r}.json")) for r in range(world)]
        assert all(per_rank)      # every rank's rows carry the columns
        results[world] = {(i, x): (c, s) for part in per_rank for i, x, c, s in part}
        csv_rows = list(csv.DictReader(open(out / "set.csv")))
        assert {(r["id"], r["index"]): (int(r["cluster"]), int(r["is_center"])) for r in csv_rows} == results[world]
    assert results[1] == results[2]
    assert any(s for c, s in results[1].values())
