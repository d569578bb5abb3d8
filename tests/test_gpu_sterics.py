"""All-atom clash / contact screen on the GPU (dfm_atoms_create, dfm_pose_sterics, kernels_sterics.hip) against its float64 definition
dfmdock_amd/sterics.py, and through the drivers and the command line.

Counts are integers and min_dist a minimum.  A pair whose float64 distance is within 1e-3 A of a cutoff (the border tests/test_gpu_metrics.py
and tests/test_gpu_consensus.py grant) may fall either way; such pairs may be at most 0.5 % of the pairs below that cutoff.  On every
ligand atom without a border pair the per-atom counts must equal the definition exactly, elsewhere differ by at most the atom's number
of border pairs; the per-pose counts must equal the sums of the call's own per-atom counts; min_dist must be within 1e-9 A of the
definition unless the pose's minimum is itself a border pair of the contact cutoff."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, complex_for, db5_complex, db5_ids

pytestmark = pytest.mark.gpu

BORDER = 1e-3
KEYS = ("n_clash", "n_contact", "min_dist")
ATOM_KEYS = ("lig_clash", "lig_contact")


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def check_against_definition(model, rec, lig, center, rot, tr, clash=3.0, contact=5.0, label="", chunk_poses=0):
    """One handle, one call with per-atom output, against the definition; returns (pairs, clash pairs, contact pairs, border pairs of the
    clash cutoff, of the contact cutoff, poses without a contact, largest clash count, result)."""
    from dfmdock_amd import sterics as ST
    rec, lig = np.asarray(rec, np.float32).reshape(-1, 3), np.asarray(lig, np.float32).reshape(-1, 3)
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    P, Ar, Al = rot.shape[0], rec.shape[0], lig.shape[0]
    cc, ct = float(np.float32(clash)), float(np.float32(contact))
    with model.atoms(rec, lig, center, clash, contact) as at:
        got = at.sterics(rot, tr, per_atom=True, chunk_poses=chunk_poses)
    assert got["lig_clash"].shape == (P, Al) and got["lig_clash"].dtype == np.int32 and got["min_dist"].dtype == np.float64
    assert np.array_equal(got["n_clash"], got["lig_clash"].sum(1)) and np.array_equal(got["n_contact"], got["lig_contact"].sum(1)), label
    n = np.zeros(5, np.int64)
    for p in range(P):
        a, _, d = ST.near_pairs(rec, ST.pose_atoms(lig, center, rot[p], tr[p]), ct + BORDER)
        is_t, is_c = d < ct, d < cc
        bt, bc = np.abs(d - ct) < BORDER, np.abs(d - cc) < BORDER
        n += [is_c.sum(), is_t.sum(), bc.sum(), bt.sum(), is_t.sum() == 0]
        for key, want, border in (("lig_clash", is_c, bc), ("lig_contact", is_t, bt)):
            w, b = np.bincount(a[want], minlength=Al), np.bincount(a[border], minlength=Al)
            off = np.abs(got[key][p] - w)
            assert (off <= b).all(), (label, key, p, np.nonzero(off > b)[0][:5].tolist(), got[key][p][off > b][:5].tolist(), w[off > b][:5].tolist())
        want_min = d[is_t].min() if is_t.any() else np.inf
        g = got["min_dist"][p]
        if is_t.any() and not bt[is_t][np.argmin(d[is_t])]:
            assert abs(g - want_min) <= 1e-9, (label, "min_dist", p, g, want_min)
        elif not is_t.any() and not bt.any():
            assert g == np.inf, (label, "min_dist", p, g)
        else:      # the minimum is a border pair, or a border pair is all there is
            assert g == np.inf or abs(g - ct) < BORDER + 1e-9 or abs(g - want_min) <= 1e-9, (label, "min_dist", p, g, want_min)
    print(f"{label}: P {P} Ar {Ar} Al {Al} clash {n[0]} contact {n[1]} border {n[2]} / {n[3]} empty poses {n[4]} max clash {got['n_clash'].max()}")
    return P * Ar * Al, n[0], n[1], n[2], n[3], n[4], int(got["n_clash"].max()), got


def db5_poses(rng, P=16):
    """The issue's recipe: per pose an axis, an angle in [0, 0.3) and a translation of 2 A per axis; pose 0 is the identity (its draws
    are still consumed)."""
    rot, tr = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
    for p in range(P):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        ang = rng.uniform(0, 0.3)
        t = 2.0 * rng.standard_normal(3)
        if p == 0:
            ang, t = 0.0, np.zeros(3)
        rot[p], tr[p] = (ax * ang).astype(np.float32), t.astype(np.float32)
    return rot, tr


def five_atoms(bb):
    from dfmdock_amd import pdbio
    return pdbio.full_backbone(bb).reshape(-1, 3)


def ca_center(bb):
    return np.asarray(bb, np.float64)[:, 1].mean(0).astype(np.float32)


def test_parity_with_the_definition_on_db5(model):
    """Gate 1.  N, CA, C, O, CB of the 24 DB5 backbones, 16 seeded poses each from one default_rng(0) stream, cutoffs 3.0 and 5.0.  The
    definition alone gives 384 poses, 364 431 200 atom pairs, 12 346 clash pairs and 83 223 contact pairs, 32 and 153 border pairs
    (0.26 % and 0.18 %), 5 poses without a contact and at most 322 clashes in one pose (counted on the CPU)."""
    rng = np.random.default_rng(0)
    tot, most = np.zeros(6, np.int64), 0
    for cid in db5_ids():
        c = db5_complex(cid)
        rot, tr = db5_poses(rng)
        r = check_against_definition(model, five_atoms(c["rec_pos"]), five_atoms(c["lig_pos"]), ca_center(c["lig_pos"]), rot, tr, label=cid)
        tot += r[:6]
        most = max(most, r[6])
    print(f"atom pairs {tot[0]}, clash {tot[1]}, contact {tot[2]}, border {tot[3]} / {tot[4]}, poses without a contact {tot[5]}, most clashes {most}")
    assert tot[0] == 364431200 and tot[1] == 12346 and tot[2] == 83223
    assert tot[3] <= 0.005 * tot[1] and tot[4] <= 0.005 * tot[2]


def _ensemble_7cei(P=96, seed=1):
    cx = complex_for("fwd_7CEI_p0")
    rng = np.random.default_rng(seed)
    rot = (0.2 * rng.standard_normal((P, 3))).astype(np.float32)
    tr = (2.0 * rng.standard_normal((P, 3))).astype(np.float32)
    return five_atoms(cx["rec_pos"]), five_atoms(cx["lig_pos"]), ca_center(cx["lig_pos"]), rot, tr


def _same(a, b, keys, label=""):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (label, k)


def test_invariances_are_exact(model):
    """Gate 2."""
    from dfmdock_amd import _lib as L
    rec, lig, cen, rot, tr = _ensemble_7cei()
    with model.atoms(rec, lig, cen) as at:
        full = at.sterics(rot, tr, per_atom=True)
        assert full["n_clash"].sum() > 0 and (full["n_contact"] > 0).sum() > 48
        # three split calls
        parts = [at.sterics(rot[lo:hi], tr[lo:hi], per_atom=True) for lo, hi in ((0, 31), (31, 32), (32, 96))]
        _same(full, {k: np.concatenate([q[k] for q in parts]) for k in KEYS + ATOM_KEYS}, KEYS + ATOM_KEYS, "split")
        # a permuted call, un-permuted
        perm = np.random.default_rng(2).permutation(96)
        op = at.sterics(rot[perm], tr[perm], per_atom=True)
        _same({k: full[k][perm] for k in KEYS + ATOM_KEYS}, op, KEYS + ATOM_KEYS, "permuted")
        for cp in (1, 7, 96):
            _same(full, at.sterics(rot, tr, per_atom=True, chunk_poses=cp), KEYS + ATOM_KEYS, f"chunk {cp}")
            _same(full, at.sterics(rot, tr, chunk_poses=cp), KEYS, f"chunk {cp}, no per-atom output")
        _same(full, at.sterics(rot, tr), KEYS, "no per-atom output")
        # any subset of the output pointers NULL
        types = {"n_clash": C.c_int32, "n_contact": C.c_int32, "min_dist": C.c_double, "lig_clash": C.c_int32, "lig_contact": C.c_int32}
        f = lambda x: x.ctypes.data_as(L.F32P)
        for mask in range(32):
            out, bufs = L.StericsOutC(), {}
            for b, (k, t) in enumerate(types.items()):
                if mask >> b & 1:
                    bufs[k] = np.full_like(full[k], 7)
                    setattr(out, k, bufs[k].ctypes.data_as(C.POINTER(t)))
            assert L.lib().dfm_pose_sterics(at._h, 96, f(rot), f(tr), C.byref(out)) == 0, mask
            _same(full, bufs, tuple(bufs), f"pointer mask {mask}")
        # two host threads on the same handle at once
        res, errs = [None, None], []

        def work(i):
            try:
                res[i] = [at.sterics(rot, tr, per_atom=True, chunk_poses=(0, 5)[i]) for _ in range(3)]
            except BaseException as e:      # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for rs in res:
            for r in rs:
                _same(full, r, KEYS + ATOM_KEYS, "threads")
        info = at.info()
        assert info["cell_edge"] == 5.0 and info["n_cells"] >= 8 and 1 <= info["max_cell_atoms"] <= rec.shape[0]
    from dfmdock_amd import engine
    cp, kn = engine.sterics_last_timing()
    assert cp > 0 and kn > 0


def test_small_shapes(model):
    """Gate 3: sizes and placements at which the kernel takes another path, each against the definition."""
    rng = np.random.default_rng(5)
    zero = np.zeros(3, np.float32)
    poses = lambda P, s_rot=0.5, s_tr=1.5: ((s_rot * rng.standard_normal((P, 3))).astype(np.float32), (s_tr * rng.standard_normal((P, 3))).astype(np.float32))
    # Al around the block size, one receptor atom
    for Al in (1, 63, 64, 65, 130):
        lig = (3.0 * rng.standard_normal((Al, 3))).astype(np.float32)
        rot, tr = poses(6)
        r = check_against_definition(model, np.array([[0.5, -0.25, 1.0]], np.float32), lig, lig.mean(0), rot, tr, label=f"Ar 1, Al {Al}")
        assert r[2] > 0 or Al == 1
    # every receptor atom in one cell; 200 atoms at one point: a cell holds more than a wave
    lig = (4.0 * rng.standard_normal((90, 3))).astype(np.float32)
    rot, tr = poses(5)
    one_cell = (1.2 * rng.random((150, 3))).astype(np.float32) + np.float32(1.0)
    r = check_against_definition(model, one_cell, lig, zero, rot, tr, label="one cell, 150 atoms")
    assert r[2] > 1000
    point = np.tile(np.array([[1.0, 2.0, -0.5]], np.float32), (200, 1))
    r = check_against_definition(model, point, lig, zero, rot, tr, label="200 atoms at one point")
    assert r[2] >= 200 and r[2] % 200 == 0
    # a ligand wholly outside the grid box by more than the cutoff: nothing, +inf
    rec = (8.0 * rng.random((300, 3))).astype(np.float32)
    lig = (2.0 * rng.random((70, 3))).astype(np.float32)
    far = np.array([[30.0, 0, 0], [0, -25.0, 0], [0, 0, 14.1], [-7.2, -7.2, -7.2]], np.float32)
    r = check_against_definition(model, rec, lig, lig.mean(0), np.zeros((4, 3), np.float32), far, label="outside by more than the cutoff")
    assert r[2] == 0 and (r[7]["n_contact"] == 0).all() and np.isinf(r[7]["min_dist"]).all() and not r[7]["lig_contact"].any()
    # outside by less than the cutoff on the low side: negative cell coordinates before the clamp
    low = np.array([[-4.5, 3.0, 3.0], [3.0, -5.5, 3.0], [3.0, 3.0, -6.0], [-3.0, -3.0, -3.0]], np.float32)
    r = check_against_definition(model, rec, lig, lig.mean(0), np.zeros((4, 3), np.float32), low, label="outside on the low side by less than the cutoff")
    assert r[2] > 0
    # a ligand atom exactly on a cell face (the grid's origin is the receptor's low corner, the edge 5)
    grid = np.array([[0, 0, 0], [10, 10, 10], [2, 3, 4], [5.5, 4.5, 6.0], [9, 1, 1], [4.0, 6.0, 9.0]], np.float32)
    face = np.array([[5, 5, 5], [10, 5, 0], [0, 0, 0], [5, 2.5, 7.5], [10, 10, 10], [15, 5, 5]], np.float32)
    r = check_against_definition(model, grid, face, zero, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), label="atoms on cell faces")
    assert r[2] > 0
    # one long line of receptor atoms: two grid dimensions are 1
    line = np.zeros((400, 3), np.float32)
    line[:, 0] = np.arange(400) * np.float32(1.5)
    lig = (3.0 * rng.standard_normal((100, 3))).astype(np.float32) + np.array([300.0, 0, 0], np.float32)
    rot, tr = poses(6, 0.5, 3.0)
    r = check_against_definition(model, line, lig, lig.mean(0), rot, tr, label="receptor on a line")
    assert r[2] > 0
    # P = 1; equal cutoffs; a deep overlap
    cx = complex_for("fwd_7CEI_p0")
    rec, lig = five_atoms(cx["rec_pos"]), five_atoms(cx["lig_pos"])
    cen = ca_center(cx["lig_pos"])
    rot, tr = poses(4, 0.2, 1.0)
    assert check_against_definition(model, rec, lig, cen, rot[:1], tr[:1], label="P = 1")[0] == rec.shape[0] * lig.shape[0]
    r = check_against_definition(model, rec, lig, cen, rot, tr, clash=4.0, contact=4.0, label="contact_cutoff == clash_cutoff")
    assert r[2] > 0 and np.array_equal(r[7]["n_clash"], r[7]["n_contact"]) and np.array_equal(r[7]["lig_clash"], r[7]["lig_contact"])
    onto = (rec.astype(np.float64).mean(0) - lig.astype(np.float64).mean(0)).astype(np.float32)
    r = check_against_definition(model, rec, lig, cen, rot, onto[None] + np.float32(0.3) * tr, label="deep overlap")
    assert r[6] > 1000


def test_nan_poses(model):
    """Gate 4."""
    rec, lig, cen, rot, tr = _ensemble_7cei(8, seed=3)
    with model.atoms(rec, lig, cen) as at:
        clean = at.sterics(rot, tr, per_atom=True)
        assert (clean["n_contact"] > 0).sum() >= 4
        r2, t2 = rot.copy(), tr.copy()
        r2[2, 1] = np.nan
        t2[5, 0] = np.nan
        dirty = at.sterics(r2, t2, per_atom=True)
    for p in (2, 5):
        assert dirty["n_clash"][p] == 0 and dirty["n_contact"][p] == 0 and dirty["min_dist"][p] == np.inf
        assert not dirty["lig_clash"][p].any() and not dirty["lig_contact"][p].any()
    keep = np.ones(8, bool)
    keep[[2, 5]] = False
    _same({k: clean[k][keep] for k in KEYS + ATOM_KEYS}, {k: dirty[k][keep] for k in KEYS + ATOM_KEYS}, KEYS + ATOM_KEYS)
    from dfmdock_amd import sterics as ST
    want = ST.sterics(rec, lig, cen, r2, t2)
    assert np.array_equal(want["n_contact"][[2, 5]], [0, 0]) and np.isinf(want["min_dist"][[2, 5]]).all()


def test_invalid_arguments(model):
    """Gate 5: DFM_E_INVALID / NULL, dfm_last_error set, nothing enqueued; create / destroy leaves the block cache's accounting sane."""
    from dfmdock_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(4)
    rec, lig = (6.0 * rng.random((40, 3))).astype(np.float32), (6.0 * rng.random((30, 3))).astype(np.float32)
    cen = lig.mean(0)
    f = lambda x: x.ctypes.data_as(L.F32P)
    prm = lambda a=3.0, b=5.0, c=0: C.byref(L.StericsParamsC(a, b, c))
    nan_rec, nan_lig, inf_cen = rec.copy(), lig.copy(), cen.copy()
    nan_rec[7, 1], nan_lig[3, 2], inf_cen[0] = np.nan, np.inf, np.inf
    wide = rec.copy()
    wide[0] = 2000.0      # 400^3 cells of 5 A > 2^24
    h = model._h
    cases = [((None, 40, f(rec), 30, f(lig), f(cen), prm()), "m is NULL"), ((h, 40, None, 30, f(lig), f(cen), prm()), "rec_atoms is NULL"),
             ((h, 40, f(rec), 30, None, f(cen), prm()), "lig_atoms is NULL"), ((h, 40, f(rec), 30, f(lig), None, prm()), "center is NULL"),
             ((h, 0, f(rec), 30, f(lig), f(cen), prm()), "Ar >= 1"), ((h, 40, f(rec), 0, f(lig), f(cen), prm()), "Al >= 1"),
             ((h, (1 << 24) + 1, f(rec), 30, f(lig), f(cen), prm()), "exceeds 2^24 atoms"),
             ((h, 40, f(rec), (1 << 24) + 1, f(lig), f(cen), prm()), "exceeds 2^24 atoms"),
             ((h, 40, f(rec), 30, f(lig), f(cen), prm(float("nan"))), "cutoffs must be finite and > 0"),
             ((h, 40, f(rec), 30, f(lig), f(cen), prm(3.0, float("inf"))), "cutoffs must be finite and > 0"),
             ((h, 40, f(rec), 30, f(lig), f(cen), prm(0.0)), "cutoffs must be finite and > 0"),
             ((h, 40, f(rec), 30, f(lig), f(cen), prm(3.0, -5.0)), "cutoffs must be finite and > 0"),
             ((h, 40, f(rec), 30, f(lig), f(cen), prm(5.0, 3.0)), "contact_cutoff must be >= clash_cutoff"),
             ((h, 40, f(rec), 30, f(lig), f(cen), prm(3.0, 5.0, -1)), "chunk_poses must be >= 0"),
             ((h, 40, f(nan_rec), 30, f(lig), f(cen), prm()), "rec_atoms: atom 7 is not finite"),
             ((h, 40, f(rec), 30, f(nan_lig), f(cen), prm()), "lig_atoms: atom 3 is not finite"),
             ((h, 40, f(rec), 30, f(lig), f(inf_cen), prm()), "center is not finite"),
             ((h, 40, f(wide), 30, f(lig), f(cen), prm()), "more than 2^24 cells")]
    for args, word in cases:
        assert lib.dfm_atoms_create(*args) is None, word
        msg = lib.dfm_last_error().decode()
        print(word, "->", msg)
        assert word in msg, (word, msg)
    lib.dfm_trim_cache(-1)
    for _ in range(20):
        a = lib.dfm_atoms_create(h, 40, f(rec), 30, f(lig), f(cen), None)      # NULL parameters: the defaults
        assert a
        lib.dfm_atoms_destroy(a)
    parked = lib.dfm_trim_cache(-1)
    assert 0 < parked <= 5 * 65536 and lib.dfm_trim_cache(-1) == 0      # five blocks of one 64 KiB granule, handed on from handle to handle
    a = lib.dfm_atoms_create(h, 40, f(rec), 30, f(lig), f(cen), prm())
    rot, tr = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out = L.StericsOutC()
    n_con = np.zeros(4, np.int32)
    out.n_contact = n_con.ctypes.data_as(L.I32P)
    o = C.byref(out)
    for args, word in [((None, 4, f(rot), f(tr), o), "a is NULL"), ((a, 4, None, f(tr), o), "rot is NULL"), ((a, 4, f(rot), None, o), "tr is NULL"),
                       ((a, 4, f(rot), f(tr), None), "out is NULL"), ((a, 0, f(rot), f(tr), o), "P >= 1")]:
        assert lib.dfm_pose_sterics(*args) == -1, word
        assert word in lib.dfm_last_error().decode(), word
    assert lib.dfm_pose_sterics_chunked(a, 4, f(rot), f(tr), -1, o) == -1 and "chunk_poses" in lib.dfm_last_error().decode()
    assert lib.dfm_sterics_last_timing(None, None) == -1 and lib.dfm_atoms_info(None, None, None, None) == -1
    assert lib.dfm_pose_sterics(a, 4, f(rot), f(tr), o) == 0 and (n_con == n_con[0]).all()      # the handle still works
    lib.dfm_atoms_destroy(a)
    lib.dfm_atoms_destroy(None)
    with pytest.raises(ValueError):
        model.atoms(rec, lig, cen, clash_cutoff=6.0)
    with pytest.raises(ValueError):
        model.atoms(rec, lig, cen[:2])


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def _pdb_sterics(path, n_rec_atoms, clash=3.0, contact=5.0):
    """(n_clash, n_contact, border pairs of the clash cutoff, of the contact cutoff) of a written complex, re-read from disk."""
    from dfmdock_amd import pdbio
    from dfmdock_amd import sterics as ST
    atoms = pdbio.read_pdb(path)
    rec_a, lig_a = atoms[:n_rec_atoms], atoms[n_rec_atoms:]
    xyz = lambda at: np.array([at[i]["coord"] for i in ST.heavy_atoms(at)], np.float64)
    _, _, d = ST.near_pairs(xyz(rec_a), xyz(lig_a), contact + 3 * BORDER)
    return int((d < clash).sum()), int((d < contact).sum()), int((np.abs(d - clash) < 3 * BORDER).sum()), int((np.abs(d - contact) < 3 * BORDER).sum())


def test_drivers_and_cli(model, tmp_path):
    """Gate 6, on 7CEI with the seeded checkpoint.  Without the new flags `dock` writes what dock_pair without options writes; --clash-screen
    adds the fields, and the kept pose's counts equal the definition on the coordinates of the written file (each coordinate is rounded to
    1e-3 A there, so a distance moves by up to 2 sqrt(3) 5e-4 < 3e-3 A: the border of this comparison); --clash-filter never keeps a
    flagged pose of an ensemble with injected deep overlaps."""
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    from dfmdock_amd import cli, driver, pdbio
    from dfmdock_amd import sterics as ST
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    base = [rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--seed", "3", "--max-batch", "8", "--no-selfcheck", "--num-samples", "8",
            "--num-steps", "6"]
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    n_rec_atoms = len(rec["atoms"])
    pdb = lambda name: open(tmp_path / name, "rb").read()
    # the default is untouched: the CLI's files equal dock_pair's without options
    p0 = _run(["dock"] + base + ["--out", "plain.pdb"], cwd=str(tmp_path))
    assert p0.returncode == 0, p0.stdout + p0.stderr
    plain = json.loads(p0.stdout.strip().splitlines()[-1])
    d0 = driver.dock_pair(model, rec, lig, rec_x, lig_x, num_samples=8, num_steps=6, seed=3, max_batch=8, selfcheck=False,
                          out_pdb=str(tmp_path / "api.pdb"))
    assert pdb("plain.pdb") == pdb("api.pdb") and plain["energy"] == d0["energy"] and "sterics" not in plain and "sterics" not in d0
    assert b"REMARK" not in pdb("plain.pdb")
    # --clash-screen: the fields, the REMARK, nothing else moves
    p1 = _run(["dock"] + base + ["--out", "screen.pdb", "--clash-screen", "--top-k", "3", "--clash-residues", "res.txt"], cwd=str(tmp_path))
    assert p1.returncode == 0, p1.stdout + p1.stderr
    line = json.loads(p1.stdout.strip().splitlines()[-1])
    d2 = driver.dock_pair(model, rec, lig, rec_x, lig_x, num_samples=8, num_steps=6, seed=3, max_batch=8, selfcheck=False,
                          out_pdb=str(tmp_path / "topk.pdb"), top_k=3)      # the same run without the screen
    topk = {"models": [dict(m, path=driver.model_path(str(tmp_path / "topk.pdb"), m["rank"])) for m in d2["models"]]}
    assert all("sterics" not in m for m in d2["models"]) and pdb("topk.pdb") == pdb("plain.pdb")
    st = line["sterics"]
    assert set(st) == {"n_clash", "n_contact", "min_dist", "threshold", "flagged", "ensemble_mean", "ensemble_std", "clash_cutoff",
                       "contact_cutoff", "filtered", "fallback"}
    assert st["filtered"] is False and st["fallback"] is False and (st["clash_cutoff"], st["contact_cutoff"]) == (3.0, 5.0)
    strip = lambda b: b"".join(l for l in b.splitlines(True) if not l.startswith(b"REMARK"))
    assert strip(pdb("screen.pdb")) == pdb("plain.pdb") and pdb("screen.pdb").startswith(b"REMARK")
    assert f"n_clash {st['n_clash']} n_contact {st['n_contact']}".encode() in pdb("screen.pdb").splitlines()[0]
    nc, nt, bc, bt = _pdb_sterics(str(tmp_path / "screen.pdb"), n_rec_atoms)
    print("kept pose:", st, "from the file:", nc, nt, "border", bc, bt)
    assert abs(st["n_clash"] - nc) <= bc and abs(st["n_contact"] - nt) <= bt
    assert len(line["models"]) == len(topk["models"]) >= 1
    for m, m0 in zip(line["models"], topk["models"]):
        assert set(m["sterics"]) == {"n_clash", "n_contact", "min_dist", "flagged"} and m["index"] == m0["index"]
        name = os.path.basename(m["path"])
        assert strip(pdb(name)) == pdb(os.path.basename(m0["path"]))
        nc, nt, bc, bt = _pdb_sterics(str(tmp_path / name), n_rec_atoms)
        assert abs(m["sterics"]["n_clash"] - nc) <= bc and abs(m["sterics"]["n_contact"] - nt) <= bt
    text = (tmp_path / "res.txt").read_text().splitlines()
    assert text[0].startswith("#") and sum(int(l.split()[3]) for l in text[1:]) == st["n_contact"]
    assert sum(int(l.split()[2]) for l in text[1:]) == st["n_clash"]
    # --clash-filter: refine's start_pos puts two of 24 trajectories into deep overlap (the ligand's CA centroid on the receptor's) and
    # t_begin = 0.02 without noise leaves them there.  CAPRI's rule then flags exactly those: with 2 outliers of 24 at about the same
    # count B and the rest near 0 the threshold is about (1/12 + 2 sqrt(11) / 12) B = 0.64 B.
    lig0 = np.asarray(lig["bb_coords"], np.float32)
    onto = (np.asarray(rec["bb_coords"], np.float32)[:, 1].mean(0) - lig0[:, 1].mean(0)).astype(np.float32)
    shift = np.zeros((24, 3), np.float32)
    shift[[5, 17]] = onto
    kw = dict(t_begin=0.02, num_samples=24, num_steps=4, seed=2, max_batch=16, selfcheck=False, perturb=False, start_shift=shift)
    scr = driver.refine_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "r_screen.pdb"), clash_screen=True, **kw)
    fil = driver.refine_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "r_filter.pdb"), clash_filter=True, **kw)
    sd = scr["sterics_data"]
    print("n_clash of the 24 trajectories:", sd["n_clash"].tolist(), "threshold", sd["threshold"], "flags", np.nonzero(sd["flags"])[0].tolist())
    assert np.nonzero(sd["flags"])[0].tolist() == [5, 17] and sd["n_clash"][[5, 17]].min() > 500
    assert np.array_equal(sd["n_clash"], fil["sterics_data"]["n_clash"]) and np.array_equal(sd["flags"], fil["sterics_data"]["flags"])
    assert not scr["sterics"]["filtered"] and fil["sterics"]["filtered"] and not fil["sterics"]["fallback"]
    assert fil["index"] not in (5, 17) and not fil["sterics"]["flagged"]
    assert fil["index"] == int(np.argmin(np.where(sd["flags"], np.inf, scr["trajectories"]["energy"])))
    assert scr["index"] == int(np.argmin(scr["trajectories"]["energy"]))      # the screen alone keeps the energy pick
    # the kept file of the filtered run holds what the line says
    nc, nt, bc, bt = _pdb_sterics(str(tmp_path / "r_filter.pdb"), n_rec_atoms)
    assert abs(fil["sterics"]["n_clash"] - nc) <= bc and abs(fil["sterics"]["n_contact"] - nt) <= bt
    # the definition agrees with the device on this ensemble's flags
    ra, la, cen = driver.sterics_inputs(rec, lig, 0)
    want = ST.sterics(ra, la, cen, scr["trajectories"]["rot_update"], scr["trajectories"]["tr_update"])
    assert np.abs(want["n_clash"] - sd["n_clash"]).max() <= 0.005 * want["n_clash"].max() + 2
