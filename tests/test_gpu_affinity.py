"""Residue contacts by class on the GPU (dfm_rescon_create, dfm_pose_rescon, kernels_rescon.hip) against their float64 definition
dfmdock_amd/affinity.py, and through the drivers and the command line.

Everything the call returns is an integer and a set does not depend on the order its members were found in, so every comparison is
np.array_equal: ic, n_pairs, n_rec_res, n_lig_res, both degree arrays and contact_bits.  Every call is also held against itself:
ic.sum(1) == n_pairs == popcount(bits), and the degrees equal the row and column popcounts."""
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

KEYS = ("ic", "n_pairs", "n_rec_res", "n_lig_res", "rec_degree", "lig_degree", "contact_bits")


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def consistent(got, Rr, label=""):
    """The call's own consistency."""
    from dfmdock_amd import affinity as AF
    bits = got["contact_bits"]
    m = np.stack([AF.unpack_bits(b, Rr) for b in bits])      # [P,Lr,Rr]
    assert np.array_equal(got["ic"].sum(1), got["n_pairs"]) and np.array_equal(got["n_pairs"], AF.popcount(bits)), label
    assert np.array_equal(got["lig_degree"], m.sum(2)) and np.array_equal(got["rec_degree"], m.sum(1)), label
    assert np.array_equal(got["n_rec_res"], (got["rec_degree"] > 0).sum(1)) and np.array_equal(got["n_lig_res"], (got["lig_degree"] > 0).sum(1)), label
    assert AF.popcount(bits).sum() == m.sum(), label      # no bit past Rr in the last word of a row


def same(a, b, label="", keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)


def check(model, rec, rres, rcls, lig, lres, lcls, cen, rot, tr, cutoff=5.5, chunk_poses=0, label=""):
    """One handle, one call with every output, against the definition; returns (the device's result, the definition's)."""
    from dfmdock_amd import affinity as AF
    want = AF.residue_contacts(rec, rres, rcls, lig, lres, lcls, cen, rot, tr, cutoff, per_residue=True, bits=True)
    with model.contacts(rec, rres, rcls, lig, lres, lcls, cen, cutoff) as h:
        got = h.count(rot, tr, per_residue=True, bits=True, chunk_poses=chunk_poses)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (label, k)
        assert np.array_equal(got[k], want[k]), (label, k, np.argwhere(got[k] != want[k])[:5].tolist())
    consistent(got, len(rcls), label)
    print(f"{label}: P {len(rot)} Ar {len(rec)} Al {len(lig)} Rr {len(rcls)} Lr {len(lcls)} residue pairs {int(got['n_pairs'].sum())} "
          f"empty poses {int((got['n_pairs'] == 0).sum())}")
    return got, want


def random_complex(rng, Ar, Al, Rr, Lr, spread=4.0, sep=3.0):
    """Two lumps `sep` A apart; residues assigned at random, so some may have no atom."""
    rec = (spread * rng.standard_normal((Ar, 3))).astype(np.float32)
    lig = (spread * rng.standard_normal((Al, 3)) + np.float32([sep, 0, 0])).astype(np.float32)
    return (rec, rng.integers(0, Rr, Ar).astype(np.int32), rng.integers(0, 3, Rr).astype(np.uint8),
            lig, rng.integers(0, Lr, Al).astype(np.int32), rng.integers(0, 3, Lr).astype(np.uint8), lig.astype(np.float64).mean(0).astype(np.float32))


def poses(rng, P, s_rot=0.4, s_tr=1.5):
    return (s_rot * rng.standard_normal((P, 3))).astype(np.float32), (s_tr * rng.standard_normal((P, 3))).astype(np.float32)


def _ensemble_7cei(P=24, seed=1):
    from test_gpu_sterics import ca_center, five_atoms
    cx = complex_for("fwd_7CEI_p0")
    rng = np.random.default_rng(seed)
    rot, tr = poses(rng, P, 0.2, 2.0)
    rec, lig = five_atoms(cx["rec_pos"]), five_atoms(cx["lig_pos"])
    Rr, Lr = rec.shape[0] // 5, lig.shape[0] // 5
    return (rec, (np.arange(rec.shape[0]) // 5).astype(np.int32), rng.integers(0, 3, Rr).astype(np.uint8), lig,
            (np.arange(lig.shape[0]) // 5).astype(np.int32), rng.integers(0, 3, Lr).astype(np.uint8), ca_center(cx["lig_pos"])), rot, tr


@pytest.fixture(scope="module")
def db5_runs(model):
    """The DB5 recipe of tests/test_gpu_sterics.py: N, CA, C, O, CB of the 24 committed backbones, 16 poses each from one default_rng(0)
    stream, classes from the committed sequences through IC_CLASS.  Per complex: the definition, the device's result and the device's
    all-atom screen at contact cutoff 5.5 on the same atoms and poses."""
    from test_gpu_sterics import ca_center, db5_poses, five_atoms
    from dfmdock_amd import affinity as AF
    rng = np.random.default_rng(0)
    runs, missed = [], 0
    for cid in db5_ids():
        c = db5_complex(cid)
        rot, tr = db5_poses(rng)
        rec, lig, cen = five_atoms(c["rec_pos"]), five_atoms(c["lig_pos"]), ca_center(c["lig_pos"])
        rcls, m1 = AF.residue_classes(list(c["rec_seq"]), AF.IC_CLASS)
        lcls, m2 = AF.residue_classes(list(c["lig_seq"]), AF.IC_CLASS)
        missed += m1 + m2
        rres, lres = (np.arange(rec.shape[0]) // 5).astype(np.int32), (np.arange(lig.shape[0]) // 5).astype(np.int32)
        got, want = check(model, rec, rres, rcls, lig, lres, lcls, cen, rot, tr, label=cid)
        with model.atoms(rec, lig, cen, 3.0, 5.5) as at:
            sd = at.sterics(rot, tr, per_atom=True)
        runs.append((cid, got, want, sd, lres, len(lcls)))
    return runs, missed


def test_parity_with_the_definition_on_db5(db5_runs):
    """17 012 residue pairs over 384 poses, 4 of them empty, AA 4592, AP 4398, AC 3922, PP 970, PC 2102, CC 1028 (counted by the
    definition on a CPU); no sequence letter outside the 20."""
    runs, missed = db5_runs
    ic = sum(got["ic"].astype(np.int64).sum(0) for _, got, _, _, _, _ in runs)
    empty = sum(int((got["n_pairs"] == 0).sum()) for _, got, _, _, _, _ in runs)
    print("ic", ic.tolist(), "total", int(ic.sum()), "empty poses", empty, "letters outside the 20:", missed)
    assert sum(len(got["n_pairs"]) for _, got, _, _, _, _ in runs) == 384 and missed == 0
    assert int(ic.sum()) == 17012 and empty == 4 and ic.tolist() == [4592, 4398, 3922, 970, 2102, 1028]


def test_cross_check_against_the_screen(db5_runs):
    """dfm_pose_sterics, an independent kernel on the same walk: the ligand residues with an atom in contact are those with a partner
    residue, and a pose has a contact pair iff it has a residue pair."""
    from dfmdock_amd import sterics as ST
    for cid, got, _, sd, lres, Lr in db5_runs[0]:
        touched = ST.residue_counts(sd["lig_contact"], lres, Lr) > 0
        assert np.array_equal(touched, got["lig_degree"] > 0), cid
        assert np.array_equal(sd["n_contact"] > 0, got["n_pairs"] > 0), cid


def test_small_shapes(model):
    """The smallest shapes at which the kernels take another path, each against the definition."""
    rng = np.random.default_rng(5)
    zero = np.zeros(3, np.float32)
    z1 = np.zeros((1, 3), np.float32)
    # Al around the block of 64; Rr around the words of a bitmap row.  Residues drawn at random: some have no atom
    for Al, Rr in ((1, 33), (63, 1), (64, 32), (65, 31), (130, 65)):
        cx = random_complex(rng, 90, Al, Rr, max(1, Al // 4))
        rot, tr = poses(rng, 5)
        got, _ = check(model, *cx, rot, tr, label=f"Al {Al}, Rr {Rr}")
        assert got["n_pairs"].sum() > 0
    for Rr in (1, 31, 32, 33, 65):
        rec, rres, rcls, lig, lres, lcls, cen = random_complex(rng, 200, 70, Rr, 9)
        rres[:Rr] = np.arange(Rr)      # every residue has an atom, the last bit of the last word included
        rot, tr = poses(rng, 4, 0.2, 0.5)
        got, _ = check(model, rec, rres, rcls, lig, lres, lcls, cen, rot, tr, cutoff=16.0, label=f"Rr {Rr}, cutoff 16")
        assert got["rec_degree"][:, Rr - 1].any() and got["n_rec_res"].max() > min(Rr, 31) - 1
    # a receptor residue and a ligand residue without atoms: never in contact
    rec, rres, rcls, lig, lres, lcls, cen = random_complex(rng, 120, 40, 40, 12)
    rres[rres == 7], lres[lres == 3] = 8, 4
    got, _ = check(model, rec, rres, rcls, lig, lres, lcls, cen, *poses(rng, 4), label="residues without atoms")
    assert not got["rec_degree"][:, 7].any() and not got["lig_degree"][:, 3].any() and got["n_pairs"].sum() > 0
    # ONE ligand residue of 130 atoms (three blocks of 64: the same bits from several waves) against ONE receptor residue (every
    # lane of a wave hits the same word at once), next to a second residue pair
    rec, _, _, lig, _, _, cen = random_complex(rng, 100, 130, 1, 1, spread=2.0, sep=1.0)
    rres, lres = np.zeros(100, np.int32), np.zeros(130, np.int32)
    rres[-1], lres[-1] = 1, 1
    got, _ = check(model, rec, rres, np.uint8([2, 0]), lig, lres, np.uint8([1, 2]), cen, *poses(rng, 4, 0.3, 0.5), label="one residue pair, 13 000 atom pairs")
    assert (got["contact_bits"][:, 0, 0] & 1).all()
    # more than 64 receptor atoms in one cell row: 150 atoms in one cell cross the staging batch twice
    lig = (4.0 * rng.standard_normal((90, 3))).astype(np.float32)
    one_cell = (1.2 * rng.random((150, 3))).astype(np.float32) + np.float32(1.0)
    got, _ = check(model, one_cell, (np.arange(150) % 37).astype(np.int32), rng.integers(0, 3, 37).astype(np.uint8), lig,
                   (np.arange(90) // 6).astype(np.int32), rng.integers(0, 3, 15).astype(np.uint8), zero, *poses(rng, 5), label="one cell, 150 atoms")
    assert got["n_pairs"].max() > 100
    # a pair at exactly d == cutoff does not count, the next float32 below does: representable coordinates under the identity pose
    # about the origin (R = I and tr = 0 leave every coordinate as it is)
    below = np.nextafter(np.float32(5.5), np.float32(0))
    rec = np.float32([[0, 0, 0]])
    lig = np.float32([[5.5, 0, 0], [below, 0, 0], [0, -5.5, 0], [0, 0, -below], [0, 5.5, 5.5]])
    got, want = check(model, rec, np.int32([0]), np.uint8([1]), lig, np.arange(5, dtype=np.int32), np.uint8([0, 1, 2, 0, 1]), zero, z1, z1,
                      label="d == cutoff")
    assert got["lig_degree"][0].tolist() == [0, 1, 0, 1, 0] and got["ic"][0].tolist() == [0, 1, 0, 1, 0, 0]
    # a pose far away takes the early exits: all zeros
    cx = random_complex(rng, 300, 70, 20, 10)
    far = np.float32([[60.0, 0, 0], [0, -55.0, 0], [0, 0, 47.1], [-31.2, -31.2, -31.2]])
    got, _ = check(model, *cx, np.zeros((4, 3), np.float32), far, label="far away")
    assert not any(got[k].any() for k in KEYS)


def test_chunks_and_order(model):
    """What a result may not depend on: the chunks of a call, the call before it, the order of the poses."""
    (cx, rot, tr), rng = _ensemble_7cei(7, seed=2), np.random.default_rng(9)
    from dfmdock_amd import affinity as AF, engine
    want = AF.residue_contacts(*cx, rot, tr, per_residue=True, bits=True)
    assert (want["n_pairs"] > 0).sum() >= 4
    with model.contacts(*cx) as h:
        info = h.info()
        Rr, Lr = len(cx[2]), len(cx[5])
        assert info["row_words"] == (Rr + 31) // 32 and info["cell_edge"] == 5.5 and info["n_cells"] >= 8
        assert info["chunk_poses"] == min(32768, max(1, (64 << 20) // (Lr * info["row_words"] * 4)))
        full = h.count(rot, tr, per_residue=True, bits=True)
        same(full, want, "definition")
        for chunk in (1, 3, 0):
            same(full, h.count(rot, tr, per_residue=True, bits=True, chunk_poses=chunk), f"chunk_poses {chunk}")
        same(full, h.count(rot, tr, per_residue=True, bits=True), "the same handle called twice")
        # a dense first chunk, then poses far away: the second chunk's bitmap is zeroed again
        dense = np.argsort(-full["n_pairs"], kind="stable")[:3]
        r6, t6 = np.concatenate([rot[dense], np.zeros((3, 3), np.float32)]), np.concatenate([tr[dense], np.float32([[90, 0, 0], [0, 90, 0], [0, 0, -90]])])
        two = h.count(r6, t6, per_residue=True, bits=True, chunk_poses=3)
        assert full["n_pairs"][dense].min() > 0
        same({k: full[k][dense] for k in KEYS}, {k: two[k][:3] for k in KEYS}, "first chunk")
        assert not any(two[k][3:].any() for k in KEYS)
        # permuted poses give permuted outputs
        perm = rng.permutation(7)
        got = h.count(rot[perm], tr[perm], per_residue=True, bits=True, chunk_poses=2)
        same({k: full[k][perm] for k in KEYS}, got, "permuted poses")
        # any subset of the output pointers
        lean = h.count(rot, tr)
        assert set(lean) == {"ic", "n_pairs", "n_rec_res", "n_lig_res"}
        same(full, lean, "lean", tuple(lean))
    cp, kn = engine.rescon_last_timing()
    assert cp > 0 and kn > 0


def test_nan_poses(model):
    (cx, rot, tr) = _ensemble_7cei(8, seed=3)
    from dfmdock_amd import affinity as AF
    with model.contacts(*cx) as h:
        clean = h.count(rot, tr, per_residue=True, bits=True)
        assert (clean["n_pairs"] > 0).sum() >= 4
        r2, t2 = rot.copy(), tr.copy()
        r2[2, 1], t2[5, 0], t2[6, 2] = np.nan, np.inf, -np.inf
        dirty = h.count(r2, t2, per_residue=True, bits=True)
    for p in (2, 5, 6):
        assert not any(dirty[k][p].any() for k in KEYS)
    keep = np.ones(8, bool)
    keep[[2, 5, 6]] = False
    same({k: clean[k][keep] for k in KEYS}, {k: dirty[k][keep] for k in KEYS}, "neighbours")
    same(dirty, AF.residue_contacts(*cx, r2, t2, per_residue=True, bits=True), "definition")


def test_two_threads_on_one_handle(model):
    (cx, rot, tr) = _ensemble_7cei(12, seed=4)
    with model.contacts(*cx) as h:
        full = h.count(rot, tr, per_residue=True, bits=True)
        res, errs = [None, None], []

        def work(i):
            try:
                res[i] = [h.count(rot, tr, per_residue=True, bits=True, chunk_poses=(0, 5)[i]) for _ in range(3)]
            except BaseException as e:      # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errs, errs
    assert full["n_pairs"].sum() > 0
    for rs in res:
        for r in rs:
            same(full, r, "threads")


def test_invalid_arguments(model):
    """Every limit through the C entry points: DFM_E_INVALID / NULL and a message, nothing enqueued; the handle works afterwards."""
    from dfmdock_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(4)
    rec, rres, rcls, lig, lres, lcls, cen = random_complex(rng, 40, 30, 10, 8, spread=2.0, sep=1.0)
    h = model._h
    keep = []
    u8 = C.POINTER(C.c_uint8)

    def create(m=h, Ar=40, rec=rec, rres=rres, Rr=10, rcls=rcls, Al=30, lig=lig, lres=lres, Lr=8, lcls=lcls, cen=cen, cutoff=5.5):
        a = [None if v is None else np.ascontiguousarray(v, t) for v, t in ((rec, np.float32), (rres, np.int32), (rcls, np.uint8),
                                                                               (lig, np.float32), (lres, np.int32), (lcls, np.uint8), (cen, np.float32))]
        keep.append(a)
        p = [None if v is None else v.ctypes.data_as(t) for v, t in zip(a, (L.F32P, L.I32P, u8, L.F32P, L.I32P, u8, L.F32P))]
        return lib.dfm_rescon_create(m, Ar, p[0], p[1], Rr, p[2], Al, p[3], p[4], Lr, p[5], p[6], cutoff)

    def mod(a, i, v):
        q = a.copy()
        q[i] = v
        return q
    nan_rec, inf_cen = rec.copy(), cen.copy()
    nan_rec[7, 1], inf_cen[0] = np.nan, np.inf
    wide = rec.copy()
    wide[0] = 4000.0      # more than 700^3 cells of 5.5 A > 2^24
    many = np.zeros(4097, np.uint8)
    cases = [(dict(m=None), "m is NULL"), (dict(rec=None), "rec_atoms is NULL"), (dict(lig=None), "lig_atoms is NULL"), (dict(cen=None), "center is NULL"),
             (dict(rres=None), "rec_res is NULL"), (dict(lres=None), "lig_res is NULL"), (dict(rcls=None), "rec_class is NULL"),
             (dict(lcls=None), "lig_class is NULL"), (dict(Ar=0), "Ar >= 1"), (dict(Al=0), "Al >= 1"), (dict(Ar=(1 << 24) + 1), "exceeds 2^24 atoms"),
             (dict(rec=nan_rec), "rec_atoms: atom 7 is not finite"), (dict(cen=inf_cen), "center is not finite"),
             (dict(Rr=0), "rec: need 1 <= residues <= 4096"), (dict(Rr=4097, rcls=many), "rec: need 1 <= residues <= 4096"),
             (dict(Lr=0), "lig: need 1 <= residues <= 4096"), (dict(Lr=4097, lcls=many), "lig: need 1 <= residues <= 4096"),
             (dict(rres=mod(rres, 5, 10)), "rec_res: atom 5 has residue 10 outside [0, 10)"), (dict(rres=mod(rres, 0, -1)), "rec_res: atom 0 has residue -1"),
             (dict(lres=mod(lres, 29, 8)), "lig_res: atom 29 has residue 8 outside [0, 8)"),
             (dict(rcls=mod(rcls, 9, 3)), "rec_class: residue 9 has class 3"), (dict(lcls=mod(lcls, 0, 255)), "lig_class: residue 0 has class 255"),
             (dict(cutoff=0.0), "cutoff must be in (0, 16]"), (dict(cutoff=16.5), "cutoff must be in (0, 16]"), (dict(cutoff=float("nan")), "cutoff must be in (0, 16]"),
             (dict(rec=wide), "more than 2^24 cells")]
    for kw, word in cases:
        assert create(**kw) is None, word
        msg = lib.dfm_last_error().decode()
        print(word, "->", msg)
        assert word in msg, (word, msg)
    a = create()
    assert a
    f = lambda x: x.ctypes.data_as(L.F32P)
    rot, tr = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out = L.ResconOutC()
    n_pairs = np.zeros(4, np.int32)
    out.n_pairs = n_pairs.ctypes.data_as(L.I32P)
    o = C.byref(out)
    for args, word in [((None, 4, f(rot), f(tr), o), "h is NULL"), ((a, 4, None, f(tr), o), "rot is NULL"), ((a, 4, f(rot), None, o), "tr is NULL"),
                       ((a, 4, f(rot), f(tr), None), "out is NULL"), ((a, 0, f(rot), f(tr), o), "1 <= P <= 65536"),
                       ((a, 65537, f(rot), f(tr), o), "1 <= P <= 65536")]:
        assert lib.dfm_pose_rescon(*args) == -1, word
        assert word in lib.dfm_last_error().decode(), word
    assert lib.dfm_pose_rescon_chunked(a, 4, f(rot), f(tr), -1, o) == -1 and "chunk_poses" in lib.dfm_last_error().decode()
    assert lib.dfm_rescon_last_timing(None, None) == -1 and lib.dfm_rescon_info(None, None, None, None, None, None) == -1
    assert lib.dfm_pose_rescon(a, 4, f(rot), f(tr), o) == 0 and (n_pairs == n_pairs[0]).all() and n_pairs[0] > 0      # the handle still works
    lib.dfm_rescon_destroy(a)
    lib.dfm_rescon_destroy(None)
    with pytest.raises(ValueError):
        model.contacts(rec, rres, rcls, lig, lres, lcls, cen, cutoff=17.0)
    with pytest.raises(ValueError):
        model.contacts(rec, rres[:-1], rcls, lig, lres, lcls, cen)
    with pytest.raises(ValueError):
        model.contacts(rec, rres, rcls, lig, lres, mod(lcls, 1, 3), cen)
    with pytest.raises(ValueError):
        model.contacts(rec, rres, rcls, lig, lres, lcls, cen[:2])


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def test_drivers_and_cli(model, tmp_path):
    """One `dock --affinity --contact-residues` run on 7CEI with the seeded checkpoint, end to end: the object's ic equals the definition
    on the kept pose, dg equals affinity.dg of the reported inputs bit for bit, the residue file has n_pairs lines; dock_pair returns
    the same object, one per model, and the arrays of every trajectory."""
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    from dfmdock_amd import affinity as AF
    from dfmdock_amd import cli, driver
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    base = [rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--seed", "3", "--max-batch", "8", "--no-selfcheck", "--num-samples", "8",
            "--num-steps", "6"]
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    kw = dict(num_samples=8, num_steps=6, seed=3, max_batch=8, selfcheck=False)
    p1 = _run(["dock"] + base + ["--out", "aff.pdb", "--affinity", "--contact-residues", "pairs.txt"], cwd=str(tmp_path))
    assert p1.returncode == 0, p1.stdout + p1.stderr
    line = json.loads(p1.stdout.strip().splitlines()[-1])
    d0 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "plain.pdb"), **kw)
    d1 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api.pdb"), affinity=True, top_k=3, **kw)
    pdb = lambda name: open(tmp_path / name, "rb").read()
    assert "affinity" not in d0 and "index" not in d0 and pdb("aff.pdb") == pdb("plain.pdb") == pdb("api.pdb") and line["energy"] == d0["energy"]
    af = line["affinity"]
    assert set(af) == {"ic", "n_pairs", "n_rec_res", "n_lig_res", "nis_apolar", "nis_charged", "dg", "kd", "cutoff"} and af["cutoff"] == 5.5
    k = line["index"]
    assert k == d1["index"] and af == json.loads(json.dumps(d1["affinity"]))
    # the definition on the kept pose, and on every trajectory
    inp = driver.rescon_inputs(rec, lig, 0)
    tj = d1["trajectories"]
    want = AF.residue_contacts(*inp[:7], tj["rot_update"], tj["tr_update"], bits=True)
    ad = d1["affinity_data"]
    for key in ("ic", "n_pairs", "n_rec_res", "n_lig_res"):
        assert np.array_equal(want[key], ad[key]), key
    assert af["ic"] == want["ic"][k].tolist() and af["n_pairs"] == int(want["n_pairs"][k]) and want["n_pairs"].max() > 0
    print("kept", k, af)
    # dg of the reported inputs, bit for bit; kd of it; the contact part of every trajectory
    assert af["dg"] == float(AF.dg(np.int64(af["ic"]), af["nis_apolar"], af["nis_charged"])[0]) and af["kd"] == float(AF.kd(af["dg"]))
    assert np.array_equal(ad["dg_contacts"], AF.dg_contacts(want["ic"])) and 0.0 <= af["nis_apolar"] <= 100.0 and 0.0 <= af["nis_charged"] <= 100.0
    assert all(m["affinity"] == driver._pose_affinity(ad, m["index"]) for m in d1["models"]) and len(d1["models"]) >= 1
    assert ad["unclassified"] == (0, 0) and "affinity_unclassified" not in line
    # with --bsa at the default probe and points one surface call serves both: the same numbers either way
    d3 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=None, affinity=True, bsa=True, **kw)
    assert d3["affinity"] == d1["affinity"] and np.array_equal(d3["affinity_data"]["nis"], ad["nis"]) and d3["bsa"] > 0
    assert d3["bsa"] == driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=None, bsa=True, **kw)["bsa"]
    # the residue file: one line per residue pair of the kept pose, the definition's pairs
    AF.write_contact_residues(str(tmp_path / "want.txt"), inp[7], inp[8], AF.pairs_of(want["contact_bits"][k]))
    assert pdb("pairs.txt") == pdb("want.txt") and len(pdb("pairs.txt").splitlines()) == 1 + af["n_pairs"]
    # refine_pair goes through the same path
    r1 = driver.refine_pair(model, rec, lig, rec_x, lig_x, t_begin=0.05, num_samples=4, num_steps=4, seed=2, max_batch=4, selfcheck=False,
                            out_pdb=None, affinity=True, affinity_cutoff=6.0)
    w2 = AF.residue_contacts(*inp[:7], r1["trajectories"]["rot_update"], r1["trajectories"]["tr_update"], 6.0)
    assert np.array_equal(w2["ic"], r1["affinity_data"]["ic"]) and r1["affinity"]["cutoff"] == 6.0 and r1["affinity"]["ic"] == w2["ic"][r1["index"]].tolist()
