"""Interface hydrogen bonds and salt bridges on the GPU (dfm_hbond_create, dfm_pose_hbonds, kernels_hbond.hip) against their float64
definition dfmdock_amd/hbonds.py, and through the drivers and the command line.

Everything the call returns is an integer, so every comparison is np.array_equal against the definition.  Every call is also held
against itself: hb_kind.sum(1) == n_hbond, lig_hb.sum(1) == rec_hb.sum(1) == n_hbond, lig_sb.sum(1) == rec_sb.sum(1) == n_salt_atoms."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, complex_for
from test_hbonds_cpu import A, AN, CAT, D, SC, Z3, Z13, backbone_polar, chain, db5_definition, lump, poses

pytestmark = pytest.mark.gpu

TOTALS = ("n_hbond", "hb_kind", "n_salt", "n_salt_atoms")
KEYS = TOTALS + ("rec_hb", "lig_hb", "rec_sb", "lig_sb")


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def consistent(got, label=""):
    """The call's own consistency."""
    assert np.array_equal(got["hb_kind"].sum(1), got["n_hbond"]), label
    assert np.array_equal(got["lig_hb"].sum(1), got["n_hbond"]) and np.array_equal(got["rec_hb"].sum(1), got["n_hbond"]), label
    assert np.array_equal(got["lig_sb"].sum(1), got["n_salt_atoms"]) and np.array_equal(got["rec_sb"].sum(1), got["n_salt_atoms"]), label
    assert (got["n_salt"] <= got["n_salt_atoms"]).all() and ((got["n_salt"] > 0) == (got["n_salt_atoms"] > 0)).all(), label


def same(a, b, label="", keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)


def check(model, rec, lig, cen, rot, tr, label="", chunk_poses=0, want=None, **kw):
    """One handle, one call with every output, against the definition; returns (the device's result, the definition's)."""
    from dfmdock_amd import hbonds as HB
    want = HB.hbonds(rec, lig, cen, rot, tr, per_atom=True, **kw) if want is None else want
    with model.hbonds(rec, lig, cen, **kw) as h:
        got = h.count(rot, tr, per_atom=True, chunk_poses=chunk_poses)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype == np.int32 and got[k].shape == want[k].shape, (label, k)
        assert np.array_equal(got[k], want[k]), (label, k, np.argwhere(got[k] != want[k])[:5].tolist())
    consistent(got, label)
    print(f"{label}: P {len(rot)} Nr {len(rec['role'])} Nl {len(lig['role'])} bonds {int(got['n_hbond'].sum())} salt bridges "
          f"{int(got['n_salt'].sum())} / {int(got['n_salt_atoms'].sum())} atom pairs, poses without a bond {int((got['n_hbond'] == 0).sum())}")
    return got, want


@pytest.fixture(scope="module")
def db5_runs(model):
    """The DB5 recipe (tests/test_hbonds_cpu.py: db5_definition): per complex the definition, computed once, and the device's result."""
    return [(cid, rec, lig, cen, rot, tr, want, check(model, rec, lig, cen, rot, tr, label=cid, want=want)[0])
            for cid, rec, lig, cen, rot, tr, want in db5_definition()]


def test_parity_with_the_definition_on_db5(db5_runs):
    """384 poses, 549 hydrogen bonds, 175 poses without one, 48 bonds over the 24 identity poses with 9 each in 2SIC and 2SNI (counted by
    the definition on a CPU, tests/test_hbonds_cpu.py: test_db5_recipe, where no pair is within 1e-4 A of the cutoff or 1e-6 of cos = 0)."""
    n = np.concatenate([got["n_hbond"] for *_, got in db5_runs])
    ident = {cid: int(got["n_hbond"][0]) for cid, *_, got in db5_runs}
    print("bonds", int(n.sum()), "poses", n.size, "without one", int((n == 0).sum()), "identity poses", ident)
    assert (n.size, int(n.sum()), int((n == 0).sum())) == (384, 549, 175)
    assert sum(ident.values()) == 48 and ident["2SIC"] == 9 and ident["2SNI"] == 9
    assert all(not got["n_salt"].any() and not got["rec_sb"].any() and np.array_equal(got["hb_kind"][:, 0], got["n_hbond"]) for *_, got in db5_runs)


def test_cross_check_against_the_screen(model, db5_runs):
    """dfm_pose_sterics, an independent kernel on the same walk, over N, CA, C, O, CB at contact cutoff 3.5: every ligand residue with a
    bond has an atom in contact."""
    from conftest import db5_complex
    from test_gpu_sterics import ca_center, five_atoms
    from dfmdock_amd import sterics as ST
    bonded = 0
    for cid, rec, lig, cen, rot, tr, _, got in db5_runs:
        c = db5_complex(cid)
        lig5 = five_atoms(c["lig_pos"])
        with model.atoms(five_atoms(c["rec_pos"]), lig5, ca_center(c["lig_pos"]), 3.0, 3.5) as at:
            sd = at.sterics(rot, tr, per_atom=True)
        touched = ST.residue_counts(sd["lig_contact"], np.arange(lig5.shape[0]) // 5, lig["n_res"]) > 0
        with_bond = ST.residue_counts(got["lig_hb"], lig["res"], lig["n_res"]) > 0
        assert not (with_bond & ~touched).any(), cid
        bonded += int(with_bond.sum())
    assert bonded > 400


def charged_lump(rng, n, n_res, n_charged, center=(0, 0, 0), spread=4.0):
    """lump() with exactly the residues 0 .. n_charged - 1 charged: every other atom loses its CATION and ANION bits (and keeps a role),
    and each of those residues gets one atom that is cation or anion."""
    c = lump(rng, n, n_res, center, spread)
    c["role"] &= np.uint8(D | A | SC)
    c["role"][(c["role"] & (D | A)) == 0] |= np.uint8(D)
    pick = rng.permutation(n)[:n_charged]
    c["res"][pick] = np.arange(n_charged)
    c["res"][np.setdiff1d(np.arange(n), pick)] = rng.integers(0, n_res, n - n_charged)
    c["role"][pick] |= rng.choice(np.uint8([CAT, AN, CAT | AN]), n_charged)
    return c


def test_small_shapes(model):
    """The smallest shapes at which the kernels take another path, each against the definition."""
    from dfmdock_amd import hbonds as HB
    rng = np.random.default_rng(5)
    # Nl around the block of 64
    for Nl in (1, 63, 64, 65, 130):
        rec, lig = lump(rng, 90, 12), lump(rng, Nl, max(1, Nl // 4), center=(3, 0, 0))
        got, _ = check(model, rec, lig, lig["xyz"].astype(np.float64).mean(0).astype(np.float32), *poses(rng, 5), label=f"Nl {Nl}")
        assert Nl == 1 or (got["n_hbond"].sum() > 0 and got["n_salt"].sum() > 0)
    # the receptor's charged residues around the words of a bitmap row, cutoffs 8.0 on a tight lump: the last charged residue - the last
    # bit of the last word - is in a bridge
    for Rc in (0, 1, 31, 32, 33, 65):
        rec, lig = charged_lump(rng, 200, 70, Rc, spread=2.0), lump(rng, 70, 9, center=(1, 0, 0), spread=2.0)
        with model.hbonds(rec, lig, Z3, 8.0, 90.0, 8.0) as h:
            info = h.info()
        assert info["n_rec_charged"] == Rc and info["n_lig_charged"] == len(np.unique(lig["res"][(lig["role"] & (CAT | AN)) > 0])) and info["cell_edge"] == 8.0
        got, _ = check(model, rec, lig, Z3, *poses(rng, 4, 0.2, 0.5), label=f"Rc {Rc}, cutoffs 8", hb_cutoff=8.0, salt_cutoff=8.0)
        last = (rec["res"] == Rc - 1) & ((rec["role"] & (CAT | AN)) > 0)
        assert (Rc == 0 and not got["n_salt_atoms"].any()) or (got["rec_sb"][:, last].any() and got["n_salt"].max() >= min(Rc, 31))
    # a ligand without a charged residue: legal, no bridge
    rec, lig = lump(rng, 120, 15), charged_lump(rng, 40, 6, 0, center=(3, 0, 0))
    got, _ = check(model, rec, lig, Z3, *poses(rng, 4), label="no charged ligand residue")
    assert not got["n_salt"].any() and not got["lig_sb"].any() and got["n_hbond"].sum() > 0
    # min_angle 120, and 150 at cutoff 5
    rec, lig = lump(rng, 150, 15), lump(rng, 100, 10, center=(3, 0, 0))
    g90, _ = check(model, rec, lig, Z3, *poses(np.random.default_rng(1), 5), label="min_angle 90")
    g120, _ = check(model, rec, lig, Z3, *poses(np.random.default_rng(1), 5), label="min_angle 120", min_angle=120.0)
    assert 0 < g120["n_hbond"].sum() < g90["n_hbond"].sum() and np.array_equal(g120["n_salt_atoms"], g90["n_salt_atoms"])
    check(model, rec, lig, Z3, *poses(rng, 3), label="min_angle 150, cutoffs 5 / 3", min_angle=150.0, hb_cutoff=5.0, salt_cutoff=3.0)
    # ONE ligand residue of 130 cations (three blocks of 64: the same bit from several waves) against ONE receptor residue of anions
    # (every lane of a wave hits the same word at once): one bridge
    rec, lig = lump(rng, 100, 1, spread=2.0), lump(rng, 130, 1, center=(1, 0, 0), spread=2.0)
    rec["role"][:], lig["role"][:] = A | AN | SC, D | CAT | SC
    got, _ = check(model, rec, lig, Z3, *poses(rng, 4, 0.3, 0.5), label="one bridge, thousands of atom pairs")
    assert got["n_salt"].tolist() == [1, 1, 1, 1] and got["n_salt_atoms"].min() > 1000
    # more than 64 receptor atoms in one cell row: 150 atoms in one cell cross the staging batch twice
    one_cell = lump(rng, 150, 37, spread=1.0)
    one_cell["xyz"] = (1.2 * rng.random((150, 3))).astype(np.float32) + np.float32(1.0)
    lig = lump(rng, 90, 15)
    with model.hbonds(one_cell, lig, Z3) as h:
        assert h.info()["max_cell_atoms"] == 150 and h.info()["n_cells"] == 1
    got, _ = check(model, one_cell, lig, Z3, *poses(rng, 5), label="one cell, 150 atoms")
    assert got["n_hbond"].max() > 10
    # exactly at the cutoff, exactly at 90 degrees, a coincident antecedent: representable coordinates under the identity pose about the origin
    below = np.nextafter(np.float32(3.5), np.float32(0))
    rec = chain([(0, 0, 0)], [(-1.25, 0, 0)], [A | AN])
    lig = chain([(3.5, 0, 0), (0, below, 0), (0, 0, -3), (0, -3, 0), (-2, 0, 0), (4, 0, 0), (0, np.nextafter(np.float32(4), np.float32(0)), 0)],
                [(4.5, 0, 0), (-1, below, 0), (0, 1, -3), (0, -3, 0), (-3, 0, 0), (5, 0, 0), (0, 5, 0)],
                [D, D, D, D | SC, D, CAT, CAT | SC], [0, 1, 2, 3, 4, 5, 6])
    got, _ = check(model, rec, lig, Z3, Z13, Z13, label="at the thresholds")
    #  d == cutoff | below, both angles 90 | angle at X 90 | coincident antecedent | angle at Y is 0 | salt d == 4 | salt below 4
    assert got["lig_hb"][0].tolist() == [0, 1, 1, 1, 0, 0, 0] and got["lig_sb"][0].tolist() == [0, 0, 0, 0, 0, 0, 1]
    assert got["hb_kind"][0].tolist() == [2, 1, 0] and got["n_salt"][0] == 1
    # SER OG with THR OG1 is one bond; donor - donor is none
    got, _ = check(model, chain([(0, 0, 0), (0, 0, 9)], [(-1, 0, 0), (-1, 0, 9)], [D | A | SC, D]),
                   chain([(3, 0, 0), (3, 0, 9)], [(4, 0, 0), (4, 0, 9)], [D | A | SC, D | SC]), Z3, Z13, Z13, label="both ways")
    assert got["n_hbond"].tolist() == [1] and got["hb_kind"].tolist() == [[0, 0, 1]]
    # a pose far away takes the early exits: all zeros
    rec, lig = lump(rng, 300, 20), lump(rng, 70, 10)
    far = np.float32([[60.0, 0, 0], [0, -55.0, 0], [0, 0, 47.1], [-31.2, -31.2, -31.2]])
    got, _ = check(model, rec, lig, Z3, np.zeros((4, 3), np.float32), far, label="far away")
    assert not any(got[k].any() for k in KEYS)


ENSEMBLE_KW = dict(hb_cutoff=5.0, salt_cutoff=8.0)


def _ensemble_7cei(P=7, seed=2):
    """The 7CEI ensemble recipe of tests/test_gpu_affinity.py on the backbone's polar atoms, with seeded CATION / ANION / SIDECHAIN bits on
    top of the backbone's donors and acceptors so that bridges form; the tests take it at cutoffs 5 and 8 (ENSEMBLE_KW), at which most of
    these poses, 2 A apart per axis, have bonds and bridges."""
    from cli_fixtures import golden_7cei
    from test_gpu_sterics import ca_center
    cx, rs, ls = golden_7cei()
    rng = np.random.default_rng(seed)
    rot, tr = poses(rng, P, 0.2, 2.0)
    rec, lig = backbone_polar(cx["rec_pos"], rs), backbone_polar(cx["lig_pos"], ls)
    for c in (rec, lig):
        c["role"] = c["role"] | (rng.integers(0, 8, len(c["role"])).astype(np.uint8) << 2) * (rng.random(len(c["role"])) < 0.5).astype(np.uint8)
    return (rec, lig, ca_center(cx["lig_pos"])), rot, tr


def test_chunks_and_order(model):
    """What a result may not depend on: the chunks of a call, the call before it, the order of the poses, the outputs asked for."""
    from dfmdock_amd import engine, hbonds as HB
    (cx, rot, tr), rng = _ensemble_7cei(), np.random.default_rng(9)
    kw = ENSEMBLE_KW
    want = HB.hbonds(*cx, rot, tr, per_atom=True, **kw)
    assert (want["n_hbond"] > 0).sum() >= 3 and (want["n_salt"] > 0).sum() >= 4
    with model.hbonds(*cx, **kw) as h:
        info = h.info()
        Rc, Lc = (len(np.unique(c["res"][(c["role"] & (CAT | AN)) > 0])) for c in cx[:2])
        assert (info["n_rec_charged"], info["n_lig_charged"]) == (Rc, Lc) and info["cell_edge"] == 8.0 and info["n_cells"] >= 8
        assert info["chunk_poses"] == min(32768, max(1, (64 << 20) // (Lc * ((Rc + 31) // 32) * 4)))
        full = h.count(rot, tr, per_atom=True)
        same(full, want, "definition")
        for chunk in (1, 3, 0):
            same(full, h.count(rot, tr, per_atom=True, chunk_poses=chunk), f"chunk_poses {chunk}")
        same(full, h.count(rot, tr, per_atom=True), "the same handle called twice")
        # a dense first chunk, then poses far away: the second chunk's bitmap and per-atom arrays are zeroed again
        dense = np.argsort(-full["n_salt"], kind="stable")[:3]
        r6, t6 = np.concatenate([rot[dense], np.zeros((3, 3), np.float32)]), np.concatenate([tr[dense], np.float32([[90, 0, 0], [0, 90, 0], [0, 0, -90]])])
        two = h.count(r6, t6, per_atom=True, chunk_poses=3)
        assert full["n_salt"][dense].min() > 0
        same({k: full[k][dense] for k in KEYS}, {k: two[k][:3] for k in KEYS}, "first chunk")
        assert not any(two[k][3:].any() for k in KEYS)
        # permuted poses give permuted outputs
        perm = rng.permutation(7)
        same({k: full[k][perm] for k in KEYS}, h.count(rot[perm], tr[perm], per_atom=True, chunk_poses=2), "permuted poses")
        # any subset of the output pointers, through the C entry point
        lean = h.count(rot, tr)
        assert set(lean) == set(TOTALS)
        same(full, lean, "lean", TOTALS)
        from dfmdock_amd import _lib as L
        f = lambda x: x.ctypes.data_as(L.F32P)
        for keys in (("n_salt",), ("rec_sb", "hb_kind"), ("lig_hb",), ("n_hbond", "lig_sb", "rec_hb"), ()):
            out, bufs = L.HbondOutC(), {k: np.full_like(full[k], -7) for k in keys}
            for k, v in bufs.items():
                setattr(out, k, v.ctypes.data_as(L.I32P))
            assert L.lib().dfm_pose_hbonds_chunked(h._h, 7, f(rot), f(tr), 4, C.byref(out)) == 0
            same(full, bufs, f"subset {keys}", keys)
    cp, kn = engine.hbond_last_timing()
    assert cp > 0 and kn > 0 and abs(sum(engine.hbond_last_phases()) - kn) < 1e-3 * max(kn, 1.0) + 1e-3


def test_nan_poses(model):
    from dfmdock_amd import hbonds as HB
    (cx, rot, tr) = _ensemble_7cei(8, seed=3)
    kw = ENSEMBLE_KW
    with model.hbonds(*cx, **kw) as h:
        clean = h.count(rot, tr, per_atom=True)
        assert (clean["n_hbond"] > 0).sum() >= 3 and (clean["n_salt"] > 0).sum() >= 4
        r2, t2 = rot.copy(), tr.copy()
        r2[2, 1], t2[5, 0], t2[6, 2] = np.nan, np.inf, -np.inf
        dirty = h.count(r2, t2, per_atom=True)
    for p in (2, 5, 6):
        assert not any(dirty[k][p].any() for k in KEYS)
    keep = np.ones(8, bool)
    keep[[2, 5, 6]] = False
    same({k: clean[k][keep] for k in KEYS}, {k: dirty[k][keep] for k in KEYS}, "neighbours")
    same(dirty, HB.hbonds(*cx, r2, t2, per_atom=True, **kw), "definition")


def test_two_threads_on_one_handle(model):
    (cx, rot, tr) = _ensemble_7cei(12, seed=4)
    with model.hbonds(*cx, **ENSEMBLE_KW) as h:
        full = h.count(rot, tr, per_atom=True)
        res, errs = [None, None], []

        def work(i):
            try:
                res[i] = [h.count(rot, tr, per_atom=True, chunk_poses=(0, 5)[i]) for _ in range(3)]
            except BaseException as e:      # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errs, errs
    assert full["n_hbond"].sum() > 0 and full["n_salt"].sum() > 0
    for rs in res:
        for r in rs:
            same(full, r, "threads")


def test_invalid_arguments(model):
    """Every limit through the C entry points: DFM_E_INVALID / NULL, the code in `status` and a message, nothing enqueued; the handle
    works afterwards."""
    from dfmdock_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(4)
    rec, lig = lump(rng, 40, 10, spread=2.0), lump(rng, 30, 8, center=(1, 0, 0), spread=2.0)
    keep = []
    u8 = C.POINTER(C.c_uint8)
    types = (np.float32, np.float32, np.uint8, np.int32)
    ptrs = (L.F32P, L.F32P, u8, L.I32P)

    def create(m=model._h, Nr=40, rec=rec, n_rr=10, Nl=30, lig=lig, n_lr=8, cen=Z3, hb=3.5, c2=0.0, salt=4.0, drop=None):
        arrs = [None if (side, k) == drop else np.ascontiguousarray(c[k], t) for side, c in (("rec", rec), ("lig", lig))
                for k, t in zip(("xyz", "ante", "role", "res"), types)]
        cen_a = None if cen is None else np.ascontiguousarray(cen, np.float32)
        keep.append((arrs, cen_a))
        p = [None if a is None else a.ctypes.data_as(t) for a, t in zip(arrs, ptrs + ptrs)]
        status = C.c_int(99)
        h = lib.dfm_hbond_create(m, Nr, p[0], p[1], p[2], p[3], n_rr, Nl, p[4], p[5], p[6], p[7], n_lr, None if cen_a is None else cen_a.ctypes.data_as(L.F32P),
                                 hb, c2, salt, C.byref(status))
        return h, status.value

    def mod(c, key, i, v):
        q = dict(c, **{key: c[key].copy()})
        q[key][i] = v
        return q
    wide = mod(rec, "xyz", 0, 4000.0)      # more than 1000^3 cells of 4 A > 2^24
    cases = [(dict(m=None), "m is NULL"), (dict(drop=("rec", "xyz")), "rec_atoms is NULL"), (dict(drop=("lig", "xyz")), "lig_atoms is NULL"),
             (dict(cen=None), "center is NULL"), (dict(drop=("rec", "ante")), "rec_ante is NULL"), (dict(drop=("lig", "role")), "lig_role is NULL"),
             (dict(drop=("lig", "res")), "lig_res is NULL"), (dict(Nr=0), "Ar >= 1"), (dict(Nl=0), "Al >= 1"), (dict(Nr=(1 << 24) + 1), "exceeds 2^24 atoms"),
             (dict(rec=mod(rec, "xyz", (7, 1), np.nan)), "rec_atoms: atom 7 is not finite"), (dict(cen=np.float32([np.inf, 0, 0])), "center is not finite"),
             (dict(lig=mod(lig, "ante", (3, 0), np.nan)), "lig_ante: atom 3 is not finite"),
             (dict(n_rr=0), "rec: need 1 <= residues <= 4096"), (dict(n_rr=4097), "rec: need 1 <= residues <= 4096"),
             (dict(n_lr=0), "lig: need 1 <= residues <= 4096"), (dict(n_lr=4097), "lig: need 1 <= residues <= 4096"),
             (dict(rec=mod(rec, "role", 5, 32)), "rec_role: atom 5 has role 32 outside the five bits"),
             (dict(lig=mod(lig, "role", 29, 128)), "lig_role: atom 29 has role 128"),
             (dict(rec=mod(rec, "res", 5, 10)), "rec_res: atom 5 has residue 10 outside [0, 10)"), (dict(lig=mod(lig, "res", 0, -1)), "lig_res: atom 0 has residue -1"),
             (dict(hb=0.0), "hb_cutoff must be in (0, 8]"), (dict(hb=8.5), "hb_cutoff must be in (0, 8]"), (dict(hb=float("nan")), "hb_cutoff must be in (0, 8]"),
             (dict(salt=-1.0), "salt_cutoff must be in (0, 8]"), (dict(salt=9.0), "salt_cutoff must be in (0, 8]"),
             (dict(c2=-0.25), "min_cos2 must be in [0, 1)"), (dict(c2=1.0), "min_cos2 must be in [0, 1)"), (dict(c2=float("nan")), "min_cos2 must be in [0, 1)"),
             (dict(rec=wide), "more than 2^24 cells")]
    for kw, word in cases:
        h, status = create(**kw)
        msg = lib.dfm_last_error().decode()
        print(word, "->", status, msg)
        assert h is None and status == -1 and word in msg, (word, status, msg)
    a, status = create()
    assert a and status == 0
    f = lambda x: x.ctypes.data_as(L.F32P)
    rot, tr = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out = L.HbondOutC()
    n_sa = np.zeros(4, np.int32)
    out.n_salt_atoms = n_sa.ctypes.data_as(L.I32P)
    o = C.byref(out)
    for args, word in [((None, 4, f(rot), f(tr), o), "h is NULL"), ((a, 4, None, f(tr), o), "rot is NULL"), ((a, 4, f(rot), None, o), "tr is NULL"),
                       ((a, 4, f(rot), f(tr), None), "out is NULL"), ((a, 0, f(rot), f(tr), o), "1 <= P <= 65536"),
                       ((a, 65537, f(rot), f(tr), o), "1 <= P <= 65536")]:
        assert lib.dfm_pose_hbonds(*args) == -1, word
        assert word in lib.dfm_last_error().decode(), word
    assert lib.dfm_pose_hbonds_chunked(a, 4, f(rot), f(tr), -1, o) == -1 and "chunk_poses" in lib.dfm_last_error().decode()
    assert lib.dfm_hbond_last_timing(None, None) == -1 and lib.dfm_hbond_info(None, None, None, None, None, None, None) == -1
    assert lib.dfm_pose_hbonds(a, 4, f(rot), f(tr), o) == 0 and (n_sa == n_sa[0]).all() and n_sa[0] > 0      # the handle still works
    lib.dfm_hbond_destroy(a)
    lib.dfm_hbond_destroy(None)
    for bad in (dict(hb_cutoff=9.0), dict(min_angle=80.0), dict(salt_cutoff=0.0)):
        with pytest.raises(ValueError):
            model.hbonds(rec, lig, Z3, **bad)
    with pytest.raises(ValueError):
        model.hbonds(dict(rec, res=rec["res"][:-1]), lig, Z3)
    with pytest.raises(ValueError):
        model.hbonds(rec, mod(lig, "role", 1, 64), Z3)
    with pytest.raises(ValueError):
        model.hbonds(rec, lig, Z3[:2])


ALLOC_ENVS = {"nan": {"DFM_ALLOC_POISON": "255"}, "junk": {"DFM_ALLOC_POISON": "90"}, "guard": {"DFM_ALLOC_GUARD": "64", "DFM_ALLOC_POISON": "90"}}


def test_under_the_allocator_diagnostics(tmp_path):
    """One call with every output (two chunks) and one lean call in a child process under DFM_ALLOC_POISON / DFM_ALLOC_GUARD, set as
    tests/test_gpu_alloc_diag.py sets them: byte-equal to the plain child's outputs and to the definition, and no damaged band.  A child
    that ends by a signal or at its limit stops the test: nothing more is started."""
    import alloc_recipe as ar
    runs = {}
    for tag, extra in [("default", {})] + list(ALLOC_ENVS.items()):
        out = str(tmp_path / f"{tag}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("DFM_")}      # the switches are read once per process
        env.update(extra)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hbond_alloc_child.py"), out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=60)
        assert p.returncode == 0, f"{tag}: exit {p.returncode}\n" + p.stdout.decode(errors="replace")[-2000:]
        runs[tag] = dict(np.load(out, allow_pickle=False))
    ref = runs["default"]
    assert len([k for k in ref if not k.startswith("__")]) == 12 and ref["full/n_hbond"].sum() > 0 and ref["full/n_salt"].sum() > 0
    assert ref["__differs_from_definition"].tolist() == []
    for tag, extra in ALLOC_ENVS.items():
        r = runs[tag]
        d, cfg = dict(zip(ar.DIAG, r["__diag"].tolist())), str(r["__config"])
        assert ar.compare(ref, r) == [] and r["__differs_from_definition"].tolist() == [], tag
        assert all(f"{k}={v}" in cfg for k, v in extra.items()) and d["blocks"] > 0 and d["poisoned_bytes"] > 0, (tag, d, cfg)
        if "DFM_ALLOC_GUARD" in extra:
            assert d["bands_checked"] == 2 * d["blocks"] and d["bands_damaged"] == 0 and d["first_damaged_size"] == -1, d
        else:
            assert d["bands_checked"] == 0 and d["bands_damaged"] == 0, d


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def test_drivers_and_cli(model, tmp_path):
    """One `dock --hbonds --bsa --top-k 2 --hbond-residues` run on 7CEI with the seeded checkpoint, end to end: the counts of the line and
    of every model equal the definition on that pose, n_unsat equals hbonds.unsatisfied on the surface call's per-atom points, the
    residue files hold the definition's per-residue counts; without the flag nothing changes."""
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    from dfmdock_amd import cli, driver, hbonds as HB
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    base = [rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--seed", "3", "--max-batch", "8", "--no-selfcheck", "--num-samples", "8",
            "--num-steps", "6"]
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    kw = dict(num_samples=8, num_steps=6, seed=3, max_batch=8, selfcheck=False)
    p1 = _run(["dock"] + base + ["--out", "hb.pdb", "--hbonds", "--bsa", "--top-k", "2", "--hbond-residues", "f.txt"], cwd=str(tmp_path))
    assert p1.returncode == 0, p1.stdout + p1.stderr
    line = json.loads(p1.stdout.strip().splitlines()[-1])
    d0 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "plain.pdb"), **kw)
    d1 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api.pdb"), hbonds=True, bsa=True, top_k=2, **kw)
    pdb = lambda name: open(tmp_path / name, "rb").read()
    assert not any(k in d0 for k in ("n_hbond", "hbond_data", "index")) and pdb("hb.pdb") == pdb("plain.pdb") == pdb("api.pdb") and line["energy"] == d0["energy"]
    fields = ("n_hbond", "hb_bb_bb", "hb_bb_sc", "hb_sc_sc", "n_salt", "n_unsat")
    k = line["index"]
    assert k == d1["index"] and all(line[f] == d1[f] for f in fields) and "hbond_untyped" not in line and "polar atoms" not in p1.stderr
    # the definition on every trajectory
    rp, lp, cen = driver.hbond_inputs(rec, lig, 0)
    hd, tj = d1["hbond_data"], d1["trajectories"]
    want = HB.hbonds(rp, lp, cen, tj["rot_update"], tj["tr_update"], per_atom=True)
    same(want, hd, "trajectories")
    assert np.array_equal(np.float32(line["rot_update"]), tj["rot_update"][k]) and np.array_equal(np.float32(line["tr_update"]), tj["tr_update"][k])
    bd = d1["bsa_data"]
    unsat = sum(HB.unsatisfied(pa["role"], bd[s + "_exposed"][pa["index"]], bd[s + "_buried"][:, pa["index"]], want[s + "_hb"])["n_unsat"]
                for s, pa in (("rec", rp), ("lig", lp)))
    assert np.array_equal(hd["n_unsat"], unsat)

    def pose_fields(p):
        return {"n_hbond": int(want["n_hbond"][p]), "hb_bb_bb": int(want["hb_kind"][p, 0]), "hb_bb_sc": int(want["hb_kind"][p, 1]),
                "hb_sc_sc": int(want["hb_kind"][p, 2]), "n_salt": int(want["n_salt"][p]), "n_unsat": int(unsat[p])}
    assert {f: line[f] for f in fields} == pose_fields(k) and 1 <= len(line["models"]) <= 2
    assert [m["index"] for m in line["models"]] == [m["index"] for m in d1["models"]]
    for m in line["models"]:
        assert {f: m[f] for f in fields} == pose_fields(m["index"]), m
    print("kept", k, pose_fields(k), "bonds of every trajectory", want["n_hbond"].tolist(), "n_unsat", unsat.tolist())
    assert line["hb_bb_sc"] == line["hb_sc_sc"] == line["n_salt"] == 0      # the files hold backbones and no OXT

    # the residue files: the definition's per-residue counts of the kept pose and of every model
    def table(path, p):
        HB.write_hbond_residues(path, rp["keys"], HB.residue_bonds(want["rec_hb"][p], rp["res"], rp["n_res"]), HB.residue_bonds(want["rec_sb"][p], rp["res"], rp["n_res"]),
                                lp["keys"], HB.residue_bonds(want["lig_hb"][p], lp["res"], lp["n_res"]), HB.residue_bonds(want["lig_sb"][p], lp["res"], lp["n_res"]))
        return open(path, "rb").read()
    assert pdb("f.txt") == table(str(tmp_path / "want.txt"), k) and os.path.samefile(line["hbond_residues"], tmp_path / "f.txt")
    for m in line["models"]:
        assert pdb(f"f_{m['rank']}.txt") == table(str(tmp_path / "want_m.txt"), m["index"])
    # refine_pair goes through the same path, with other parameters and without the surface
    r1 = driver.refine_pair(model, rec, lig, rec_x, lig_x, t_begin=0.05, num_samples=4, num_steps=4, seed=2, max_batch=4, selfcheck=False,
                            out_pdb=None, hbonds=True, hbond_cutoff=3.8, hbond_angle=100.0, salt_cutoff=5.0)
    w2 = HB.hbonds(rp, lp, cen, r1["trajectories"]["rot_update"], r1["trajectories"]["tr_update"], 3.8, 100.0, 5.0)
    assert np.array_equal(w2["n_hbond"], r1["hbond_data"]["n_hbond"]) and r1["n_hbond"] == int(w2["n_hbond"][r1["index"]]) and "n_unsat" not in r1
