"""Interface energy on the GPU (dfm_iface_create, dfm_pose_iface_energy, kernels_iface.hip) against its float64 definition
dfmdock_amd/ifenergy.py, and through the drivers and the command line.

Every result is an integer: a count, or a sum of terms rounded to quanta of 2^-20 kcal/mol.  The terms are fp64 + - * / in a fixed order
on both sides (no square root, no transcendental, nothing contracted), which IEEE 754 rounds correctly on host and device alike, so the
device's integers must EQUAL the definition's - rep_q, att_q, elec_q, n_pairs and both per-atom arrays - and the pose totals must equal
the sums of the call's own per-atom arrays."""
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

KEYS = ("rep_q", "att_q", "elec_q", "n_pairs")
ATOM_KEYS = ("lig_vdw_q", "lig_elec_q")


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def five_atoms(bb):
    from dfmdock_amd import pdbio
    return pdbio.full_backbone(bb).reshape(-1, 3)


def five_atom_params(n_res, rng):
    """ifenergy.atom_parameters on the records of N, CA, C, O, CB of n_res residues of one chain, plus a seeded +-0.5 charge on every
    CB so that the Coulomb term has pairs of both signs."""
    from dfmdock_amd import ifenergy as IE
    atoms = [{"hetero": False, "name": nm, "res_name": "ALA", "chain": "A", "res_id": i + 1, "ins": " ", "coord": (0.0, 0.0, 0.0),
              "element": nm[0]} for i in range(n_res) for nm in ("N", "CA", "C", "O", "CB")]
    par = IE.atom_parameters(atoms)
    par[4::5, 2] = rng.choice(np.float32([-0.5, 0.5]), n_res)
    assert par[0, 2] == 1.0 and par.shape == (5 * n_res, 3)
    return par


def ca_center(bb):
    return np.asarray(bb, np.float64)[:, 1].mean(0).astype(np.float32)


def db5_poses(rng, P=16):
    """The recipe of tests/test_gpu_sterics.py: per pose an axis, an angle in [0, 0.3) and a translation of 2 A per axis; pose 0 is the
    identity (its draws are still consumed)."""
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


def random_params(n, rng, charged=True):
    par = np.zeros((n, 3), np.float32)
    par[:, 0] = rng.uniform(1.5, 2.2, n)
    par[:, 1] = rng.uniform(0.1, 0.6, n)
    if charged:
        par[:, 2] = rng.choice(np.float32([-1.0, -0.5, 0.0, 0.0, 0.5, 1.0]), n)
    return par


def check_against_definition(model, rec, rp, lig, lp, center, rot, tr, label="", chunk_poses=0, **scalars):
    """One handle, one call with per-atom output: integer equality with the definition on all six arrays, totals == the call's own
    per-atom sums.  Returns (pairs, result)."""
    from dfmdock_amd import ifenergy as IE
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    with model.interface(rec, rp, lig, lp, center, **scalars) as h:
        got = h.energy(rot, tr, per_atom=True, chunk_poses=chunk_poses)
    want = IE.interface_energy(rec, rp, lig, lp, center, rot, tr, per_atom=True, **scalars)
    P, Al = rot.shape[0], np.asarray(lig).reshape(-1, 3).shape[0]
    assert got["lig_vdw_q"].shape == (P, Al) and all(got[k].dtype == np.int64 for k in KEYS + ATOM_KEYS)
    assert np.array_equal(got["rep_q"] + got["att_q"], got["lig_vdw_q"].sum(1)) and np.array_equal(got["elec_q"], got["lig_elec_q"].sum(1)), label
    for k in ("n_pairs",) + KEYS + ATOM_KEYS:
        off = got[k] != want[k]
        assert not off.any(), (label, k, int(off.sum()), got[k][off][:5].tolist(), want[k][off][:5].tolist())
    assert np.array_equal(got["rep"], got["rep_q"] / 2.0 ** 20)
    print(f"{label}: P {P} Ar {np.asarray(rec).reshape(-1, 3).shape[0]} Al {Al} pairs {int(want['n_pairs'].sum())} rep {want['rep_q'].sum() / 2.0 ** 20:.3f} "
          f"att {want['att_q'].sum() / 2.0 ** 20:.3f} elec {want['elec_q'].sum() / 2.0 ** 20:.3f} kcal/mol")
    return int(want["n_pairs"].sum()), got


def test_parity_with_the_definition_on_db5(model):
    """N, CA, C, O, CB of the 24 DB5 backbones, 16 seeded poses each from one default_rng(0) stream, the default scalars.  Integer
    equality of everything."""
    rng, prng = np.random.default_rng(0), np.random.default_rng(1)
    pairs = 0
    for cid in db5_ids():
        c = db5_complex(cid)
        rot, tr = db5_poses(rng)
        rec, lig = five_atoms(c["rec_pos"]), five_atoms(c["lig_pos"])
        rp, lp = five_atom_params(rec.shape[0] // 5, prng), five_atom_params(lig.shape[0] // 5, prng)
        n, got = check_against_definition(model, rec, rp, lig, lp, ca_center(c["lig_pos"]), rot, tr, label=cid)
        pairs += n
    print("pairs within 8 A:", pairs)
    assert pairs > 83223      # the pairs below 5 A of the same recipe (tests/test_gpu_sterics.py)


def _ensemble_7cei(P=96, seed=1):
    cx = complex_for("fwd_7CEI_p0")
    rng = np.random.default_rng(seed)
    rot = (0.2 * rng.standard_normal((P, 3))).astype(np.float32)
    tr = (2.0 * rng.standard_normal((P, 3))).astype(np.float32)
    rec, lig = five_atoms(cx["rec_pos"]), five_atoms(cx["lig_pos"])
    return rec, five_atom_params(rec.shape[0] // 5, rng), lig, five_atom_params(lig.shape[0] // 5, rng), ca_center(cx["lig_pos"]), rot, tr


def _same(a, b, keys, label=""):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (label, k)


def test_invariances_are_exact(model):
    from dfmdock_amd import _lib as L
    from dfmdock_amd import engine
    rec, rp, lig, lp, cen, rot, tr = _ensemble_7cei()
    with model.interface(rec, rp, lig, lp, cen) as h:
        full = h.energy(rot, tr, per_atom=True)
        assert (full["n_pairs"] > 0).sum() > 48 and (full["elec_q"] != 0).any() and (full["rep_q"] > 0).any()
        parts = [h.energy(rot[lo:hi], tr[lo:hi], per_atom=True) for lo, hi in ((0, 31), (31, 32), (32, 96))]
        _same(full, {k: np.concatenate([q[k] for q in parts]) for k in KEYS + ATOM_KEYS}, KEYS + ATOM_KEYS, "split")
        perm = np.random.default_rng(2).permutation(96)
        _same({k: full[k][perm] for k in KEYS + ATOM_KEYS}, h.energy(rot[perm], tr[perm], per_atom=True), KEYS + ATOM_KEYS, "permuted")
        for cp in (1, 7, 96):
            _same(full, h.energy(rot, tr, per_atom=True, chunk_poses=cp), KEYS + ATOM_KEYS, f"chunk {cp}")
            _same(full, h.energy(rot, tr, chunk_poses=cp), KEYS, f"chunk {cp}, no per-atom output")
        _same(full, h.energy(rot, tr), KEYS, "no per-atom output")
        # any subset of the output pointers NULL
        f = lambda x: x.ctypes.data_as(L.F32P)
        for mask in range(64):
            out, bufs = L.IfaceOutC(), {}
            for b, k in enumerate(KEYS + ATOM_KEYS):
                if mask >> b & 1:
                    bufs[k] = np.full_like(full[k], 7)
                    setattr(out, k, bufs[k].ctypes.data_as(C.POINTER(C.c_int64)))
            assert L.lib().dfm_pose_iface_energy(h._h, 96, f(rot), f(tr), C.byref(out)) == 0, mask
            _same(full, bufs, tuple(bufs), f"pointer mask {mask}")
        # two host threads on the same handle at once
        res, errs = [None, None], []

        def work(i):
            try:
                res[i] = [h.energy(rot, tr, per_atom=True, chunk_poses=(0, 5)[i]) for _ in range(3)]
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
        info = h.info()
        assert info["cell_edge"] == 8.0 and info["n_cells"] >= 8 and 1 <= info["max_cell_atoms"] <= rec.shape[0]
        assert np.abs(full["lig_vdw_q"]).max() < info["sum_bound_q"] < 2.0 ** 62
    cp, kn = engine.iface_last_timing()
    assert cp > 0 and kn > 0


def test_small_shapes(model):
    """Sizes and placements at which the kernel takes another path, each against the definition."""
    from dfmdock_amd import ifenergy as IE
    rng = np.random.default_rng(5)
    zero = np.zeros(3, np.float32)
    poses = lambda P, s_rot=0.5, s_tr=1.5: ((s_rot * rng.standard_normal((P, 3))).astype(np.float32), (s_tr * rng.standard_normal((P, 3))).astype(np.float32))
    chk = lambda *a, **k: check_against_definition(model, *a, **k)
    # Al around the block size, one receptor atom
    one = np.array([[0.5, -0.25, 1.0]], np.float32)
    for Al in (1, 63, 64, 65, 130):
        lig = (3.0 * rng.standard_normal((Al, 3))).astype(np.float32)
        rot, tr = poses(6)
        n, _ = chk(one, random_params(1, rng), lig, random_params(Al, rng), lig.mean(0), rot, tr, label=f"Ar 1, Al {Al}")
        assert n > 0 or Al == 1
    # every receptor atom in one cell (150: crosses the 64-atom staging batch twice); 200 atoms at one point
    lig = (4.0 * rng.standard_normal((90, 3))).astype(np.float32)
    lp = random_params(90, rng)
    rot, tr = poses(5)
    one_cell = (1.2 * rng.random((150, 3))).astype(np.float32) + np.float32(1.0)
    n, _ = chk(one_cell, random_params(150, rng), lig, lp, zero, rot, tr, label="one cell, 150 atoms")
    assert n > 1000
    point = np.tile(np.array([[1.0, 2.0, -0.5]], np.float32), (200, 1))
    n, _ = chk(point, random_params(200, rng), lig, lp, zero, rot, tr, label="200 atoms at one point")
    assert n >= 200 and n % 200 == 0
    # a ligand wholly outside the grid box by more than the cutoff: nothing
    rec = (8.0 * rng.random((300, 3))).astype(np.float32)
    rp = random_params(300, rng)
    lig = (2.0 * rng.random((70, 3))).astype(np.float32)
    lp = random_params(70, rng)
    far = np.array([[40.0, 0, 0], [0, -35.0, 0], [0, 0, 17.1], [-11.2, -11.2, -11.2]], np.float32)
    n, got = chk(rec, rp, lig, lp, lig.mean(0), np.zeros((4, 3), np.float32), far, label="outside by more than the cutoff")
    assert n == 0 and not any(got[k].any() for k in KEYS + ATOM_KEYS)
    # outside by less than the cutoff on the low side: negative cell coordinates before the clamp
    low = np.array([[-7.5, 3.0, 3.0], [3.0, -8.5, 3.0], [3.0, 3.0, -9.0], [-5.0, -5.0, -5.0]], np.float32)
    n, _ = chk(rec, rp, lig, lp, lig.mean(0), np.zeros((4, 3), np.float32), low, label="outside on the low side by less than the cutoff")
    assert n > 0
    # ligand atoms exactly on cell faces (the grid's origin is the receptor's low corner, the edge 8)
    grid = np.array([[0, 0, 0], [16, 16, 16], [2, 3, 4], [8.5, 7.5, 9.0], [15, 1, 1], [7.0, 9.0, 15.0]], np.float32)
    face = np.array([[8, 8, 8], [16, 8, 0], [0, 0, 0], [8, 4, 12], [16, 16, 16], [24, 8, 8]], np.float32)
    n, _ = chk(grid, random_params(6, rng), face, random_params(6, rng), zero, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32),
               label="atoms on cell faces")
    assert n > 0
    # P = 1; soft = 1; elec_min_dist above the cutoff; all charges zero
    rec, rp, lig, lp, cen, rot, tr = _ensemble_7cei(4, seed=7)
    assert chk(rec, rp, lig, lp, cen, rot[:1], tr[:1], label="P = 1")[0] > 0
    assert chk(rec, rp, lig, lp, cen, rot, tr, soft=1.0, label="soft = 1")[0] > 0
    n, got = chk(rec, rp, lig, lp, cen, rot, tr, elec_min_dist=9.0, label="elec_min_dist above the cutoff")
    assert n > 0 and (got["elec_q"] != 0).any()
    n, got = chk(rec, rp * np.float32([1, 1, 0]), lig, lp * np.float32([1, 1, 0]), cen, rot, tr, label="all charges zero")
    assert n > 0 and not got["elec_q"].any() and not got["lig_elec_q"].any()
    n, _ = chk(rec, rp, lig, lp, cen, rot, tr, cutoff=5.0, dielectric_slope=1.0, label="cutoff 5, slope 1")
    assert n > 0
    # a deep overlap at the parameter limits: the largest allowed term (sqrt_eps 2 x 2, soft 0.5: 4 * 2^12 kcal/mol = 2^34 quanta; charges
    # 4 x -4 at elec_min_dist 1) on 200 x 130 coincident pairs, the totals against Python-int sums of the definition's terms
    lim = np.tile(np.float32([[8.0, 2.0, 4.0]]), (200, 1))
    liml = np.tile(np.float32([[8.0, 2.0, -4.0]]), (130, 1))
    ligp = np.tile(point[:1], (130, 1))
    z1 = np.zeros((1, 3), np.float32)
    kw = dict(soft=0.5, elec_min_dist=1.0, dielectric_slope=1.0, cutoff=16.0)
    n, got = chk(point, lim, ligp, liml, point[0], z1, z1, label="deep overlap at the limits", **kw)
    rq, aq, eq = IE.pair_terms(np.zeros(1), liml[:1], lim[:1], 0.5, 1.0, 1.0)
    assert n == 26000 and int(rq[0]) == 1 << 34 and int(aq[0]) == -(1 << 29)
    assert int(got["rep_q"][0]) == 26000 * int(rq[0]) and int(got["att_q"][0]) == 26000 * int(aq[0]) and int(got["elec_q"][0]) == 26000 * int(eq[0])
    assert int(eq[0]) == -int(np.rint(332.0637 * 16.0 * 2.0 ** 20))


def test_nan_poses(model):
    rec, rp, lig, lp, cen, rot, tr = _ensemble_7cei(8, seed=3)
    with model.interface(rec, rp, lig, lp, cen) as h:
        clean = h.energy(rot, tr, per_atom=True)
        assert (clean["n_pairs"] > 0).sum() >= 4
        r2, t2 = rot.copy(), tr.copy()
        r2[2, 1] = np.nan
        t2[5, 0] = np.inf
        dirty = h.energy(r2, t2, per_atom=True)
    for p in (2, 5):
        assert not any(dirty[k][p].any() for k in KEYS + ATOM_KEYS)
    keep = np.ones(8, bool)
    keep[[2, 5]] = False
    _same({k: clean[k][keep] for k in KEYS + ATOM_KEYS}, {k: dirty[k][keep] for k in KEYS + ATOM_KEYS}, KEYS + ATOM_KEYS)
    from dfmdock_amd import ifenergy as IE
    want = IE.interface_energy(rec, rp, lig, lp, cen, r2, t2)
    assert not want["n_pairs"][[2, 5]].any() and np.array_equal(want["n_pairs"], dirty["n_pairs"])


def test_invalid_arguments(model):
    """DFM_E_INVALID / NULL, dfm_last_error set, nothing enqueued; create / destroy leaves the block cache's accounting sane."""
    from dfmdock_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(4)
    rec, lig = (6.0 * rng.random((40, 3))).astype(np.float32), (6.0 * rng.random((30, 3))).astype(np.float32)
    rp, lp = random_params(40, rng), random_params(30, rng)
    cen = lig.mean(0)
    f = lambda x: None if x is None else np.ascontiguousarray(x, np.float32).ctypes.data_as(L.F32P)
    h = model._h
    keep = []      # the arrays behind the pointers of one call

    def create(m=h, Ar=40, rec=rec, rp=rp, Al=30, lig=lig, lp=lp, cen=cen, sc=(8.0, 0.6, 3.0, 4.0), null=()):
        col = lambda p, k: None if p is None else np.ascontiguousarray(p[:, k])
        a = {"rec": rec, "rh_r": col(rp, 0), "se_r": col(rp, 1), "q_r": col(rp, 2), "lig": lig, "rh_l": col(lp, 0), "se_l": col(lp, 1),
             "q_l": col(lp, 2), "cen": cen}
        a = {k: (None if k in null or v is None else np.ascontiguousarray(v, np.float32)) for k, v in a.items()}
        keep.append(a)
        p = {k: f(v) for k, v in a.items()}
        return lib.dfm_iface_create(m, Ar, p["rec"], p["rh_r"], p["se_r"], p["q_r"], Al, p["lig"], p["rh_l"], p["se_l"], p["q_l"], p["cen"], *sc)

    def mod(par, i, k, v):
        q = par.copy()
        q[i, k] = v
        return q
    nan_rec, nan_lig, inf_cen = rec.copy(), lig.copy(), cen.copy()
    nan_rec[7, 1], nan_lig[3, 2], inf_cen[0] = np.nan, np.inf, np.inf
    wide = rec.copy()
    wide[0] = 4000.0      # 500^3 cells of 8 A > 2^24
    big = np.tile(np.float32([[2.0, 2.0, 0.0]]), (40, 1))
    cases = [(dict(m=None), "m is NULL"), (dict(null=("rec",)), "rec_atoms is NULL"), (dict(null=("lig",)), "lig_atoms is NULL"),
             (dict(null=("cen",)), "center is NULL"), (dict(null=("rh_r",)), "rec_rmin_half is NULL"), (dict(null=("se_r",)), "rec_sqrt_eps is NULL"),
             (dict(null=("q_r",)), "rec_charge is NULL"), (dict(null=("rh_l",)), "lig_rmin_half is NULL"),
             (dict(null=("se_l",)), "lig_sqrt_eps is NULL"), (dict(null=("q_l",)), "lig_charge is NULL"),
             (dict(Ar=0), "Ar >= 1"), (dict(Al=0), "Al >= 1"), (dict(Ar=(1 << 24) + 1), "exceeds 2^24 atoms"),
             (dict(rec=nan_rec), "rec_atoms: atom 7 is not finite"), (dict(lig=nan_lig), "lig_atoms: atom 3 is not finite"),
             (dict(cen=inf_cen), "center is not finite"),
             (dict(rp=mod(rp, 5, 0, 0.0)), "rec_rmin_half: atom 5 is not in (0, 8]"), (dict(rp=mod(rp, 5, 0, 8.5)), "rec_rmin_half: atom 5 is not in (0, 8]"),
             (dict(lp=mod(lp, 2, 0, np.nan)), "lig_rmin_half: atom 2 is not in (0, 8]"),
             (dict(rp=mod(rp, 6, 1, -0.1)), "rec_sqrt_eps: atom 6 is not in [0, 2]"), (dict(lp=mod(lp, 9, 1, 2.5)), "lig_sqrt_eps: atom 9 is not in [0, 2]"),
             (dict(rp=mod(rp, 1, 2, 4.5)), "rec_charge: atom 1 is not in [-4, 4]"), (dict(lp=mod(lp, 0, 2, -np.inf)), "lig_charge: atom 0 is not in [-4, 4]"),
             (dict(sc=(0.0, 0.6, 3.0, 4.0)), "cutoff must be in (0, 16]"), (dict(sc=(16.5, 0.6, 3.0, 4.0)), "cutoff must be in (0, 16]"),
             (dict(sc=(np.nan, 0.6, 3.0, 4.0)), "cutoff must be in (0, 16]"),
             (dict(sc=(8.0, 0.4, 3.0, 4.0)), "soft must be in [0.5, 1]"), (dict(sc=(8.0, 1.1, 3.0, 4.0)), "soft must be in [0.5, 1]"),
             (dict(sc=(8.0, 0.6, 0.5, 4.0)), "elec_min_dist must be finite and >= 1"), (dict(sc=(8.0, 0.6, np.inf, 4.0)), "elec_min_dist must be finite and >= 1"),
             (dict(sc=(8.0, 0.6, 3.0, 0.0)), "dielectric_slope must be finite and > 0"), (dict(sc=(8.0, 0.6, 3.0, -4.0)), "dielectric_slope must be finite and > 0"),
             (dict(rec=wide), "more than 2^24 cells"),
             # 40 x 30 pairs: a slope of 1e-30 makes one Coulomb term 1e32 kcal/mol
             (dict(sc=(8.0, 0.6, 3.0, 1e-30)), "could reach 2^62 quanta")]
    for kw, word in cases:
        assert create(**kw) is None, word
        msg = lib.dfm_last_error().decode()
        print(word, "->", msg)
        assert word in msg, (word, msg)
    lib.dfm_trim_cache(-1)
    for _ in range(20):
        a = create()
        assert a
        lib.dfm_iface_destroy(a)
    parked = lib.dfm_trim_cache(-1)
    assert 0 < parked <= 7 * 65536 and lib.dfm_trim_cache(-1) == 0      # seven blocks of one 64 KiB granule, handed on from handle to handle
    a = create()
    rot, tr = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out = L.IfaceOutC()
    n_pairs = np.zeros(4, np.int64)
    out.n_pairs = n_pairs.ctypes.data_as(C.POINTER(C.c_int64))
    o = C.byref(out)
    for args, word in [((None, 4, f(rot), f(tr), o), "h is NULL"), ((a, 4, None, f(tr), o), "rot is NULL"), ((a, 4, f(rot), None, o), "tr is NULL"),
                       ((a, 4, f(rot), f(tr), None), "out is NULL"), ((a, 0, f(rot), f(tr), o), "P >= 1")]:
        assert lib.dfm_pose_iface_energy(*args) == -1, word
        assert word in lib.dfm_last_error().decode(), word
    assert lib.dfm_pose_iface_energy_chunked(a, 4, f(rot), f(tr), -1, o) == -1 and "chunk_poses" in lib.dfm_last_error().decode()
    assert lib.dfm_iface_last_timing(None, None) == -1 and lib.dfm_iface_info(None, None, None, None, None) == -1
    assert lib.dfm_pose_iface_energy(a, 4, f(rot), f(tr), o) == 0 and (n_pairs == n_pairs[0]).all() and n_pairs[0] > 0      # the handle still works
    lib.dfm_iface_destroy(a)
    lib.dfm_iface_destroy(None)
    with pytest.raises(ValueError):
        model.interface(rec, rp, lig, lp, cen, soft=0.3)
    with pytest.raises(ValueError):
        model.interface(rec, rp[:, :2], lig, lp, cen)
    with pytest.raises(ValueError):
        model.interface(rec, rp, lig, lp, cen[:2])


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def test_drivers_and_cli(model, tmp_path):
    """On 7CEI with the seeded checkpoint.  Without the new flags `dock` writes what dock_pair without options writes and its line has
    no new key; --interface-energy adds the object and moves nothing else; under --rank interface the kept pose is the argmin of the
    total recomputed by the definition over every trajectory; --energy-residues holds the definition's per-residue sums of that pose."""
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    from dfmdock_amd import cli, driver
    from dfmdock_amd import ifenergy as IE
    from dfmdock_amd import sterics as ST
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    base = [rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--seed", "3", "--max-batch", "8", "--no-selfcheck", "--num-samples", "8",
            "--num-steps", "6"]
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    pdb = lambda name: open(tmp_path / name, "rb").read()
    kw = dict(num_samples=8, num_steps=6, seed=3, max_batch=8, selfcheck=False)
    # the default is untouched
    p0 = _run(["dock"] + base + ["--out", "plain.pdb"], cwd=str(tmp_path))
    assert p0.returncode == 0, p0.stdout + p0.stderr
    plain = json.loads(p0.stdout.strip().splitlines()[-1])
    d0 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api.pdb"), **kw)
    assert pdb("plain.pdb") == pdb("api.pdb") and plain["energy"] == d0["energy"]
    assert set(plain) == {"energy", "output", "num_samples", "precision", "rot_update", "tr_update", "selfcheck_ok"}
    assert "interface_energy" not in d0 and "index" not in d0 and "trajectories" not in d0
    # --interface-energy alone: the object, the same pose, the same file
    p1 = _run(["dock"] + base + ["--out", "ie.pdb", "--interface-energy", "--top-k", "3"], cwd=str(tmp_path))
    assert p1.returncode == 0, p1.stdout + p1.stderr
    line = json.loads(p1.stdout.strip().splitlines()[-1])
    assert pdb("ie.pdb") == pdb("plain.pdb") and line["energy"] == plain["energy"]
    assert set(line["interface_energy"]) == {"rep", "att", "elec", "total", "n_pairs", "rank", "weights", "cutoff", "ranked_by"}
    assert line["interface_energy"]["ranked_by"] == "energy" and line["interface_energy"]["weights"] == [0.18, 1.0, 0.5] and line["interface_energy"]["cutoff"] == 8.0
    assert all(set(m["interface_energy"]) == {"rep", "att", "elec", "total", "n_pairs"} for m in line["models"]) and len(line["models"]) >= 1
    # --rank interface against the definition over every trajectory
    p2 = _run(["dock"] + base + ["--out", "rank.pdb", "--rank", "interface", "--energy-residues", "res.txt"], cwd=str(tmp_path))
    assert p2.returncode == 0, p2.stdout + p2.stderr
    ranked = json.loads(p2.stdout.strip().splitlines()[-1])
    d2 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api_rank.pdb"), rank="interface", consensus=True, **kw)
    tj = d2["trajectories"]
    ra, rp, la, lp, cen = driver.iface_inputs(rec, lig, 0)
    want = IE.interface_energy(ra, rp, la, lp, cen, tj["rot_update"], tj["tr_update"], per_atom=True)
    for k in KEYS:
        assert np.array_equal(want[k], d2["interface_data"][k]), k
    total = IE.total(IE.kcal(want["rep_q"]), IE.kcal(want["att_q"]), IE.kcal(want["elec_q"]))
    k = int(np.argmin(total))
    print("totals", total.tolist(), "kept", k, "energy pick", int(np.argmin(tj["energy"])))
    assert d2["index"] == k == ranked["index"] and pdb("rank.pdb") == pdb("api_rank.pdb") and (want["n_pairs"] > 0).any()
    # the consensus object next to it describes the same, kept pose
    cs, cdata = d2["consensus"], d2["consensus_data"]
    assert cs["ranked_by"] == "interface" and cs["n_contacts"] == int(cdata["n_contacts"][k])
    assert cs["score"] == (None if np.isnan(cdata["consensus"][k]) else float(cdata["consensus"][k]))
    assert d2["interface_energy"]["total"] == float(d2["interface_data"]["total"][d2["index"]])
    ie = ranked["interface_energy"]
    assert ie["ranked_by"] == "interface" and ie["rank"] == 1 and ie["total"] == float(total[k]) and ie["n_pairs"] == int(want["n_pairs"][k])
    assert (ie["rep"], ie["att"], ie["elec"]) == tuple(float(IE.kcal(want[q][k])) for q in ("rep_q", "att_q", "elec_q"))
    assert np.array_equal(np.float32(ranked["rot_update"]), tj["rot_update"][k])
    # --energy-residues: the definition's per-atom sums of the kept pose, per ligand residue
    keys, res = ST.residue_of_atoms(lig["atoms"], ST.heavy_atoms(lig["atoms"]))
    vdw, elec = IE.residue_energy(want["lig_vdw_q"][k], res, len(keys)), IE.residue_energy(want["lig_elec_q"][k], res, len(keys))
    IE.write_energy_residues(str(tmp_path / "want.txt"), keys, vdw, elec)
    assert pdb("res.txt") == pdb("want.txt") and len(pdb("res.txt").splitlines()) > 1
    # with --clash-filter the flagged poses get NaN keys, exactly as for consensus ranking.  refine's start_shift puts two of 24 into deep
    # overlap; with the attraction alone as the total (weights 0, 1, 0) those two have the LOWEST totals, so only the filter keeps them out
    lig0 = np.asarray(lig["bb_coords"], np.float32)
    onto = (np.asarray(rec["bb_coords"], np.float32)[:, 1].mean(0) - lig0[:, 1].mean(0)).astype(np.float32)
    shift = np.zeros((24, 3), np.float32)
    shift[[5, 17]] = onto
    rk = dict(t_begin=0.02, num_samples=24, num_steps=4, seed=2, max_batch=16, selfcheck=False, perturb=False, start_shift=shift, out_pdb=None)
    fil = driver.refine_pair(model, rec, lig, rec_x, lig_x, clash_filter=True, rank="interface", ie_weights=(0.0, 1.0, 0.0), **rk)
    flags, tot = fil["sterics_data"]["flags"], fil["interface_data"]["total"]
    print("totals (attraction only)", tot.tolist(), "flags", np.nonzero(flags)[0].tolist(), "kept", fil["index"])
    assert np.nonzero(flags)[0].tolist() == [5, 17] and sorted(np.argsort(tot)[:2].tolist()) == [5, 17]
    assert fil["index"] == int(np.argmin(np.where(flags, np.inf, tot))) and fil["index"] not in (5, 17)
    assert fil["interface_energy"]["rank"] == 1 and fil["interface_energy"]["total"] == float(tot[fil["index"]])
    # the same trajectories through the clustering of top_k: the flagged poses' keys are NaN, so no model is one of them or led by one,
    # the models come in ascending total and model 1 is the kept pose
    gx = type("G", (), {"lig_pos0": lig0, "close": lambda self: None})()
    tj = fil["trajectories"]
    run = driver._Run(model, gx, rec, lig, {c: tj[c] for c in ("energy", "rot_update", "tr_update")}, "fp32",
                      dict(sterics=driver._check_sterics(False, True, 3.0, 5.0), interface=driver._check_interface(True, "interface", (0.0, 1.0, 0.0), 8.0)))
    run.key = tj["energy"]
    res = driver._finish(run, (np.argmin, "energy"), lambda k: {}, clu=(24, 4.0, "energy"))
    idx = [m["index"] for m in res["models"]]
    totals = [m["interface_energy"]["total"] for m in res["models"]]
    print("models", idx, totals)
    assert res["index"] == fil["index"] == idx[0] and not set(idx) & {5, 17} and totals == sorted(totals) and len(idx) >= 1
    assert all(m["interface_energy"]["total"] == float(tot[m["index"]]) for m in res["models"])
