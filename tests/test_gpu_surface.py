"""Buried surface area on the GPU (dfm_surface_create, dfm_pose_bsa, kernels_surface.hip) against its float64 definition
dfmdock_amd/surface.py, and through the drivers and the command line.

Counts are integers.  A border point is an exposed point whose smallest d - R_j over the other chain's candidate atoms is within 1e-6 A of
0: it may fall either way (the pose's atoms come from a float64 matrix product whose last bits depend on the library).  On every atom
without a border point the per-atom counts must equal the definition exactly, elsewhere differ by at most the atom's number of border
points; border points may be at most 0.1 % of the buried points; the per-pose and per-class counts must equal the sums of the call's own
per-atom counts, and bsa must be bitwise the definition's formula on the call's own class_points."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, complex_for, db5_complex, db5_ids
from test_gpu_sterics import ca_center, db5_poses, five_atoms

pytestmark = pytest.mark.gpu

BORDER = 1e-6
RAD5 = np.float32([1.55, 1.70, 1.70, 1.52, 1.70])      # N, CA, C, O, CB
KEYS = ("bsa", "lig_points", "rec_points", "class_points")
ATOM_KEYS = ("lig_buried", "rec_buried")


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def radii5(atoms):
    return np.tile(RAD5, len(atoms) // 5)


def check_own_sums(got, rr, lr, values, probe, K, label=""):
    """The per-pose outputs of a call against its own per-atom arrays; bsa bitwise from its own class_points."""
    from dfmdock_amd import surface as SF
    assert np.array_equal(got["lig_points"], got["lig_buried"].sum(1)) and np.array_equal(got["rec_points"], got["rec_buried"].sum(1)), label
    rc, lc = np.searchsorted(values, np.asarray(rr, np.float32)), np.searchsorted(values, np.asarray(lr, np.float32))
    for p in range(got["bsa"].shape[0]):
        assert np.array_equal(got["class_points"][p, 0], np.bincount(rc, weights=got["rec_buried"][p], minlength=16).astype(np.int32)), (label, p)
        assert np.array_equal(got["class_points"][p, 1], np.bincount(lc, weights=got["lig_buried"][p], minlength=16).astype(np.int32)), (label, p)
    assert got["bsa"].tobytes() == SF.bsa_from_class_points(got["class_points"], values, probe, K).tobytes(), label


def check_against_definition(model, rec, rr, lig, lr, center, rot, tr, probe=1.4, K=128, label="", chunk_poses=0):
    """One handle, one call with per-atom output, against the definition; returns (poses, near pairs, buried receptor points, buried
    ligand points, border points, result)."""
    from dfmdock_amd import surface as SF
    rec, lig = np.asarray(rec, np.float32).reshape(-1, 3), np.asarray(lig, np.float32).reshape(-1, 3)
    rr, lr = np.asarray(rr, np.float32), np.asarray(lr, np.float32)
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    P = rot.shape[0]
    with model.surface(rec, rr, lig, lr, center, probe, K) as sf:
        info = sf.info()
        got = sf.bsa(rot, tr, per_atom=True, chunk_poses=chunk_poses)
    er, el = SF.exposure(rec, rr, probe, K), SF.exposure(lig, lr, probe, K)
    assert np.array_equal(info["rec_exposed"], er.sum(1)) and np.array_equal(info["lig_exposed"], el.sum(1)), label
    vals = SF.radius_classes(rr, lr)[0]
    assert np.array_equal(info["class_radius"], vals), label
    iso = np.zeros((2, 2, 16), np.int64)
    iso[0, 0] = np.bincount(np.searchsorted(vals, rr), weights=er.sum(1), minlength=16)
    iso[1, 0] = np.bincount(np.searchsorted(vals, lr), weights=el.sum(1), minlength=16)
    assert [info["sasa_rec"], info["sasa_lig"]] == SF.bsa_from_class_points(iso, vals, probe, K).tolist(), label
    assert got["lig_buried"].shape == (P, lig.shape[0]) and got["rec_buried"].dtype == np.int32 and got["bsa"].dtype == np.float64
    check_own_sums(got, rr, lr, vals, probe, K, label)
    n = np.zeros(4, np.int64)
    for p in range(P):
        if not (np.isfinite(rot[p]).all() and np.isfinite(tr[p]).all()):
            assert not got["lig_buried"][p].any() and not got["rec_buried"][p].any() and got["bsa"][p] == 0, (label, p)
            continue
        lm, rm, pairs = SF.pose_margins(rec, rr, lig, lr, center, rot[p], tr[p], probe, K)
        for key, m, ex in (("lig_buried", lm, el), ("rec_buried", rm, er)):
            want, border = (ex & (m < 0)).sum(1), (ex & (np.abs(m) < BORDER)).sum(1)
            off = np.abs(got[key][p] - want)
            assert (off <= border).all(), (label, key, p, np.nonzero(off > border)[0][:5].tolist(), got[key][p][off > border][:5].tolist(), want[off > border][:5].tolist())
            n += [0, 0, 0, border.sum()]
            n[1 if key == "rec_buried" else 2] += want.sum()
        n[0] += pairs
    print(f"{label}: P {P} Ar {rec.shape[0]} Al {lig.shape[0]} K {K} near pairs {n[0]} buried rec {n[1]} lig {n[2]} border {n[3]} "
          f"bsa {got['bsa'].min():.0f} .. {got['bsa'].max():.0f}")
    return P, n[0], n[1], n[2], n[3], got


def test_parity_with_the_definition_on_db5(model):
    """Gate 1.  N, CA, C, O, CB of the first six DB5 backbones with radii 1.55, 1.70, 1.70, 1.52, 1.70, 8 seeded poses each from one
    default_rng(0) stream, K = 128, probe 1.4.  The definition alone gives 48 poses, 25 454 near atom pairs, 20 942 buried
    receptor points and 22 024 buried ligand points (BSA 122 .. 1 708 A^2 per pose) and no border point (counted on the CPU)."""
    rng = np.random.default_rng(0)
    tot = np.zeros(5, np.int64)
    for cid in db5_ids()[:6]:
        c = db5_complex(cid)
        rot, tr = db5_poses(rng, 8)
        rec, lig = five_atoms(c["rec_pos"]), five_atoms(c["lig_pos"])
        tot += check_against_definition(model, rec, radii5(rec), lig, radii5(lig), ca_center(c["lig_pos"]), rot, tr, label=cid)[:5]
    print(f"poses {tot[0]}, near pairs {tot[1]}, buried points receptor {tot[2]} ligand {tot[3]}, border points {tot[4]}")
    assert tot[:4].tolist() == PINNED
    assert tot[4] <= 0.001 * (tot[2] + tot[3])


PINNED = [48, 25454, 20942, 22024]      # poses, near pairs, buried receptor points, buried ligand points


def _ensemble_7cei(P=96, seed=1):
    cx = complex_for("fwd_7CEI_p0")
    rng = np.random.default_rng(seed)
    rot = (0.2 * rng.standard_normal((P, 3))).astype(np.float32)
    tr = (2.0 * rng.standard_normal((P, 3))).astype(np.float32)
    rec, lig = five_atoms(cx["rec_pos"]), five_atoms(cx["lig_pos"])
    return rec, radii5(rec), lig, radii5(lig), ca_center(cx["lig_pos"]), rot, tr


def _same(a, b, keys, label=""):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (label, k)


def test_invariances_are_exact(model):
    """Gate 2."""
    from dfmdock_amd import _lib as L
    from dfmdock_amd import engine
    from dfmdock_amd import surface as SF
    rec, rr, lig, lr, cen, rot, tr = _ensemble_7cei()
    ALL = KEYS + ATOM_KEYS
    with model.surface(rec, rr, lig, lr, cen) as sf, model.surface(rec, rr, lig, lr, cen, points=64) as sf64:
        full = sf.bsa(rot, tr, per_atom=True)
        assert (full["bsa"] > 0).sum() > 48 and full["lig_points"].max() > 100
        parts = [sf.bsa(rot[lo:hi], tr[lo:hi], per_atom=True) for lo, hi in ((0, 31), (31, 32), (32, 96))]
        _same(full, {k: np.concatenate([q[k] for q in parts]) for k in ALL}, ALL, "split")
        perm = np.random.default_rng(2).permutation(96)
        _same({k: full[k][perm] for k in ALL}, sf.bsa(rot[perm], tr[perm], per_atom=True), ALL, "permuted")
        for cp in (1, 7, 96):
            _same(full, sf.bsa(rot, tr, per_atom=True, chunk_poses=cp), ALL, f"chunk {cp}")
            _same(full, sf.bsa(rot, tr, chunk_poses=cp), KEYS, f"chunk {cp}, no per-atom output")
        # any subset of the output pointers NULL
        types = {"lig_buried": C.c_int32, "rec_buried": C.c_int32, "lig_points": C.c_int32, "rec_points": C.c_int32, "class_points": C.c_int32,
                 "bsa": C.c_double}
        f = lambda x: x.ctypes.data_as(L.F32P)
        for mask in range(64):
            out, bufs = L.BsaOutC(), {}
            for b, (k, t) in enumerate(types.items()):
                if mask >> b & 1:
                    bufs[k] = np.full_like(full[k], 7)
                    setattr(out, k, bufs[k].ctypes.data_as(C.POINTER(t)))
            assert L.lib().dfm_pose_bsa(sf._h, 96, f(rot), f(tr), C.byref(out)) == 0, mask
            _same(full, bufs, tuple(bufs), f"pointer mask {mask}")
        # two host threads on the same handle at once
        res, errs = [None, None], []

        def work(i):
            try:
                res[i] = [sf.bsa(rot, tr, per_atom=True, chunk_poses=(0, 5)[i]) for _ in range(3)]
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
                _same(full, r, ALL, "threads")
        # K = 64 next to K = 128: each against its own definition (8 poses)
        h64 = sf64.bsa(rot[:8], tr[:8], per_atom=True)
        info = sf.info()
        assert info["n_cells"] >= 8 and 1 <= info["max_cell_atoms"] <= rec.shape[0] and info["cell_edge"] > 6.2 and info["sasa_rec"] > 0 and info["sasa_lig"] > 0
    for K, got in ((64, h64), (128, {k: full[k][:8] for k in ALL})):
        want = SF.bsa(rec, rr, lig, lr, cen, rot[:8], tr[:8], K=K)
        nb = 0
        er, el = SF.exposure(rec, rr, K=K), SF.exposure(lig, lr, K=K)
        for p in range(8):
            lm, rm, _ = SF.pose_margins(rec, rr, lig, lr, cen, rot[p], tr[p], K=K)
            bl, br = (el & (np.abs(lm) < BORDER)).sum(1), (er & (np.abs(rm) < BORDER)).sum(1)
            assert (np.abs(got["lig_buried"][p] - want["lig_buried"][p]) <= bl).all() and (np.abs(got["rec_buried"][p] - want["rec_buried"][p]) <= br).all(), (K, p)
            nb += bl.sum() + br.sum()
        print(f"K {K}: buried points {want['rec_points'].sum()} + {want['lig_points'].sum()}, border {nb}")
    cp, kn = engine.bsa_last_timing()
    assert cp > 0 and kn > 0


def test_small_shapes(model):
    """Gate 3: sizes and placements at which the kernel takes another path, each against the definition."""
    rng = np.random.default_rng(5)
    zero = np.zeros(3, np.float32)
    poses = lambda P, s_rot=0.5, s_tr=1.5: ((s_rot * rng.standard_normal((P, 3))).astype(np.float32), (s_tr * rng.standard_normal((P, 3))).astype(np.float32))
    C17 = lambda n: np.full(n, 1.7, np.float32)
    # Al around the block size, one receptor atom (Ar = 1)
    for Al in (1, 63, 64, 65, 130):
        lig = (3.0 * rng.standard_normal((Al, 3))).astype(np.float32)
        rot, tr = poses(4)
        r = check_against_definition(model, np.array([[0.5, -0.25, 1.0]], np.float32), C17(1), lig, C17(Al), lig.mean(0), rot, tr, label=f"Ar 1, Al {Al}")
        assert r[2] + r[3] > 0
    # 200 receptor atoms at one point next to one ligand atom: more near pairs than one batch, none of the 200 has an exposed point
    # of its own except where the definition says so; then 640 near pairs of 90 ligand atoms per batch drain the queue
    point = np.tile(np.array([[1.0, 2.0, -0.5]], np.float32), (200, 1))
    r = check_against_definition(model, point, C17(200), np.array([[3.0, 2.5, 0.0]], np.float32), C17(1), zero, *poses(3, 0.3, 0.5), label="200 atoms at one point, Al 1")
    assert r[3] > 0
    lig = (4.0 * rng.standard_normal((90, 3))).astype(np.float32)
    rot, tr = poses(3)
    r = check_against_definition(model, point, C17(200), lig, C17(90), zero, rot, tr, label="200 atoms at one point, Al 90")
    assert r[1] > 1024
    # every receptor atom in one cell
    one_cell = (1.2 * rng.random((150, 3))).astype(np.float32) + np.float32(1.0)
    r = check_against_definition(model, one_cell, C17(150), lig, C17(90), zero, rot, tr, label="one cell, 150 atoms")
    assert r[1] > 1024 and r[2] > 0
    # a ligand outside the receptor's box by more than the largest R_a + R_b (6.2 A): nothing; and by less, on the low side
    rec = (8.0 * rng.random((300, 3))).astype(np.float32)
    lig = (2.0 * rng.random((70, 3))).astype(np.float32)
    far = np.array([[30.0, 0, 0], [0, -25.0, 0], [0, 0, 14.5], [-8.5, -8.5, -8.5]], np.float32)
    r = check_against_definition(model, rec, C17(300), lig, C17(70), lig.mean(0), np.zeros((4, 3), np.float32), far, label="outside by more than the reach")
    assert r[2] == 0 and r[3] == 0 and not r[5]["bsa"].any() and not r[5]["class_points"].any()
    low = np.array([[-5.5, 3.0, 3.0], [3.0, -6.0, 3.0], [3.0, 3.0, -6.5], [-3.5, -3.5, -3.5]], np.float32)
    r = check_against_definition(model, rec, C17(300), lig, C17(70), lig.mean(0), np.zeros((4, 3), np.float32), low, label="outside on the low side by less than the reach")
    assert r[2] > 0 and r[3] > 0
    # an atom with no exposed point (inside a larger neighbour) next to the ligand
    rec = np.array([[0, 0, 0], [0.1, 0, 0], [4.0, 0, 0]], np.float32)
    r = check_against_definition(model, rec, np.float32([1.0, 1.9, 1.7]), np.array([[2.0, 2.0, 0]], np.float32), C17(1), zero, *poses(3, 0.2, 0.5), label="an atom without exposed points")
    assert not r[5]["rec_buried"][:, 0].any() and r[2] > 0
    # 16 radius classes, and one
    rec = (9.0 * rng.random((120, 3))).astype(np.float32)
    lig = (9.0 * rng.random((100, 3))).astype(np.float32) + np.float32(4.0)
    r16 = (1.2 + 0.05 * np.arange(16)).astype(np.float32)
    rot, tr = poses(3, 0.3, 1.0)
    r = check_against_definition(model, rec, r16[np.arange(120) % 16], lig, r16[(np.arange(100) * 7) % 16], lig.mean(0), rot, tr, label="16 radius classes")
    assert (r[5]["class_points"].sum(0) > 0).sum() >= 24
    r = check_against_definition(model, rec, C17(120), lig, C17(100), lig.mean(0), rot, tr, label="one radius class")
    assert not r[5]["class_points"][:, :, 1:].any() and r[5]["class_points"][:, :, 0].all()
    # P = 1; K = 256 and K = 192; a deep overlap in which every exposed ligand point of the overlapped atoms is buried
    cx = complex_for("fwd_7CEI_p0")
    rec, lig = five_atoms(cx["rec_pos"]), five_atoms(cx["lig_pos"])
    cen = ca_center(cx["lig_pos"])
    rot, tr = poses(3, 0.2, 1.0)
    assert check_against_definition(model, rec, radii5(rec), lig, radii5(lig), cen, rot[:1], tr[:1], label="P = 1")[0] == 1
    assert check_against_definition(model, rec, radii5(rec), lig, radii5(lig), cen, rot[:2], tr[:2], K=256, label="K = 256")[3] > 0
    assert check_against_definition(model, rec, radii5(rec), lig, radii5(lig), cen, rot[:2], tr[:2], K=192, probe=1.0, label="K = 192, probe 1.0")[3] > 0
    onto = (rec.astype(np.float64).mean(0) - lig.astype(np.float64).mean(0)).astype(np.float32)
    r = check_against_definition(model, rec, radii5(rec), lig, radii5(lig), cen, rot, onto[None] + np.float32(0.3) * tr, label="deep overlap")
    assert r[3] > 3000
    pt = np.array([[1.0, 2.0, 3.0]], np.float32)
    r = check_against_definition(model, pt, np.float32([1.9]), pt, np.float32([1.52]), zero, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), label="atom on atom")
    assert r[5]["lig_buried"][0, 0] == 128 and r[5]["rec_buried"][0, 0] == 0


def test_non_finite_poses(model):
    """Gate 4."""
    rec, rr, lig, lr, cen, rot, tr = _ensemble_7cei(8, seed=3)
    ALL = KEYS + ATOM_KEYS
    with model.surface(rec, rr, lig, lr, cen) as sf:
        clean = sf.bsa(rot, tr, per_atom=True)
        assert (clean["bsa"] > 0).sum() >= 4
        r2, t2 = rot.copy(), tr.copy()
        r2[2, 1], t2[5, 0], t2[6, 2] = np.nan, np.nan, np.inf
        dirty = sf.bsa(r2, t2, per_atom=True)
    for p in (2, 5, 6):
        assert dirty["bsa"][p] == 0 and dirty["lig_points"][p] == 0 and dirty["rec_points"][p] == 0 and not dirty["class_points"][p].any()
        assert not dirty["lig_buried"][p].any() and not dirty["rec_buried"][p].any()
    keep = np.ones(8, bool)
    keep[[2, 5, 6]] = False
    _same({k: clean[k][keep] for k in ALL}, {k: dirty[k][keep] for k in ALL}, ALL)
    from dfmdock_amd import surface as SF
    want = SF.bsa(rec, rr, lig, lr, cen, r2, t2)
    assert not want["bsa"][[2, 5, 6]].any() and np.abs(want["lig_points"] - dirty["lig_points"]).max() <= 2


def test_invalid_arguments(model):
    """Gate 5: DFM_E_INVALID / NULL, dfm_last_error set, nothing enqueued; create / destroy leaves the block cache's accounting sane."""
    from dfmdock_amd import _lib as L
    from dfmdock_amd import surface as SF
    lib = L.lib()
    rng = np.random.default_rng(4)
    rec, lig = (6.0 * rng.random((40, 3))).astype(np.float32), (6.0 * rng.random((30, 3))).astype(np.float32)
    rr, lr = np.full(40, 1.7, np.float32), np.full(30, 1.55, np.float32)
    cen = lig.mean(0)
    f = lambda x: x.ctypes.data_as(L.F32P)
    dirs = {K: SF.sphere_points(K) for K in (64, 128)}
    d96 = np.zeros((96, 3), np.float32)
    prm = lambda probe=1.4, K=128, d=dirs[128], c=0: C.byref(L.SurfaceParamsC(probe, K, None if d is None else f(d), c))
    nan_rec, nan_lig, inf_cen, nan_rr, neg_lr, nan_dirs = rec.copy(), lig.copy(), cen.copy(), rr.copy(), lr.copy(), dirs[128].copy()
    nan_rec[7, 1], nan_lig[3, 2], inf_cen[0], nan_rr[5], neg_lr[9], nan_dirs[100, 1] = np.nan, np.inf, np.inf, np.nan, -1.0, np.nan
    zero_rr = rr.copy()
    zero_rr[2] = 0.0
    many = (1.0 + 0.01 * np.arange(40)).astype(np.float32)
    wide = rec.copy()
    wide[0] = 3000.0      # about 480^3 cells of 6.2 A > 2^24
    wide_lig = lig.copy()
    wide_lig[0] = 3000.0
    h = model._h
    A = lambda **kw: tuple({**dict(m=h, Ar=40, rec=f(rec), rr=f(rr), Al=30, lig=f(lig), lr=f(lr), cen=f(cen), prm=prm()), **kw}.values())
    cases = [(A(m=None), "m is NULL"), (A(rec=None), "rec_atoms is NULL"), (A(rr=None), "rec_radius is NULL"), (A(lig=None), "lig_atoms is NULL"),
             (A(lr=None), "lig_radius is NULL"), (A(cen=None), "center is NULL"), (A(Ar=0), "Ar >= 1"), (A(Al=0), "Al >= 1"),
             (A(Ar=(1 << 24) + 1), "exceeds 2^24 atoms"), (A(Al=(1 << 24) + 1), "exceeds 2^24 atoms"),
             (A(rec=f(nan_rec)), "rec_atoms: atom 7 is not finite"), (A(lig=f(nan_lig)), "lig_atoms: atom 3 is not finite"),
             (A(cen=f(inf_cen)), "center is not finite"), (A(rr=f(nan_rr)), "rec_radius: atom 5"), (A(lr=f(neg_lr)), "lig_radius: atom 9"),
             (A(rr=f(zero_rr)), "rec_radius: atom 2"), (A(prm=prm(0.0)), "probe must be finite and > 0"), (A(prm=prm(-1.4)), "probe must be finite and > 0"),
             (A(prm=prm(float("nan"))), "probe must be finite and > 0"), (A(prm=prm(float("inf"))), "probe must be finite and > 0"),
             (A(prm=prm(1.4, 0)), "K must be a multiple of 64"), (A(prm=prm(1.4, 96, d96)), "K must be a multiple of 64"),
             (A(prm=prm(1.4, 320)), "K must be a multiple of 64"), (A(prm=prm(1.4, -64)), "K must be a multiple of 64"),
             (A(prm=prm(1.4, 128, nan_dirs)), "dirs is not finite"), (A(prm=prm(1.4, 128, dirs[128], -1)), "chunk_poses must be >= 0"),
             (A(rr=f(many)), "more than 16 radius classes"), (A(rec=f(wide)), "more than 2^24 cells"), (A(lig=f(wide_lig)), "more than 2^24 cells")]
    for args, word in cases:
        assert lib.dfm_surface_create(*args) is None, word
        msg = lib.dfm_last_error().decode()
        print(word, "->", msg)
        assert word in msg, (word, msg)
    lib.dfm_trim_cache(-1)
    for _ in range(20):
        s = lib.dfm_surface_create(h, 40, f(rec), f(rr), 30, f(lig), f(lr), f(cen), None)      # NULL parameters: the defaults
        assert s
        lib.dfm_surface_destroy(s)
    parked = lib.dfm_trim_cache(-1)
    assert 0 < parked <= 11 * 65536 and lib.dfm_trim_cache(-1) == 0      # eleven blocks of one 64 KiB granule, handed on from handle to handle
    s = lib.dfm_surface_create(h, 40, f(rec), f(rr), 30, f(lig), f(lr), f(cen), prm(1.4, 64, None))      # dirs NULL: the library's own table
    rot, tr = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out = L.BsaOutC()
    area = np.zeros(4, np.float64)
    out.bsa = area.ctypes.data_as(C.POINTER(C.c_double))
    o = C.byref(out)
    for args, word in [((None, 4, f(rot), f(tr), o), "s is NULL"), ((s, 4, None, f(tr), o), "rot is NULL"), ((s, 4, f(rot), None, o), "tr is NULL"),
                       ((s, 4, f(rot), f(tr), None), "out is NULL"), ((s, 0, f(rot), f(tr), o), "P >= 1")]:
        assert lib.dfm_pose_bsa(*args) == -1, word
        assert word in lib.dfm_last_error().decode(), word
    assert lib.dfm_pose_bsa_chunked(s, 4, f(rot), f(tr), -1, o) == -1 and "chunk_poses" in lib.dfm_last_error().decode()
    assert lib.dfm_bsa_last_timing(None, None) == -1 and lib.dfm_surface_info(None, *([None] * 9)) == -1
    assert lib.dfm_pose_bsa(s, 4, f(rot), f(tr), o) == 0 and (area == area[0]).all() and area[0] > 0      # the handle still works
    lib.dfm_surface_destroy(s)
    lib.dfm_surface_destroy(None)
    with pytest.raises(ValueError):
        model.surface(rec, rr, lig, lr, cen, probe=0.0)
    with pytest.raises(ValueError):
        model.surface(rec, rr, lig, lr, cen, points=100)
    with pytest.raises(ValueError):
        model.surface(rec, rr[:5], lig, lr, cen)
    with pytest.raises(ValueError):
        model.surface(rec, many, lig, lr, cen)


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def _write_sticky_ckpt(path):
    """cli_fixtures.write_ckpt's file with weights.make_sticky_weights: the draw whose free runs end in contact (with the seeded
    random-init draws the ligand leaves for good and every pose buries 0 A^2)."""
    import torch
    from dfmdock_amd.weights import HParams, make_sticky_weights
    hp = HParams()
    w = make_sticky_weights()
    hyper = {"model": {"lm_embed_dim": hp.lm_embed_dim, "positional_embed_dim": hp.positional_embed_dim, "spatial_embed_dim": 100,
                       "node_dim": 256, "edge_dim": 128, "inner_dim": 128, "depth": hp.depth, "cut_off": hp.cut_off},
             "diffuser": {"r3": {"min_sigma": 0.1, "max_sigma": 30.0}, "so3": {"min_sigma": 0.1, "max_sigma": 1.5}}}
    torch.save({"state_dict": {"net." + k: torch.from_numpy(v.copy()) for k, v in w.items()}, "hyper_parameters": hyper, "epoch": 3}, path)
    return w


def test_drivers_and_cli(model, tmp_path):
    """Gate 6, on 7CEI with the checkpoint whose free runs end in contact.  Without the new flags `dock` writes what dock_pair without
    options writes; --bsa adds the areas, which equal Surface.bsa on the written models' poses bit for bit; --min-bsa drops the models
    below the threshold and says how many, alone and next to --clash-filter; --interface-residues sums to the kept pose's two sides."""
    from cli_fixtures import golden_7cei, write_pair
    from dfmdock_amd import cli, driver, engine
    from dfmdock_amd.weights import pack_blob
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    sticky = engine.Model(pack_blob(_write_sticky_ckpt(ck)))
    base = [rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--seed", "3", "--max-batch", "16", "--no-selfcheck", "--num-samples", "16",
            "--num-steps", "40"]
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    pdb = lambda name: open(tmp_path / name, "rb").read()
    # the default is untouched: the same files and the same line as dock_pair without options
    p0 = _run(["dock"] + base + ["--out", "plain.pdb", "--top-k", "8", "--cluster-radius", "1.0"], cwd=str(tmp_path))
    assert p0.returncode == 0, p0.stdout + p0.stderr
    plain = json.loads(p0.stdout.strip().splitlines()[-1])
    kw = dict(num_samples=16, num_steps=40, seed=3, max_batch=16, selfcheck=False, top_k=8, cluster_radius=1.0)
    d0 = driver.dock_pair(sticky, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api.pdb"), **kw)
    assert pdb("plain.pdb") == pdb("api.pdb") and plain["energy"] == d0["energy"] and not any(k.startswith("bsa") for k in list(plain) + list(d0))
    assert [m["index"] for m in plain["models"]] == [m["index"] for m in d0["models"]] and not any("bsa" in m for m in plain["models"])
    # --bsa: the areas of the line and of every model; nothing else moves
    p1 = _run(["dock"] + base + ["--out", "bsa.pdb", "--top-k", "8", "--cluster-radius", "1.0", "--bsa", "--interface-residues", "iface.txt"], cwd=str(tmp_path))
    assert p1.returncode == 0, p1.stdout + p1.stderr
    line = json.loads(p1.stdout.strip().splitlines()[-1])
    assert {k: v for k, v in line.items() if k in plain and k not in ("output", "models")} == {k: v for k, v in plain.items() if k not in ("output", "models")}
    assert pdb("bsa.pdb") == pdb("plain.pdb") and len(line["models"]) == len(plain["models"]) >= 2
    d1 = driver.dock_pair(sticky, rec, lig, rec_x, lig_x, out_pdb=None, bsa=True, **kw)
    traj = d1["trajectories"]
    ra, rr, la, lr, cen = driver.surface_inputs(rec, lig, 0)
    with sticky.surface(ra, rr, la, lr, cen) as sf:
        want = sf.bsa(traj["rot_update"], traj["tr_update"], per_atom=True)
    _same(want, d1["bsa_data"], KEYS)
    print("bsa of the 16 trajectories:", np.round(want["bsa"]).tolist())
    k = line["index"]
    assert (line["bsa"], line["bsa_rec"], line["bsa_lig"]) == (want["bsa"][k], want["bsa_rec"][k], want["bsa_lig"][k]) and (line["probe"], line["sphere_points"]) == (float(np.float32(1.4)), 128)
    for m, m0 in zip(line["models"], plain["models"]):
        assert {k: v for k, v in m.items() if k in m0 and k != "path"} == {k: v for k, v in m0.items() if k != "path"}
        assert (m["bsa"], m["bsa_rec"], m["bsa_lig"]) == (want["bsa"][m["index"]], want["bsa_rec"][m["index"]], want["bsa_lig"][m["index"]])
        assert pdb(os.path.basename(m["path"])) == pdb(os.path.basename(m0["path"]))
    rows = [l.split() for l in (tmp_path / "iface.txt").read_text().splitlines()[1:]]
    for side, total in (("rec", line["bsa_rec"]), ("lig", line["bsa_lig"])):
        got = sum(float(r[3]) for r in rows if r[0] == side)
        n = sum(r[0] == side for r in rows)
        assert abs(got - total) <= 0.005 * n + 1e-6 and (n > 0) == (total > 0)      # every line is rounded to 0.01 A^2
    # --min-bsa with a threshold between the models' areas: some go, not all
    areas = sorted(m["bsa"] for m in line["models"])
    print("model areas", areas)
    assert areas[0] < areas[-1]
    thr = 0.5 * (areas[0] + areas[-1])
    p2 = _run(["dock"] + base + ["--out", "min.pdb", "--top-k", "8", "--cluster-radius", "1.0", "--min-bsa", repr(thr)], cwd=str(tmp_path))
    assert p2.returncode == 0, p2.stdout + p2.stderr
    l2 = json.loads(p2.stdout.strip().splitlines()[-1])
    kept = [m for m in line["models"] if m["bsa"] >= thr]
    assert l2["min_bsa"] == thr and 0 < len(l2["models"]) < len(line["models"]) and l2["bsa_dropped"] == len(line["models"]) - len(kept)
    assert [m["index"] for m in l2["models"]] == [m["index"] for m in kept] and [m["rank"] for m in l2["models"]] == list(range(1, len(kept) + 1))
    assert [m["bsa"] for m in l2["models"]] == [m["bsa"] for m in kept] and l2["energy"] == plain["energy"] and pdb("min.pdb") == pdb("plain.pdb")
    for m in l2["models"]:      # the files are renumbered with the models
        assert pdb(os.path.basename(m["path"])) == pdb(f"bsa_{[q['index'] for q in line['models']].index(m['index']) + 1}.pdb")
    # next to --clash-filter: no model is flagged, none buries less than the threshold
    d3 = driver.dock_pair(sticky, rec, lig, rec_x, lig_x, out_pdb=None, min_bsa=thr, clash_filter=True, **kw)
    flags = d3["sterics_data"]["flags"]
    assert "bsa_dropped" in d3 and d3["sterics"]["filtered"] and all(m["bsa"] >= thr and not flags[m["index"]] for m in d3["models"])
    assert all(m["bsa"] == want["bsa"][m["index"]] for m in d3["models"])
    # refine takes the options too
    r = driver.refine_pair(model, rec, lig, rec_x, lig_x, t_begin=0.05, num_samples=4, num_steps=3, seed=1, max_batch=4, selfcheck=False, out_pdb=None,
                           bsa=True, sphere_points=64)
    assert r["sphere_points"] == 64 and r["bsa"] == r["bsa_data"]["bsa"][r["index"]] and r["bsa_data"]["bsa"].shape == (4,)
    sticky.close()
