"""Cryo-EM density fit on the GPU (dfm_density_create, dfm_pose_density, kernels_density.hip) against the float64 definition
dfmdock_amd/density.py, and through the drivers and the command line.

Every result is an integer: a count, or a sum of terms rounded to quanta of 2^-20.  A term is found from fp64 +, -, * and / in a fixed
order on both sides, nothing contracted, so the device's integers must EQUAL the definition's: sum_q, n_inside, n_above and atom_q, with
no tolerance anywhere."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, db5_complex, db5_ids

pytestmark = pytest.mark.gpu

KEYS = ("sum_q", "n_inside", "n_above")
ALL_KEYS = KEYS + ("atom_q",)


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def check_against_definition(model, grids, origin, voxel, lig, w, center, rot, tr, threshold=1.0, label="", chunk_poses=0):
    """One handle, one call with every output and one without atom_q: integer equality with the definition on all four arrays, and the
    call's own identity sum_q[:, 0] == atom_q.sum(1).  Returns (the definition's result, the device's)."""
    from dfmdock_amd import density as DN
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    with model.density(grids, origin, voxel, lig, w, center, threshold) as h:
        got = h.fit(rot, tr, per_atom=True, chunk_poses=chunk_poses)
        lean = h.fit(rot, tr, chunk_poses=chunk_poses)
        info = h.info()
    want = DN.density(grids, origin, voxel, lig, w, center, rot, tr, threshold, per_atom=True)
    g = np.asarray(grids, np.float32)
    g = g[None] if g.ndim == 3 else g
    P, Al, Cn = rot.shape[0], np.asarray(lig).reshape(-1, 3).shape[0], g.shape[0]
    assert got["sum_q"].shape == (P, Cn) and got["atom_q"].shape == (P, Al) and got["sum_q"].dtype == got["atom_q"].dtype == np.int64
    assert got["n_inside"].dtype == got["n_above"].dtype == np.int32 and "atom_q" not in lean
    assert (info["nx"], info["ny"], info["nz"], info["C"]) == (g.shape[3], g.shape[2], g.shape[1], Cn) and info["sum_bound"] == Al * 2.0 ** 37
    assert np.array_equal(got["sum_q"][:, 0], got["atom_q"].sum(1)), label
    for k in ALL_KEYS:
        off = got[k] != want[k]
        assert not off.any(), (label, k, int(off.sum()), got[k][off][:5].tolist(), want[k][off][:5].tolist())
    for k in KEYS:
        assert np.array_equal(lean[k], want[k]), (label, k, "without atom_q")
    assert np.abs(want["sum_q"]).max() <= info["sum_bound"]
    print(f"{label}: P {P} Al {Al} C {Cn} grid {g.shape[1:]} inside {int(want['n_inside'].sum())} above {int(want['n_above'].sum())} "
          f"sum {want['sum_q'].sum(0) / 2.0 ** 20}")
    return want, got


def poses(rng, P, angle=0.4, shift=1.0):
    """Pose 0 is the identity (its draws are still consumed)."""
    rot, tr = (angle * rng.standard_normal((P, 3))).astype(np.float32), (shift * rng.standard_normal((P, 3))).astype(np.float32)
    rot[0], tr[0] = 0.0, 0.0
    return rot, tr


def test_small_shapes(model):
    """The smallest sizes and placements at which each path of the kernel can break, each against the definition."""
    rng = np.random.default_rng(5)
    # 2 x 2 x 2 and [nz,ny,nx] = 3 x 5 x 4, anisotropic voxels, a negative origin; C = 1, 3, 4; every block shape; P = 1, 2, 5 in chunks of 2
    boxes = [((2, 2, 2), np.float32([-3.0, 0.5, -1.0]), np.float32([2.0, 0.75, 1.5])), ((3, 5, 4), np.float32([-2.0, -4.0, 1.0]), np.float32([0.5, 1.25, 3.0]))]
    inside_total = 0
    for shape, origin, voxel in boxes:
        ext = voxel.astype(np.float64) * (np.array(shape[::-1]) - 1)
        for Cn in (1, 3, 4):
            grids = rng.uniform(-6.0, 6.0, (Cn,) + shape).astype(np.float32)
            for Al in (1, 63, 64, 65, 130):
                lig = (origin + ext * rng.uniform(-0.15, 1.15, (Al, 3))).astype(np.float32)      # about a quarter of the atoms start outside
                w = rng.uniform(-8.0, 8.0, Al).astype(np.float32)
                for P in (1, 2, 5):
                    rot, tr = poses(rng, P, 0.3, 0.3)
                    want, _ = check_against_definition(model, grids, origin, voxel, lig, w, lig.mean(0), rot, tr, 0.5, label=f"grid {shape} C {Cn} Al {Al} P {P}", chunk_poses=2)
                    inside_total += int(want["n_inside"].sum())
    assert inside_total > 5000
    # planted atoms under the identity about a centre of zero - the posed atom IS the float32 atom: on nodes, on the faces of the box, one
    # float32 ulp inside and outside each face, and entirely outside
    shape, origin, voxel = boxes[1]
    grids = rng.uniform(-6.0, 6.0, (3,) + shape).astype(np.float32)
    lo, hi = origin, (origin + voxel * (np.array(shape[::-1], np.float32) - 1)).astype(np.float32)      # exact: small binary fractions
    mid = ((lo + hi) / 2).astype(np.float32)
    planted, expect = [], []
    for iz in range(shape[0]):
        for ix in range(shape[2]):
            planted.append([lo[0] + voxel[0] * ix, lo[1] + voxel[1] * 2, lo[2] + voxel[2] * iz])      # nodes: the last of an axis is outside
            expect.append(ix < shape[2] - 1 and iz < shape[0] - 1)
    for k in range(3):
        for val, ok in ((lo[k], True), (np.nextafter(lo[k], np.float32(-np.inf)), False), (np.nextafter(lo[k], np.float32(np.inf)), True),
                        (hi[k], False), (np.nextafter(hi[k], np.float32(-np.inf)), True), (np.nextafter(hi[k], np.float32(np.inf)), False)):
            p = mid.copy()
            p[k] = val
            planted.append(p)
            expect.append(ok)
    planted += [[lo[0] - 50, mid[1], mid[2]], [mid[0], hi[1] + 1e6, mid[2]], [1e30, -1e30, 1e30], [-3e38, 0, 0]]
    expect += [False] * 4
    planted = np.asarray(planted, np.float32)
    w = rng.uniform(1.0, 8.0, planted.shape[0]).astype(np.float32)
    zero = np.zeros((1, 3), np.float32)
    want, got = check_against_definition(model, grids, origin, voxel, planted, w, [0, 0, 0], zero, zero, 0.0, label="planted atoms")
    assert got["n_inside"][0] == sum(expect) and (got["atom_q"][0][~np.array(expect)] == 0).all()
    from dfmdock_amd import density as DN
    assert DN.interpolate(grids, origin, voxel, planted.astype(np.float64))[1].tolist() == expect
    # every atom outside: zeros, and the wave adds nothing
    far = (planted[:5] + np.float32([500, 0, 0])).astype(np.float32)
    want, _ = check_against_definition(model, grids, origin, voxel, far, w[:5], [0, 0, 0], *poses(rng, 3), label="all outside")
    assert not want["n_inside"].any() and not want["sum_q"].any()
    # the limits themselves: values of 2^10 and weights of 2^7 on every node give terms of exactly 2^37
    full = np.full((1, 2, 2, 2), 1024.0, np.float32)
    want, _ = check_against_definition(model, full, [0, 0, 0], [16, 16, 16], np.float32([[8, 8, 8], [1, 2, 3]]), np.float32([128, -128]), [0, 0, 0], zero, zero, 1024.0, label="limits")
    assert want["atom_q"][0].tolist() == [1 << 37, -(1 << 37)] and want["n_above"][0] == 2


def _ensemble(seed=2, P=12, Al=200, Cn=3):
    rng = np.random.default_rng(seed)
    shape, origin, voxel = (9, 12, 10), np.float32([-3.0, 2.0, -5.0]), np.float32([1.5, 1.0, 2.0])
    grids = rng.uniform(-4.0, 4.0, (Cn,) + shape).astype(np.float32)
    ext = voxel * (np.array(shape[::-1], np.float32) - 1)
    lig = (origin + ext * rng.uniform(0.05, 0.95, (Al, 3))).astype(np.float32)
    w = rng.uniform(-8.0, 8.0, Al).astype(np.float32)
    rot, tr = poses(rng, P, 0.3, 1.5)
    return grids, origin, voxel, lig, w, lig.mean(0), rot, tr


def _same(a, b, keys, label=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)


def test_invariances_are_exact(model):
    """Bitwise: the order of the poses, the chunks of a call, atom_q asked for or not, the order of the atoms."""
    grids, origin, voxel, lig, w, cen, rot, tr = _ensemble()
    P, Al = rot.shape[0], lig.shape[0]
    want, full = check_against_definition(model, grids, origin, voxel, lig, w, cen, rot, tr, 0.25, label="ensemble")
    assert (want["n_inside"] > 0).all() and (want["n_inside"] < Al).any() and 0 < want["n_above"].sum() < want["n_inside"].sum()
    rng = np.random.default_rng(9)
    with model.density(grids, origin, voxel, lig, w, cen, 0.25) as h:
        perm = rng.permutation(P)
        got = h.fit(rot[perm], tr[perm], per_atom=True)
        _same({k: full[k][perm] for k in ALL_KEYS}, got, ALL_KEYS, "poses permuted")
        for chunk in (1, 5, P, P + 7):
            _same(full, h.fit(rot, tr, per_atom=True, chunk_poses=chunk), ALL_KEYS, f"chunks of {chunk}")
            _same(full, h.fit(rot, tr, chunk_poses=chunk), KEYS, f"chunks of {chunk}, no atom_q")
        one = h.fit(rot[7:8], tr[7:8], per_atom=True)
        _same({k: full[k][7:8] for k in ALL_KEYS}, one, ALL_KEYS, "a pose alone")
    aperm = rng.permutation(Al)
    with model.density(grids, origin, voxel, lig[aperm], w[aperm], cen, 0.25) as h:
        got = h.fit(rot, tr, per_atom=True)
    _same(full, got, KEYS, "atoms permuted")
    assert np.array_equal(got["atom_q"], full["atom_q"][:, aperm])
    # a channel alone gives that channel's sums
    with model.density(grids[1], origin, voxel, lig, w, cen, 0.25) as h:
        assert np.array_equal(h.fit(rot, tr)["sum_q"][:, 0], full["sum_q"][:, 1])


def five_atoms(bb):
    from dfmdock_amd import pdbio
    return pdbio.full_backbone(bb).reshape(-1, 3)


def test_realistic_case_on_db5(model):
    """N, CA, C, O, CB of one DB5 complex weighted by atomic number, the map of its native pose at 8 A on a 2 A grid, 256 poses from
    dfm_sample with the seeded weights: the four arrays equal the definition's, and so does density_cc."""
    from dfmdock_amd import density as DN
    from dfmdock_amd import engine
    c = db5_complex(db5_ids()[0])
    rec, lig = five_atoms(c["rec_pos"]).astype(np.float32), five_atoms(c["lig_pos"]).astype(np.float32)
    z = np.float32([7, 6, 6, 8, 6])
    rw, lw = np.tile(z, rec.shape[0] // 5), np.tile(z, lig.shape[0] // 5)
    cen = np.asarray(c["lig_pos"], np.float64)[:, 1].mean(0).astype(np.float32)
    gx = engine.Complex(model, c["rec_x"], c["lig_x"], c["rec_pos"], c["lig_pos"])
    r = gx.sample(B=256, num_steps=4, seed=6, mfma16=True)
    gx.close()
    rot, tr = r["rot_update"].copy(), r["tr_update"].copy()
    rot[0], tr[0] = 0.0, 0.0      # the native pose among them
    both = np.concatenate([rec, lig]).astype(np.float64)
    voxel, sigma = np.float32([2, 2, 2]), 8.0 * DN.SIGMA_FACTOR
    origin = np.floor(both.min(0) - 10.0).astype(np.float32)
    shape = tuple(int(n) + 1 for n in np.ceil((both.max(0) + 10.0 - origin) / 2.0)[::-1])
    dmap = {"grid": DN.simulate_map(both, np.concatenate([rw, lw]), sigma, shape, origin, voxel).astype(np.float32), "origin": origin, "voxel": voxel}
    grids, sc = DN.channels(dmap, rec, rw, sigma, lig, lw)
    want, got = check_against_definition(model, grids, origin, voxel, lig, lw, cen, rot, tr, 1.0, label=c["id"])
    cc, cc_dev = DN.correlation(want["sum_q"], sc), DN.correlation(got["sum_q"], sc)
    assert np.array_equal(cc, cc_dev, equal_nan=True) and np.isfinite(cc).all() and int(np.argmax(cc)) == 0
    assert want["n_inside"][0] == lig.shape[0] and (want["n_inside"] < lig.shape[0]).any() and want["n_inside"].sum() > 256
    print(f"{c['id']}: Al {lig.shape[0]} grid {shape} cc {cc.min():.4f} .. {cc.max():.4f}, native {cc[0]:.4f}, poses with atoms outside "
          f"{int((want['n_inside'] < lig.shape[0]).sum())}")


def test_nan_poses(model):
    from dfmdock_amd import density as DN
    grids, origin, voxel, lig, w, cen, rot, tr = _ensemble(seed=3, P=8)
    with model.density(grids, origin, voxel, lig, w, cen, 0.25) as h:
        clean = h.fit(rot, tr, per_atom=True)
        assert (clean["n_inside"] > 0).all()
        r2, t2 = rot.copy(), tr.copy()
        r2[2, 1] = np.nan
        t2[5, 0] = np.inf
        r2[6, 2] = -np.inf
        dirty = h.fit(r2, t2, per_atom=True, chunk_poses=3)
        lean = h.fit(r2, t2, chunk_poses=3)
    for p in (2, 5, 6):
        assert not any(dirty[k][p].any() for k in ALL_KEYS) and not any(lean[k][p].any() for k in KEYS)
    keep = np.ones(8, bool)
    keep[[2, 5, 6]] = False
    _same({k: clean[k][keep] for k in ALL_KEYS}, {k: dirty[k][keep] for k in ALL_KEYS}, ALL_KEYS)
    want = DN.density(grids, origin, voxel, lig, w, cen, r2, t2, 0.25, per_atom=True)
    for k in ALL_KEYS:
        assert np.array_equal(want[k], dirty[k]), k


def test_invalid_arguments(model):
    """DFM_E_INVALID / NULL, dfm_last_error set, *err set, nothing enqueued, in the order the header gives; the handle still works
    afterwards."""
    from dfmdock_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(4)
    shape = (3, 5, 4)
    grids = rng.uniform(-2, 2, (2,) + shape).astype(np.float32)
    origin, voxel, cen = np.float32([0, 0, 0]), np.float32([1, 1, 1]), np.float32([1, 1, 1])
    lig, w = rng.uniform(0, 2, (30, 3)).astype(np.float32), rng.uniform(1, 8, 30).astype(np.float32)
    f = lambda x: None if x is None else x.ctypes.data_as(L.F32P)
    keep = []      # the arrays behind the pointers of one call
    err = C.c_int(0)

    def create(m=model._h, nx=4, ny=5, nz=3, origin=origin, voxel=voxel, Cn=2, grids=grids, Al=30, lig=lig, w=w, cen=cen, thr=1.0):
        a = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (origin, voxel, grids, lig, w, cen)]
        keep.append(a)
        err.value = 99
        return lib.dfm_density_create(m, nx, ny, nz, f(a[0]), f(a[1]), Cn, f(a[2]), Al, f(a[3]), f(a[4]), f(a[5]), thr, C.byref(err))

    def mod(a, k, v):
        b = np.array(a, copy=True)
        b[k] = v
        return b
    cases = [(dict(m=None), "m is NULL"), (dict(Cn=0), "need 1 <= C <= 4"), (dict(Cn=5), "need 1 <= C <= 4"), (dict(nx=1), "need 2 <= nx <= 1024"),
             (dict(ny=1025), "need 2 <= ny <= 1024"), (dict(nz=0), "need 2 <= nz <= 1024"), (dict(origin=None), "origin is NULL"), (dict(voxel=None), "voxel is NULL"),
             (dict(grids=None), "grids is NULL"), (dict(origin=mod(origin, 1, np.nan)), "origin is not finite"), (dict(voxel=mod(voxel, 0, 0.0)), "voxel is not in (0, 16]"),
             (dict(voxel=mod(voxel, 2, 16.5)), "voxel is not in (0, 16]"), (dict(voxel=mod(voxel, 1, -1.0)), "voxel is not in (0, 16]"),
             (dict(grids=mod(grids, (1, 2, 4, 3), np.nan)), "grids: value 119 is not in [-1024, 1024]"), (dict(grids=mod(grids, (0, 0, 0, 1), -1024.5)), "grids: value 1 is not in"),
             (dict(grids=mod(grids, (0, 0, 0, 0), np.inf)), "grids: value 0 is not in"),
             (dict(lig=None), "lig_atoms is NULL"), (dict(w=None), "lig_w is NULL"), (dict(cen=None), "center is NULL"), (dict(Al=0), "need Al >= 1"),
             (dict(Al=(1 << 24) + 1), "Al exceeds 2^24 atoms"), (dict(lig=mod(lig, (3, 2), np.inf)), "lig_atoms: atom 3 is not finite"),
             (dict(w=mod(w, 7, np.nan)), "lig_w: weight 7 is not in [-128, 128]"), (dict(w=mod(w, 0, 128.5)), "lig_w: weight 0 is not in [-128, 128]"),
             (dict(cen=mod(cen, 0, np.inf)), "center is not finite"), (dict(thr=float("nan")), "threshold is not finite"), (dict(thr=float("inf")), "threshold is not finite")]
    for kw, word in cases:
        assert create(**kw) is None, word
        msg = lib.dfm_last_error().decode()
        print(word, "->", msg)
        assert word in msg and err.value == -1, (word, msg, err.value)
    # the order: the grid before the atoms before the threshold
    assert create(Cn=9, lig=None, thr=float("nan")) is None and "need 1 <= C" in lib.dfm_last_error().decode()
    assert create(grids=mod(grids, (0, 0, 0, 0), np.nan), w=None) is None and "grids: value 0" in lib.dfm_last_error().decode()
    assert create(w=mod(w, 2, 200.0), thr=float("nan")) is None and "lig_w: weight 2" in lib.dfm_last_error().decode()
    keep.clear()
    a = create(voxel=np.float32([16, 16, 16]), grids=mod(mod(grids, (0, 0, 0, 0), 1024.0), (1, 2, 4, 3), -1024.0), w=mod(w, 0, -128.0))      # the limits themselves are fine
    assert a and err.value == 0
    lib.dfm_density_destroy(a)
    a = create()
    assert a and err.value == 0
    b2 = lib.dfm_density_create(model._h, 4, 5, 3, f(origin), f(voxel), 2, f(grids), 30, f(lig), f(w), f(cen), 1.0, None)      # err may be NULL
    assert b2
    lib.dfm_density_destroy(b2)
    nx, ch, b = C.c_int32(0), C.c_int32(0), C.c_double(0)
    assert lib.dfm_density_info(a, C.byref(nx), None, None, None, C.byref(ch), C.byref(b)) == 0 and (nx.value, ch.value, b.value) == (4, 32768, 30 * 2.0 ** 37)
    rot, tr = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out = L.DensityOutC()
    n_inside = np.zeros(4, np.int32)
    out.n_inside = n_inside.ctypes.data_as(L.I32P)
    o = C.byref(out)
    for args, word in [((None, 4, f(rot), f(tr), o), "h is NULL"), ((a, 4, None, f(tr), o), "rot is NULL"), ((a, 4, f(rot), None, o), "tr is NULL"),
                       ((a, 4, f(rot), f(tr), None), "out is NULL"), ((a, 0, f(rot), f(tr), o), "P >= 1")]:
        assert lib.dfm_pose_density(*args) == -1, word
        assert word in lib.dfm_last_error().decode(), word
    assert lib.dfm_pose_density_chunked(a, 4, f(rot), f(tr), -1, o) == -1 and "chunk_poses" in lib.dfm_last_error().decode()
    assert lib.dfm_density_last_timing(None, None) == -1 and lib.dfm_density_info(None, None, None, None, None, None, None) == -1
    assert lib.dfm_pose_density(a, 4, f(rot), f(tr), o) == 0 and (n_inside == n_inside[0]).all() and n_inside[0] > 0      # the handle still works
    cp, km = C.c_double(-1), C.c_double(-1)
    assert lib.dfm_density_last_timing(C.byref(cp), C.byref(km)) == 0 and cp.value >= 0 and km.value > 0
    lib.dfm_density_destroy(a)
    lib.dfm_density_destroy(None)
    for bad in (dict(grids=np.zeros((5,) + shape)), dict(voxel=[1, 17, 1]), dict(w=w[:-1]), dict(cen=cen[:2]), dict(grids=np.full((2, 2, 2), 2000.0))):
        kw = dict(dict(grids=grids, origin=origin, voxel=voxel, lig=lig, w=w, cen=cen), **bad)
        with pytest.raises(ValueError):
            model.density(kw["grids"], kw["origin"], kw["voxel"], kw["lig"], kw["w"], kw["cen"])


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
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "density_alloc_child.py"), out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=60)
        assert p.returncode == 0, f"{tag}: exit {p.returncode}\n" + p.stdout.decode(errors="replace")[-2000:]
        runs[tag] = dict(np.load(out, allow_pickle=False))
    ref = runs["default"]
    assert len([k for k in ref if not k.startswith("__")]) == 7 and ref["full/n_inside"].min() > 0 and np.array_equal(ref["full/sum_q"][:, 0], ref["full/atom_q"].sum(1))
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
    """On 7CEI with the seeded checkpoint and the map of its input pose at 8 A.  Without the new flags `dock` writes what dock_pair without
    options writes and its line has no new key; under --rank density the kept pose is the argmax of the correlation recomputed by the
    definition over every trajectory; --density-residues and --write-simulated-map hold the definition's numbers; `rescore` of the same
    poses keeps the same one."""
    from cli_fixtures import write_ckpt
    from test_density_cpu import native_map_7cei
    from dfmdock_amd import driver
    from dfmdock_amd import density as DN
    from dfmdock_amd import sterics as ST
    f = native_map_7cei(tmp_path)
    rec, lig, rec_x, lig_x = f["rec"], f["lig"], f["rec_x"], f["lig_x"]
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    common = [f["rec_pdb"], f["lig_pdb"], "--ckpt", ck, "--features", f["feat"], "--seed", "3", "--max-batch", "8", "--no-selfcheck"]
    base = common + ["--num-samples", "8", "--num-steps", "6"]
    pdb = lambda name: open(tmp_path / name, "rb").read()
    kw = dict(num_samples=8, num_steps=6, seed=3, max_batch=8, selfcheck=False)
    # the default is untouched
    p0 = _run(["dock"] + base + ["--out", "plain.pdb"], cwd=str(tmp_path))
    assert p0.returncode == 0, p0.stdout + p0.stderr
    plain = json.loads(p0.stdout.strip().splitlines()[-1])
    d0 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api.pdb"), **kw)
    assert pdb("plain.pdb") == pdb("api.pdb") and plain["energy"] == d0["energy"]
    assert set(plain) == {"energy", "output", "num_samples", "precision", "rot_update", "tr_update", "selfcheck_ok"}
    assert "density" not in d0 and "index" not in d0 and "trajectories" not in d0
    # --rank density against the definition over every trajectory
    p2 = _run(["dock"] + base + ["--out", "rank.pdb", "--density", f["path"], "--density-resolution", "8", "--rank", "density", "--top-k", "3",
                                 "--density-residues", "res.txt", "--write-simulated-map", "sim.mrc"], cwd=str(tmp_path))
    assert p2.returncode == 0, p2.stdout + p2.stderr
    ranked = json.loads(p2.stdout.strip().splitlines()[-1])
    d2 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api_rank.pdb"), rank="density", density_map=f["path"], density_resolution=8.0,
                          top_k=3, **kw)
    tj = d2["trajectories"]
    grids, sc = DN.channels(f["map"], f["ra"], f["rw"], f["sigma"], f["la"], f["lw"])
    want = DN.density(grids, f["map"]["origin"], f["map"]["voxel"], f["la"], f["lw"], f["cen"], tj["rot_update"], tj["tr_update"], 1.0, per_atom=True)
    for k in KEYS:
        assert np.array_equal(want[k], d2["density_data"][k]), k
    cc = DN.correlation(want["sum_q"], sc)
    assert np.array_equal(cc, d2["density_data"]["cc"], equal_nan=True) and np.isfinite(cc).any()
    k = int(np.nanargmax(cc))
    Al = f["la"].shape[0]
    print("cc", cc.tolist(), "kept", k, "energy pick", int(np.argmin(tj["energy"])), "inside", want["n_inside"].tolist())
    assert d2["index"] == k == ranked["index"] and pdb("rank.pdb") == pdb("api_rank.pdb")
    obj = lambda p: {"density_cc": float(cc[p]) if np.isfinite(cc[p]) else None, "density_inclusion": float(want["n_above"][p] / Al), "density_n_outside": int(Al - want["n_inside"][p])}
    assert {x: ranked["density"][x] for x in obj(k)} == obj(k) == {x: d2["density"][x] for x in obj(k)}
    assert ranked["density"]["rank"] == 1 and ranked["density"]["resolution"] == 8.0 and ranked["density"]["sigma"] == f["sigma"] and ranked["density"]["threshold"] == 1.0
    assert np.array_equal(np.float32(ranked["rot_update"]), tj["rot_update"][k])
    models = ranked["models"]
    assert len(models) >= 1 and models[0]["index"] == k and all({x: m[x] for x in obj(0)} == obj(m["index"]) for m in models)
    ccs = [m["density_cc"] for m in models]
    assert ccs == sorted(ccs, reverse=True) and all(os.path.exists(m["path"]) for m in models)
    # --density-residues: the definition's per-atom terms of the kept pose and the models, the mean per ligand residue
    idx = [k] + [m["index"] for m in models]
    keys, res = ST.residue_of_atoms(lig["atoms"], ST.heavy_atoms(lig["atoms"]))
    mean = DN.units(DN.residue_density(want["atom_q"][idx], res, len(keys)).sum(0)) / (np.bincount(res, minlength=len(keys)) * len(idx))
    DN.write_density_residues(str(tmp_path / "want.txt"), keys, mean)
    assert pdb("res.txt") == pdb("want.txt") and len(pdb("res.txt").splitlines()) == 1 + len(keys)
    # --write-simulated-map: the kept model on the map's grid
    sim = DN.read_mrc(str(tmp_path / "sim.mrc"))
    posed = ST.pose_atoms(f["la"], f["cen"], tj["rot_update"][k], tj["tr_update"][k])
    ref = DN.simulate_map(np.concatenate([f["ra"].astype(np.float64), posed]), np.concatenate([f["rw"], f["lw"]]), f["sigma"], f["map"]["grid"].shape, f["map"]["origin"],
                          f["map"]["voxel"])
    assert np.array_equal(sim["origin"], f["map"]["origin"]) and sim["grid"].shape == f["map"]["grid"].shape
    np.testing.assert_allclose(sim["grid"], ref, rtol=0, atol=1e-4 * float(ref.max()))      # (the file's ligand went through float32 coordinates)
    # rescore of the same poses: the same correlations, the same pick
    np.savez(tmp_path / "poses.npz", rot_update=tj["rot_update"], tr_update=tj["tr_update"])
    p3 = _run(["rescore"] + common + ["--poses", "poses.npz", "--out", "resc.pdb", "--density", f["path"], "--density-resolution", "8", "--rank", "density"], cwd=str(tmp_path))
    assert p3.returncode == 0, p3.stdout + p3.stderr
    resc = json.loads(p3.stdout.strip().splitlines()[-1])
    assert resc["index"] == k and {x: resc["density"][x] for x in obj(k)} == obj(k) and resc["num_decoys"] == 8 and os.path.exists(tmp_path / "resc.pdb")
