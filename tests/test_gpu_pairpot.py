"""Tabulated pair potential and pair counts on the GPU (dfm_pairpot_create, dfm_pose_pairpot, kernels_pairpot.hip) against the float64
definition dfmdock_amd/pairpot.py, and through the drivers and the command line.

Every result is an integer: a count, or a sum of table entries rounded to quanta of 2^-20 kcal/mol on the host.  The bin of a pair is
found from r2 alone - fp64 + and * in a fixed order on both sides, nothing contracted, compared with the exact squares of the float32
edges - so the device's integers must EQUAL the definition's: energy_q, n_pairs, lig_q and counts, with no tolerance anywhere."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, db5_complex, db5_ids

pytestmark = pytest.mark.gpu

KEYS = ("energy_q", "n_pairs")
ALL_KEYS = KEYS + ("lig_q", "counts")
AA = "ACDEFGHIKLMNPQRSTVWY"


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


def residue_types(seq):
    """One of 20 types per residue by its letter (an unknown letter: its code modulo 20), repeated over N, CA, C, O, CB."""
    t = np.array([AA.index(c) if c in AA else ord(c) % 20 for c in seq], np.int32)
    return np.repeat(t, 5)


def ca_center(bb):
    return np.asarray(bb, np.float64)[:, 1].mean(0).astype(np.float32)


def db5_poses(rng, P=8):
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


def seeded_table(T, NB, rng, scale=3.0):
    """An asymmetric table with both signs."""
    t = rng.uniform(-scale, scale, (T, T, NB)).astype(np.float32)
    assert (t > 0).any() and (t < 0).any() and (T == 1 or not np.array_equal(t, t.transpose(1, 0, 2)))
    return t


def check_against_definition(model, rec, rt, lig, lt, center, rot, tr, edges, table, label="", chunk_poses=0):
    """One handle, one call with every output: integer equality with the definition on all four arrays, and the call's own identities:
    totals == per-atom sums, sum(counts) == n_pairs, <counts, table_q> == energy_q.  Returns (pairs, result)."""
    from dfmdock_amd import pairpot as PP
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    with model.pairpot(rec, rt, lig, lt, center, edges, table) as h:
        got = h.energy(rot, tr, per_atom=True, counts=True, chunk_poses=chunk_poses)
        info = h.info()
    want = PP.pair_potential(rec, rt, lig, lt, center, rot, tr, edges, table, per_atom=True, counts=True)
    P, Al = rot.shape[0], np.asarray(lig).reshape(-1, 3).shape[0]
    T, NB = np.asarray(table).shape[0], np.asarray(table).shape[2]
    assert got["lig_q"].shape == (P, Al) and got["counts"].shape == (P, T, T, NB) and got["counts"].dtype == np.int32
    assert all(got[k].dtype == np.int64 for k in KEYS + ("lig_q",)) and info["T"] == T and info["NB"] == NB
    tq = PP.quantise(table)
    assert np.array_equal(got["energy_q"], got["lig_q"].sum(1)), label
    assert np.array_equal(got["counts"].reshape(P, -1).sum(1, dtype=np.int64), got["n_pairs"]), label
    assert np.array_equal((got["counts"].astype(np.int64) * tq[None]).reshape(P, -1).sum(1), got["energy_q"]), label
    for k in ALL_KEYS:
        off = got[k] != want[k]
        assert not off.any(), (label, k, int(off.sum()), got[k][off][:5].tolist(), want[k][off][:5].tolist())
    assert np.array_equal(got["energy"], got["energy_q"] / 2.0 ** 20) and want["n_pairs"].max() <= info["pair_bound"]
    print(f"{label}: P {P} Ar {np.asarray(rec).reshape(-1, 3).shape[0]} Al {Al} T {T} NB {NB} pairs {int(want['n_pairs'].sum())} "
          f"energy {want['energy_q'].sum() / 2.0 ** 20:.3f} kcal/mol")
    return int(want["n_pairs"].sum()), got


def test_parity_with_the_definition_on_db5(model):
    """N, CA, C, O, CB of four DB5 backbones, 8 seeded poses each from one default_rng(0) stream, 20 residue types, 30 bins to 15 A, a
    seeded asymmetric table with both signs.  Integer equality of everything."""
    rng, trng = np.random.default_rng(0), np.random.default_rng(1)
    edges = np.linspace(0.0, 15.0, 31).astype(np.float32)
    table = seeded_table(20, 30, trng)
    pairs = 0
    for cid in db5_ids()[:4]:
        c = db5_complex(cid)
        rot, tr = db5_poses(rng)
        rec, lig = five_atoms(c["rec_pos"]), five_atoms(c["lig_pos"])
        rt, lt = residue_types(c["rec_seq"]), residue_types(c["lig_seq"])
        n, got = check_against_definition(model, rec, rt, lig, lt, ca_center(c["lig_pos"]), rot, tr, edges, table, label=cid)
        assert n > 0 and len(set(rt.tolist())) > 10
        pairs += n
    print("pairs within 15 A:", pairs)
    assert pairs > 10000


def lumps(rng, Ar, Al, T, rec_scale=8.0, lig_scale=5.0, lig_shift=1.5):
    rec = (rec_scale * rng.random((Ar, 3))).astype(np.float32)
    lig = (lig_scale * rng.random((Al, 3)) + lig_shift).astype(np.float32)
    return rec, rng.integers(0, T, Ar).astype(np.int32), lig, rng.integers(0, T, Al).astype(np.int32)


def test_small_shapes(model):
    """The smallest sizes and placements at which each path of the kernel can break, each against the definition."""
    rng = np.random.default_rng(5)
    zero = np.zeros(3, np.float32)
    poses = lambda P, s_rot=0.5, s_tr=1.5: ((s_rot * rng.standard_normal((P, 3))).astype(np.float32), (s_tr * rng.standard_normal((P, 3))).astype(np.float32))
    chk = lambda *a, **k: check_against_definition(model, *a, **k)
    e8 = np.linspace(0.0, 8.0, 9).astype(np.float32)
    # Al around the block size; Ar = 130 in ONE cell (three staged batches, the last ragged); each atom its own type (T = 256), so that a
    # wrong lig_index, a wrong receptor order or [ta][tb] for [tb][ta] shows
    one_cell = (1.5 * rng.random((130, 3))).astype(np.float32) + np.float32(1.0)
    rt = np.arange(130, dtype=np.int32)
    t256 = seeded_table(256, 4, rng)
    e4 = np.float32([0.0, 2.0, 3.5, 5.0, 7.0])
    for Al in (1, 64, 65):
        lig = (3.0 * rng.standard_normal((Al, 3))).astype(np.float32)
        lt = (130 + np.arange(Al)).astype(np.int32)
        rot, tr = poses(3)
        n, got = chk(one_cell, rt, lig, lt, lig.mean(0), rot, tr, e4, t256, label=f"Ar 130 in one cell, Al {Al}, T 256")
        assert (n > 0 or Al == 1) and got["counts"].max() <= 1      # every (ligand type, receptor type) is one atom pair
    # a cell with more than 64 atoms next to others; 200 atoms at one point
    rec, rt, lig, lt = lumps(rng, 300, 90, 7, rec_scale=10.0)
    rot, tr = poses(4)
    t7 = seeded_table(7, 8, rng)
    with model.pairpot(rec, rt, lig, lt, lig.mean(0), e8, t7) as h:
        assert h.info()["max_cell_atoms"] > 64 and h.info()["n_cells"] == 8 and h.info()["cell_edge"] == 8.0
    assert chk(rec, rt, lig, lt, lig.mean(0), rot, tr, e8, t7, label="a cell above 64 atoms")[0] > 1000
    point = np.tile(np.array([[1.0, 2.0, -0.5]], np.float32), (200, 1))
    n, _ = chk(point, rng.integers(0, 7, 200).astype(np.int32), lig, lt, lig.mean(0), rot, tr, e8, t7, label="200 atoms at one point")
    assert n >= 200 and n % 200 == 0
    # T = 1; NB = 1; NB = 64; edges[0] > 0; entries at +-1024
    rec, rt, lig, lt = lumps(rng, 150, 70, 1)
    assert chk(rec, rt, lig, lt, lig.mean(0), rot, tr, e8, seeded_table(1, 8, rng), label="T = 1")[0] > 0
    rec, rt, lig, lt = lumps(rng, 150, 70, 3)
    n1, g1 = chk(rec, rt, lig, lt, lig.mean(0), rot, tr, np.float32([0.0, 6.0]), seeded_table(3, 1, rng), label="NB = 1")
    e64 = np.sort(rng.uniform(0.0, 16.0, 65)).astype(np.float32)
    n, got = chk(rec, rt, lig, lt, lig.mean(0), rot, tr, e64, seeded_table(3, 64, rng), label="NB = 64")
    assert n > 0 and (got["counts"].sum((0, 1, 2)) > 0).sum() > 32      # most of the 64 bins are hit
    n, got = chk(rec, rt, lig, lt, lig.mean(0), rot, tr, np.float32([3.0, 4.0, 6.0]), seeded_table(3, 2, rng), label="edges[0] > 0")
    assert 0 < n < n1
    lim = np.where(rng.random((3, 3, 8)) < 0.5, np.float32(1024.0), np.float32(-1024.0)).astype(np.float32)
    n, got = chk(rec, rt, lig, lt, lig.mean(0), rot, tr, e8, lim, label="entries at +-1024")
    assert n > 0 and (np.abs(got["lig_q"]).max() >= 1 << 30) and (got["energy_q"] % (1 << 30) == 0).all()
    # pairs placed exactly on edges under the identity pose: r = 2 is bin 0, r = 3 bin 1, r = 4.5 bin 2, r = 6 = the last edge is out,
    # r = 1.5 is below the first edge; squares of these are exact
    edges = np.float32([2.0, 3.0, 4.5, 6.0])
    rec1 = np.zeros((1, 3), np.float32)
    lig = np.float32([[2, 0, 0], [0, 3, 0], [0, 0, -4.5], [6, 0, 0], [0, 1.5, 0], [0, 0, np.nextafter(np.float32(6), np.float32(0))]])
    tab = np.float32([[[1.0, 2.0, 4.0]]])
    z1 = np.zeros((1, 3), np.float32)
    n, got = chk(rec1, np.zeros(1, np.int32), lig, np.zeros(6, np.int32), zero, z1, z1, edges, tab, label="pairs exactly on edges")
    assert n == 4 and got["lig_q"][0].tolist() == [1 << 20, 2 << 20, 4 << 20, 0, 0, 4 << 20] and got["counts"][0, 0, 0].tolist() == [1, 1, 2]
    # a ligand far away: every wave leaves early and the outputs are zero
    rec, rt, lig, lt = lumps(rng, 300, 70, 7)
    far = np.array([[40.0, 0, 0], [0, -35.0, 0], [0, 0, 30.0], [-20.0, -20.0, -20.0]], np.float32)
    n, got = chk(rec, rt, lig, lt, lig.mean(0), np.zeros((4, 3), np.float32), far, e8, t7, label="a ligand far away")
    assert n == 0 and not any(got[k].any() for k in ALL_KEYS)
    # outside on the low side by less than the cutoff: negative cell coordinates before the clamp; P = 1
    low = np.array([[-7.5, 3.0, 3.0], [3.0, -8.5, 3.0], [3.0, 3.0, -9.0], [-5.0, -5.0, -5.0]], np.float32)
    assert chk(rec, rt, lig, lt, lig.mean(0), np.zeros((4, 3), np.float32), low, e8, t7, label="outside on the low side")[0] > 0
    assert chk(rec, rt, lig, lt, lig.mean(0), rot[:1], tr[:1], e8, t7, label="P = 1")[0] > 0


def _ensemble(seed=1, P=5, Ar=400, Al=150, T=6, NB=10):
    rng = np.random.default_rng(seed)
    rec, rt, lig, lt = lumps(rng, Ar, Al, T, rec_scale=14.0, lig_scale=7.0, lig_shift=3.0)
    rot, tr = (0.3 * rng.standard_normal((P, 3))).astype(np.float32), (2.0 * rng.standard_normal((P, 3))).astype(np.float32)
    edges = np.sort(rng.uniform(0.5, 9.0, NB + 1)).astype(np.float32)
    return rec, rt, lig, lt, lig.mean(0), rot, tr, edges, seeded_table(T, NB, rng)


def _same(a, b, keys, label=""):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (label, k)


def test_invariances_are_exact(model):
    from dfmdock_amd import _lib as L
    from dfmdock_amd import engine
    rec, rt, lig, lt, cen, rot, tr, edges, table = _ensemble()
    P = rot.shape[0]
    with model.pairpot(rec, rt, lig, lt, cen, edges, table) as h:
        full = h.energy(rot, tr, per_atom=True, counts=True)
        assert (full["n_pairs"] > 0).all() and (full["energy_q"] != 0).all()
        cp, kn = engine.pairpot_last_timing()
        ph = engine.pairpot_last_phases()
        assert cp > 0 and kn > 0 and ph[0] > 0 and ph[1] > 0 and ph[2] >= 0 and abs(sum(ph) - kn) <= 1e-3 * kn + 1e-3
        # chunks of 0, 1 and 2 poses on 5
        for c in (0, 1, 2):
            _same(full, h.energy(rot, tr, per_atom=True, counts=True, chunk_poses=c), ALL_KEYS, f"chunk {c}")
            _same(full, h.energy(rot, tr, chunk_poses=c), KEYS, f"chunk {c}, totals alone")
        # counts=False gives the same energies as counts=True; each optional output alone
        _same(full, h.energy(rot, tr), KEYS, "energy only")
        _same(full, h.energy(rot, tr, per_atom=True), KEYS + ("lig_q",), "per atom")
        _same(full, h.energy(rot, tr, counts=True), KEYS + ("counts",), "counts")
        # permuting the poses; P = 1 against the same pose inside P
        perm = np.random.default_rng(2).permutation(P)
        _same({k: full[k][perm] for k in ALL_KEYS}, h.energy(rot[perm], tr[perm], per_atom=True, counts=True), ALL_KEYS, "poses permuted")
        for p in (0, P - 1):
            _same({k: full[k][p:p + 1] for k in ALL_KEYS}, h.energy(rot[p:p + 1], tr[p:p + 1], per_atom=True, counts=True), ALL_KEYS, f"P = 1, pose {p}")
        # any subset of the output pointers NULL
        f = lambda x: x.ctypes.data_as(L.F32P)
        for mask in range(16):
            out, bufs = L.PairpotOutC(), {}
            for b, k in enumerate(ALL_KEYS):
                if mask >> b & 1:
                    bufs[k] = np.full_like(full[k], 7)
                    setattr(out, k, bufs[k].ctypes.data_as(C.POINTER(C.c_int32 if k == "counts" else C.c_int64)))
            assert L.lib().dfm_pose_pairpot(h._h, P, f(rot), f(tr), C.byref(out)) == 0, mask
            _same(full, bufs, tuple(bufs), f"pointer mask {mask}")
        # two host threads on the same handle at once
        res, errs = [None, None], []

        def work(i):
            try:
                res[i] = [h.energy(rot, tr, per_atom=True, counts=True, chunk_poses=(0, 2)[i]) for _ in range(3)]
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
                _same(full, r, ALL_KEYS, "threads")
    # permuting either chain's atoms with their types
    prng = np.random.default_rng(3)
    pr, pl = prng.permutation(rec.shape[0]), prng.permutation(lig.shape[0])
    with model.pairpot(rec[pr], rt[pr], lig, lt, cen, edges, table) as h:
        _same(full, h.energy(rot, tr, per_atom=True, counts=True), ALL_KEYS, "receptor atoms permuted")
    with model.pairpot(rec, rt, lig[pl], lt[pl], cen, edges, table) as h:
        got = h.energy(rot, tr, per_atom=True, counts=True)
        _same(full, got, KEYS + ("counts",), "ligand atoms permuted")
        assert np.array_equal(got["lig_q"], full["lig_q"][:, pl])
    # relabelling the types with the table permuted to match: new type s[t] for old type t
    T = table.shape[0]
    s = prng.permutation(T).astype(np.int32)
    inv = np.argsort(s)
    tab2 = np.ascontiguousarray(table[inv][:, inv])      # tab2[s[a], s[b]] = table[a, b]
    with model.pairpot(rec, s[rt], lig, s[lt], cen, edges, tab2) as h:
        got = h.energy(rot, tr, per_atom=True, counts=True)
        _same(full, got, KEYS + ("lig_q",), "types relabelled")
        assert np.array_equal(got["counts"][:, s][:, :, s], full["counts"])


def test_nan_poses(model):
    from dfmdock_amd import pairpot as PP
    rec, rt, lig, lt, cen, rot, tr, edges, table = _ensemble(seed=3, P=8)
    with model.pairpot(rec, rt, lig, lt, cen, edges, table) as h:
        clean = h.energy(rot, tr, per_atom=True, counts=True)
        assert (clean["n_pairs"] > 0).sum() >= 6
        r2, t2 = rot.copy(), tr.copy()
        r2[2, 1] = np.nan
        t2[5, 0] = np.inf
        r2[6, 2] = -np.inf
        dirty = h.energy(r2, t2, per_atom=True, counts=True, chunk_poses=3)
    for p in (2, 5, 6):
        assert not any(dirty[k][p].any() for k in ALL_KEYS)
    keep = np.ones(8, bool)
    keep[[2, 5, 6]] = False
    _same({k: clean[k][keep] for k in ALL_KEYS}, {k: dirty[k][keep] for k in ALL_KEYS}, ALL_KEYS)
    want = PP.pair_potential(rec, rt, lig, lt, cen, r2, t2, edges, table)
    assert not want["n_pairs"][[2, 5, 6]].any() and np.array_equal(want["n_pairs"], dirty["n_pairs"])


def test_invalid_arguments(model):
    """DFM_E_INVALID / NULL, dfm_last_error set, nothing enqueued, in the order the header gives; the handle still works afterwards."""
    from dfmdock_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(4)
    rec, rt, lig, lt = lumps(rng, 40, 30, 3, rec_scale=6.0)
    edges, table = np.float32([0.0, 2.0, 4.0, 6.0, 8.0]), seeded_table(3, 4, rng)
    cen = lig.mean(0)
    f = lambda x: None if x is None else x.ctypes.data_as(L.F32P)
    i = lambda x: None if x is None else x.ctypes.data_as(L.I32P)
    keep = []      # the arrays behind the pointers of one call

    def create(m=model._h, Ar=40, rec=rec, rt=rt, Al=30, lig=lig, lt=lt, cen=cen, T=3, NB=4, edges=edges, table=table, chunk=0):
        a = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (rec, lig, cen, edges, table)]
        b = [None if v is None else np.ascontiguousarray(v, np.int32) for v in (rt, lt)]
        keep.append((a, b))
        return lib.dfm_pairpot_create(m, Ar, f(a[0]), i(b[0]), Al, f(a[1]), i(b[1]), f(a[2]), T, NB, f(a[3]), f(a[4]), chunk)

    def mod(a, k, v):
        b = np.array(a, copy=True)
        b[k] = v
        return b
    wide = mod(rec, 0, 4000.0)      # 500^3 cells of 8 A > 2^24
    cases = [(dict(m=None), "m is NULL"), (dict(rec=None), "rec_atoms is NULL"), (dict(lig=None), "lig_atoms is NULL"), (dict(cen=None), "center is NULL"),
             (dict(Ar=0), "Ar >= 1"), (dict(Al=0), "Al >= 1"), (dict(Ar=(1 << 24) + 1), "exceeds 2^24 atoms"),
             (dict(rec=mod(rec, (7, 1), np.nan)), "rec_atoms: atom 7 is not finite"), (dict(lig=mod(lig, (3, 2), np.inf)), "lig_atoms: atom 3 is not finite"),
             (dict(cen=mod(cen, 0, np.inf)), "center is not finite"),
             (dict(rt=None), "rec_type is NULL"), (dict(lt=None), "lig_type is NULL"),
             (dict(T=0), "need 1 <= T <= 256"), (dict(T=257), "need 1 <= T <= 256"),
             (dict(NB=0), "need 1 <= NB <= 64"), (dict(NB=65), "need 1 <= NB <= 64"), (dict(edges=None), "edges is NULL"),
             (dict(edges=mod(edges, 2, np.nan)), "edges: edge 2 is not finite"), (dict(edges=mod(edges, 4, np.inf)), "edges: edge 4 is not finite"),
             (dict(edges=mod(edges, 2, 2.0)), "edges: edge 2 is not above edge 1"), (dict(edges=mod(edges, 3, 1.0)), "edges: edge 3 is not above edge 2"),
             (dict(edges=mod(edges, 0, -1.0)), "edges: edge 0 is below 0"), (dict(edges=mod(edges, 4, 16.5)), "edges: the last edge is above 16"),
             (dict(table=None), "table is NULL"), (dict(table=mod(table, (1, 2, 3), np.nan)), "table: entry 23 is not in [-1024, 1024]"),
             (dict(table=mod(table, (0, 0, 1), 1024.5)), "table: entry 1 is not in [-1024, 1024]"), (dict(table=mod(table, (2, 2, 3), -np.inf)), "table: entry 35 is not in [-1024, 1024]"),
             (dict(rt=mod(rt, 5, 3), lt=mod(lt, 2, -1)), "rec_type: atom 5 has type 3 outside [0, 3)"), (dict(lt=mod(lt, 2, -1)), "lig_type: atom 2 has type -1 outside [0, 3)"),
             (dict(chunk=-1), "chunk_poses must be >= 0"), (dict(rec=wide), "more than 2^24 cells of the last edge")]
    for kw, word in cases:
        assert create(**kw) is None, word
        msg = lib.dfm_last_error().decode()
        print(word, "->", msg)
        assert word in msg, (word, msg)
    # the order: the atoms before the types before T before the edges before the table before a type out of range
    assert create(rec=mod(rec, (7, 1), np.nan), rt=None, T=0, edges=None, table=None) is None and "rec_atoms: atom 7" in lib.dfm_last_error().decode()
    assert create(lt=None, T=0, edges=None) is None and "lig_type is NULL" in lib.dfm_last_error().decode()
    assert create(T=300, edges=None, table=None) is None and "need 1 <= T" in lib.dfm_last_error().decode()
    assert create(edges=mod(edges, 0, -1.0), table=None, rt=mod(rt, 5, 9)) is None and "edge 0 is below 0" in lib.dfm_last_error().decode()
    assert create(table=mod(table, (0, 0, 0), np.nan), rt=mod(rt, 5, 9), chunk=-1) is None and "table: entry 0" in lib.dfm_last_error().decode()
    assert create(rt=mod(rt, 5, 9), chunk=-1) is None and "rec_type: atom 5" in lib.dfm_last_error().decode()
    # the pair bound: 32768 receptor atoms at one point (one cell) against 65536 ligand atoms are 2^31 pairs, one above the limit; with
    # one receptor atom fewer the creator accepts.  Around it: a receptor box without a grid is refused first, the bound next, the
    # ligand's extent about the centre last
    big_r, big_l = np.tile(np.float32([[1.0, 2.0, 3.0]]), (32768, 1)), np.zeros((65536, 3), np.float32)
    zr, zl = np.zeros(32768, np.int32), np.zeros(65536, np.int32)
    far_l, far_c = mod(big_l, (0, 0), 3e38), np.float32([-3e38, 0.0, 0.0])      # every input finite, the block's centre about the rotation centre is not
    big = dict(Ar=32768, rec=big_r, rt=zr, Al=65536, lig=big_l, lt=zl)
    assert create(**big) is None and "atom pairs in range, more than 2^31 - 1" in lib.dfm_last_error().decode()
    assert create(**dict(big, rec=mod(big_r, 0, 4000.0))) is None and "more than 2^24 cells of the last edge" in lib.dfm_last_error().decode()
    assert create(**dict(big, lig=far_l, cen=far_c)) is None and "more than 2^31 - 1" in lib.dfm_last_error().decode()
    assert create(lig=mod(lig, (0, 0), 3e38), cen=far_c) is None
    assert "lig_atoms / center: the ligand's extent about the centre overflows fp32" in lib.dfm_last_error().decode()
    a = create(**dict(big, Ar=32767, rec=big_r[:32767], rt=zr[:32767]))
    assert a
    pb = C.c_double(0)
    assert lib.dfm_pairpot_info(a, None, None, None, C.byref(pb), None, None) == 0 and pb.value == 32767.0 * 65536.0 <= 2.0 ** 31 - 1
    lib.dfm_pairpot_destroy(a)
    keep.clear()
    a = create(edges=mod(edges, 4, 16.0), table=mod(mod(table, (0, 0, 0), 1024.0), (2, 2, 3), -1024.0))      # the limits themselves are fine
    assert a
    lib.dfm_pairpot_destroy(a)
    a = create()
    assert a
    rot, tr = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    out = L.PairpotOutC()
    n_pairs = np.zeros(4, np.int64)
    out.n_pairs = n_pairs.ctypes.data_as(C.POINTER(C.c_int64))
    o = C.byref(out)
    for args, word in [((None, 4, f(rot), f(tr), o), "h is NULL"), ((a, 4, None, f(tr), o), "rot is NULL"), ((a, 4, f(rot), None, o), "tr is NULL"),
                       ((a, 4, f(rot), f(tr), None), "out is NULL"), ((a, 0, f(rot), f(tr), o), "P >= 1")]:
        assert lib.dfm_pose_pairpot(*args) == -1, word
        assert word in lib.dfm_last_error().decode(), word
    assert lib.dfm_pose_pairpot_chunked(a, 4, f(rot), f(tr), -1, o) == -1 and "chunk_poses" in lib.dfm_last_error().decode()
    assert lib.dfm_pairpot_last_timing(None, None) == -1 and lib.dfm_pairpot_last_phases(None, None, None) == -1
    assert lib.dfm_pairpot_info(None, None, None, None, None, None, None) == -1
    assert lib.dfm_pose_pairpot(a, 4, f(rot), f(tr), o) == 0 and (n_pairs == n_pairs[0]).all() and n_pairs[0] > 0      # the handle still works
    lib.dfm_pairpot_destroy(a)
    lib.dfm_pairpot_destroy(None)
    for bad in (dict(edges=[0, 17]), dict(table=table[:, :2]), dict(rt=mod(rt, 0, 3)), dict(lt=lt[:-1]), dict(cen=cen[:2])):
        kw = dict(dict(rec=rec, rt=rt, lig=lig, lt=lt, cen=cen, edges=edges, table=table), **bad)
        with pytest.raises(ValueError):
            model.pairpot(kw["rec"], kw["rt"], kw["lig"], kw["lt"], kw["cen"], kw["edges"], kw["table"])


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
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pairpot_alloc_child.py"), out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=60)
        assert p.returncode == 0, f"{tag}: exit {p.returncode}\n" + p.stdout.decode(errors="replace")[-2000:]
        runs[tag] = dict(np.load(out, allow_pickle=False))
    ref = runs["default"]
    assert len([k for k in ref if not k.startswith("__")]) == 8 and ref["full/n_pairs"].min() > 0 and ref["full/counts"].sum() == ref["full/n_pairs"].sum()
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
    """On 7CEI with the seeded checkpoint and a seeded table file.  Without the new flags `dock` writes what dock_pair without options
    writes and its line has no new key; under --rank pairpot the kept pose is the argmin of the energy recomputed by the definition over
    every trajectory; --pairpot-residues and --pair-counts hold the definition's numbers for that pose and for every model."""
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    from test_pairpot_cpu import seeded_potential
    from dfmdock_amd import cli, driver
    from dfmdock_amd import pairpot as PP
    from dfmdock_amd import sterics as ST
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    pot_path = str(tmp_path / "pot.npz")
    pot = seeded_potential(pot_path)
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
    assert "pair_potential" not in d0 and "index" not in d0 and "trajectories" not in d0
    # --rank pairpot against the definition over every trajectory
    p2 = _run(["dock"] + base + ["--out", "rank.pdb", "--pair-potential", pot_path, "--rank", "pairpot", "--top-k", "3", "--pairpot-residues", "res.txt",
                                 "--pair-counts", "cnt.npz"], cwd=str(tmp_path))
    assert p2.returncode == 0, p2.stdout + p2.stderr
    ranked = json.loads(p2.stdout.strip().splitlines()[-1])
    d2 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "api_rank.pdb"), rank="pairpot", pair_potential=pot, top_k=3, **kw)
    tj = d2["trajectories"]
    ra, rt, la, lt, cen, lk, nu = driver.pairpot_inputs(rec, lig, 0, pot)
    want = PP.pair_potential(ra, rt, la, lt, cen, tj["rot_update"], tj["tr_update"], pot["edges"], pot["table"], per_atom=True, counts=True)
    for k in KEYS:
        assert np.array_equal(want[k], d2["pairpot_data"][k]), k
    energy = PP.kcal(want["energy_q"])
    k = int(np.argmin(energy))
    print("energies", energy.tolist(), "kept", k, "energy pick", int(np.argmin(tj["energy"])))
    assert d2["index"] == k == ranked["index"] and pdb("rank.pdb") == pdb("api_rank.pdb") and (want["n_pairs"] > 0).any()
    obj = lambda p: {"energy": float(energy[p]), "n_pairs": int(want["n_pairs"][p]), "n_untyped": int(nu), "T": 21, "NB": 30, "cutoff": 15.0}
    assert ranked["pair_potential"] == obj(k) == d2["pair_potential"]
    assert np.array_equal(np.float32(ranked["rot_update"]), tj["rot_update"][k])
    models = ranked["models"]
    assert len(models) >= 1 and models[0]["index"] == k and all(m["pair_potential"] == obj(m["index"]) for m in models)
    assert [m["pair_potential"]["energy"] for m in models] == sorted(m["pair_potential"]["energy"] for m in models)
    # --pairpot-residues: the definition's per-atom sums of the kept pose, per ligand residue
    heavy = ST.heavy_atoms(lig["atoms"])
    keys, res = ST.residue_of_atoms(lig["atoms"], heavy)
    of_atom = dict(zip(heavy.tolist(), res.tolist()))
    PP.write_pairpot_residues(str(tmp_path / "want.txt"), keys, PP.residue_energy(want["lig_q"][k], np.array([of_atom[int(i)] for i in lk]), len(keys)))
    assert pdb("res.txt") == pdb("want.txt") and len(pdb("res.txt").splitlines()) > 1
    # --pair-counts: the definition's counts of the kept pose and of every model
    with np.load(tmp_path / "cnt.npz", allow_pickle=False) as z:
        idx = [k] + [m["index"] for m in models]
        assert z["index"].tolist() == idx and np.array_equal(z["counts"], want["counts"][idx]) and z["counts"].dtype == np.int32
        assert z["type_names"].tolist() == pot["type_names"] and np.array_equal(z["edges"], pot["edges"]) and z["counts"][0].sum() == want["n_pairs"][k]
