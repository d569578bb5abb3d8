"""The float64 definition of the tabulated pair potential (dfmdock_amd/pairpot.py), its typing rule and file format, the checks,
quantisation, transposition and pair bound of dfm_poseprep.h (tests/pairpot_prep_main.cpp under the address and undefined-behaviour
sanitizers) and the plumbing, on the CPU.  The GPU call is held against this definition in tests/test_gpu_pairpot.py."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_pair
from conftest import ROOT

Z3 = np.zeros((1, 3), np.float32)
Q = 2.0 ** 20


def pp(rec, rt, lig, lt, edges, table, center=(0, 0, 0), rot=Z3, tr=Z3, **kw):
    from dfmdock_amd import pairpot as PP
    f = lambda a: np.asarray(a, np.float32).reshape(-1, 3)
    return PP.pair_potential(f(rec), np.asarray(rt, np.int32), f(lig), np.asarray(lt, np.int32), np.asarray(center, np.float32), rot, tr,
                             np.asarray(edges, np.float32), np.asarray(table, np.float32), per_atom=True, counts=True, **kw)


def test_hand_placed_pairs_on_an_axis():
    """Distances whose squares are exact: a pair at 3.0 with an edge at 3.0 lands in the bin that STARTS there, a pair at exactly the
    last edge is out, a pair below edges[0] > 0 is out."""
    edges = [2.0, 3.0, 4.5, 6.0]
    table = np.float32([[[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]], [[-1.0, -2.0, -4.0], [-8.0, -16.0, -32.0]]])      # [ta][tb][bin]
    rec, rt = [[0, 0, 0]], [1]
    lig = [[3.0, 0, 0], [0, 6.0, 0], [0, 0, 1.5], [0, 2.0, 0], [0, 0, -4.5], [np.nextafter(np.float32(6.0), np.float32(0)), 0, 0], [1.0, 1.0, 1.0]]
    lt = [0, 0, 0, 1, 1, 0, 0]
    o = pp(rec, rt, lig, lt, edges, table)
    # atom 0: r = 3 -> bin 1 (16); atom 1: r = 6 = the last edge -> out; atom 2: r = 1.5 < edges[0] -> out; atom 3: r = 2 = edges[0] ->
    # bin 0 of (1, 1) (-8); atom 4: r = 4.5 -> bin 2 of (1, 1) (-32); atom 5: just below 6 -> bin 2 of (0, 1) (32); atom 6: r2 = 3 < 4 -> out
    assert o["lig_q"][0].tolist() == [int(16 * Q), 0, 0, int(-8 * Q), int(-32 * Q), int(32 * Q), 0]
    assert o["n_pairs"].tolist() == [4] and o["energy_q"].tolist() == [int(8 * Q)] and o["energy_q"].dtype == np.int64
    want = np.zeros((2, 2, 3), np.int32)
    want[0, 1, 1] = want[1, 1, 0] = want[1, 1, 2] = want[0, 1, 2] = 1
    assert np.array_equal(o["counts"][0], want) and o["counts"].dtype == np.int32
    # an entry of 0 still counts as a pair
    o = pp(rec, [0], [[3.0, 0, 0]], [0], edges, np.zeros((1, 1, 3), np.float32))
    assert o["n_pairs"].tolist() == [1] and o["energy_q"].tolist() == [0] and o["counts"][0, 0, 0].tolist() == [0, 1, 0]
    # the table is indexed (ligand type, receptor type): an asymmetric table tells the two apart
    asym = np.zeros((2, 2, 3), np.float32)
    asym[0, 1, 1] = 5.0
    assert pp(rec, [1], [[3.0, 0, 0]], [0], edges, asym)["energy_q"].tolist() == [int(5 * Q)]
    assert pp(rec, [0], [[3.0, 0, 0]], [1], edges, asym)["energy_q"].tolist() == [0]
    # a non-finite pose gets zeros; the others are not disturbed
    o = pp(rec, [1], [[3.0, 0, 0]], [0], edges, asym, rot=np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0]]), tr=np.float32([[0, 0, 0], [0, 0, 0], [np.inf, 0, 0]]))
    assert o["n_pairs"].tolist() == [1, 0, 0] and o["energy_q"].tolist() == [int(5 * Q), 0, 0] and not o["counts"][1:].any() and not o["lig_q"][1:].any()


def toy(seed=0, Ar=9, Al=6, T=3, NB=5, lo=0.5, hi=7.0):
    rng = np.random.default_rng(seed)
    rec, lig = (5.0 * rng.random((Ar, 3))).astype(np.float32), (5.0 * rng.random((Al, 3)) + 2.0).astype(np.float32)
    rt, lt = rng.integers(0, T, Ar).astype(np.int32), rng.integers(0, T, Al).astype(np.int32)
    edges = np.sort(rng.uniform(lo, hi, NB + 1)).astype(np.float32)
    table = rng.uniform(-3.0, 3.0, (T, T, NB)).astype(np.float32)
    rot, tr = (0.4 * rng.standard_normal((3, 3))).astype(np.float32), rng.standard_normal((3, 3)).astype(np.float32)
    return rec, rt, lig, lt, lig.mean(0), rot, tr, edges, table


def test_triple_loop_in_python_floats_equals_the_vectorised_definition():
    from dfmdock_amd import pairpot as PP
    from dfmdock_amd import sterics as ST
    rec, rt, lig, lt, cen, rot, tr, edges, table = toy()
    got = PP.pair_potential(rec, rt, lig, lt, cen, rot, tr, edges, table, per_atom=True, counts=True)
    e2 = [float(e) * float(e) for e in edges]
    pairs = 0
    for p in range(3):
        X = ST.pose_atoms(lig, cen, rot[p], tr[p])
        tot, per, cnt = 0, [0] * 6, np.zeros((3, 3, 5), int)
        for a in range(6):
            for b in range(9):
                dx, dy, dz = (float(X[a, k]) - float(rec[b, k]) for k in range(3))
                r2 = (dx * dx + dy * dy) + dz * dz
                if not (e2[0] <= r2 < e2[5]):
                    continue
                k = sum(1 for v in e2 if v <= r2) - 1
                q = round(float(table[lt[a], rt[b], k]) * Q)
                tot += q
                per[a] += q
                cnt[lt[a], rt[b], k] += 1
                pairs += 1
        assert int(got["energy_q"][p]) == tot and got["lig_q"][p].tolist() == per and np.array_equal(got["counts"][p], cnt)
    assert int(got["n_pairs"].sum()) == pairs and 30 < pairs < 3 * 54


def test_identities_and_the_bounding_box_shortcut():
    from dfmdock_amd import pairpot as PP
    rec, rt, lig, lt, cen, rot, tr, edges, table = toy(3, 300, 90, T=7, NB=12, lo=1.0, hi=9.0)
    rec = (rec * np.float32(6.0)).astype(np.float32)      # a 30 A box: most receptor atoms are out of reach of the ligand
    tr = np.concatenate([tr, np.float32([[70, 0, 0]])])   # and one pose out of reach altogether
    rot = np.concatenate([rot, np.zeros((1, 3), np.float32)])
    a = PP.pair_potential(rec, rt, lig, lt, cen, rot, tr, edges, table, per_atom=True, counts=True)
    b = PP.pair_potential(rec, rt, lig, lt, cen, rot, tr, edges, table, per_atom=True, counts=True, shortcut=False)
    assert a["n_pairs"][:3].min() > 0 and a["n_pairs"][3] == 0 and all(a[k].tobytes() == b[k].tobytes() for k in a)
    tq = PP.quantise(table)
    assert np.array_equal(a["counts"].reshape(4, -1).sum(1), a["n_pairs"])
    assert np.array_equal((a["counts"].astype(np.int64) * tq[None]).reshape(4, -1).sum(1), a["energy_q"])
    assert np.array_equal(a["lig_q"].sum(1), a["energy_q"])
    plain = PP.pair_potential(rec, rt, lig, lt, cen, rot, tr, edges, table)
    assert set(plain) == {"energy_q", "n_pairs"} and np.array_equal(plain["energy_q"], a["energy_q"])


def test_quantisation_and_bins():
    from dfmdock_amd import pairpot as PP
    assert PP.quantise(np.float32([0.5 / Q, 1.5 / Q, 2.5 / Q, -0.5 / Q, -1.5 / Q, 1024.0, -1024.0])).tolist() == [0, 2, 2, 0, -2, 1 << 30, -(1 << 30)]
    assert PP.kcal(np.int64([1 << 20, -(1 << 19)])).tolist() == [1.0, -0.5]
    e = np.float32([0.1, 0.3, 3.0])
    e2 = PP.edges2(e)
    assert e2.dtype == np.float64 and e2.tolist() == [float(v) * float(v) for v in e]
    assert PP.bin_of([0.0, e2[0], np.nextafter(e2[1], 0), e2[1], 8.99, 9.0, 10.0], e2).tolist() == [-1, 0, 0, 1, 1, 2, 2]


def pdb_line(k, name, res, chain, num, xyz, el, het=False):
    return "%-6s%5d %-4s %3s %s%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s\n" % (
        "HETATM" if het else "ATOM", k, name if len(name) == 4 else " " + name, res, chain, num, xyz[0], xyz[1], xyz[2], 1.0, 0.0, el)


def test_the_naming_rule_on_a_written_pdb(tmp_path):
    from dfmdock_amd import pairpot as PP
    from dfmdock_amd import pdbio
    from dfmdock_amd import sterics as ST
    rows = [("N", "LYS", "A", 1, "N"), ("CA", "LYS", "A", 1, "C"), ("NZ", "LYS", "A", 1, "N"), ("H", "LYS", "A", 1, "H"),
            ("CA", "GLY", "A", 2, "C"), ("O", "GLY", "A", 2, "O"), ("CB", "ALA", "A", 3, "C"), ("SD", "MET", "A", 4, "S"),
            ("ZN", "HIS", "A", 5, "ZN")]
    path = tmp_path / "x.pdb"
    path.write_text("".join(pdb_line(k + 1, *r[:4], (k, 0, 0), r[4]) for k, r in enumerate(rows)) + pdb_line(99, "O", "HOH", "A", 9, (0, 0, 0), "O", True))
    atoms = pdbio.read_pdb(str(path))
    heavy = ST.heavy_atoms(atoms)
    assert heavy.tolist() == [0, 1, 2, 4, 5, 6, 7, 8]
    # the priority RES:ATOM > RES:* > *:ATOM > @ELEMENT > *
    names = ["LYS:NZ", "LYS:*", "*:CA", "@O", "@C", "@S"]
    types, kept, untyped = PP.atom_types(atoms, names)
    #            LYS N   LYS CA  LYS NZ  GLY CA  GLY O  ALA CB  MET SD   HIS ZN: no name fits
    assert types.tolist() == [1, 1, 0, 2, 3, 4, 5] and kept.tolist() == [0, 1, 2, 4, 5, 6, 7] and untyped == 1
    assert types.dtype == np.int32 and kept.dtype == np.int64
    types, kept, untyped = PP.atom_types(atoms, names + ["*"])
    assert types.tolist() == [1, 1, 0, 2, 3, 4, 5, 6] and untyped == 0 and kept.tolist() == heavy.tolist()
    types, kept, untyped = PP.atom_types(atoms, ["@N", "*:CA"], heavy_index=[0, 1, 3, 4])      # (3 is the hydrogen: the caller's choice)
    assert types.tolist() == [0, 1, 1] and kept.tolist() == [0, 1, 4] and untyped == 1
    # residue types alone
    types, kept, untyped = PP.atom_types(atoms, ["GLY:*", "LYS:*", "ALA:*", "MET:*"])
    assert types.tolist() == [1, 1, 1, 0, 0, 2, 3] and untyped == 1


def test_save_load_round_trip_and_every_refusal(tmp_path):
    from dfmdock_amd import pairpot as PP
    rng = np.random.default_rng(0)
    edges, table = np.linspace(0.0, 15.0, 31), rng.uniform(-2, 2, (4, 4, 30))
    names = ["ALA:CB", "GLY:*", "@N", "*"]
    path = str(tmp_path / "pot.npz")
    PP.save(path, edges, table, names)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    d = PP.load(path)
    assert d["type_names"] == names and d["edges"].dtype == np.float32 and np.array_equal(d["edges"], np.float32(edges))
    assert d["table"].dtype == np.float32 and np.array_equal(d["table"], np.float32(table))
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["edges", "table", "type_names"]
    ok_e, ok_t = np.float32([0, 1, 2]), np.zeros((2, 2, 2), np.float32)
    assert PP.check_edges(ok_e).dtype == np.float32 and PP.check_table(ok_t, 2).shape == (2, 2, 2)
    assert PP.check_edges(np.float32([0.0, 16.0])).size == 2 and PP.check_edges(np.linspace(0, 16, 65)).size == 65
    for bad in ([1.0], np.linspace(0, 16, 66), [0, 1, np.nan], [0, np.inf], [0, 1, 1], [0, 2, 1], [-0.5, 1], [0, 16.5], [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            PP.check_edges(bad)

    def tab(T=2, NB=2, **kw):
        t = np.zeros((T, T, NB), np.float32)
        for k, v in kw.items():
            t[tuple(int(c) for c in k[1:])] = v
        return t
    assert PP.check_table(tab(_000=1024.0, _111=-1024.0)) is not None and PP.check_table(np.zeros((256, 256, 1), np.float32)) is not None
    for bad in (tab(_000=1024.5), tab(_010=np.nan), tab(_101=-np.inf), np.zeros((2, 3, 2)), np.zeros((2, 2)), np.zeros((257, 257, 1)), np.zeros((1, 1, 65)),
                np.zeros((0, 0, 2))):
        with pytest.raises(ValueError):
            PP.check_table(bad)
    with pytest.raises(ValueError):
        PP.check_table(ok_t, 3)
    assert PP.check_types([0, 1, 1], 3, 2).dtype == np.int32
    for bad, n in (([0, 2], 2), ([-1, 0], 2), ([0, 1], 3), ([0.0, 1.0], 2)):
        with pytest.raises(ValueError):
            PP.check_types(np.asarray(bad), n, 2)
    for a in ((ok_e, ok_t, ["a"]), (ok_e, ok_t, ["a", "a"]), (ok_e, np.zeros((2, 2, 3)), ["a", "b"]), ([0, 17], np.zeros((2, 2, 1)), ["a", "b"])):
        with pytest.raises(ValueError):
            PP.save(str(tmp_path / "bad.npz"), *a)
    with open(tmp_path / "missing.npz", "wb") as f:
        np.savez(f, edges=ok_e, table=ok_t)
    with pytest.raises(ValueError):
        PP.load(str(tmp_path / "missing.npz"))
    with open(tmp_path / "names.npz", "wb") as f:
        np.savez(f, edges=ok_e, table=ok_t, type_names=np.arange(2))
    with pytest.raises(ValueError):
        PP.load(str(tmp_path / "names.npz"))
    # residue sums and the residue file
    res = np.array([0, 0, 1, 2, 2, 2])
    assert PP.residue_energy(np.int64([5, -7, 3, 0, 1, 1]), res, 4).tolist() == [-2, 3, 2, 0]
    out = tmp_path / "e.txt"
    PP.write_pairpot_residues(str(out), [("B", 7, " ", "LYS"), ("B", 8, "A", "GLY"), ("B", 9, " ", "ASP")], np.int64([-(3 << 19), 0, 1]))
    assert out.read_text().splitlines()[1:] == ["B:7 LYS -1.500000", "B:9 ASP 0.000001"]


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairpot_prep")
    exe = str(d / "pairpot_prep")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "pairpot_prep_main.cpp"), "-o", exe])

    def parse(r):
        assert r.stderr == "", r.stderr      # a sanitizer report
        return r.returncode, {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}

    def run(rec, rt, lig, lt, edges, table, T=None, NB=None, center=(0, 0, 0)):
        edges = None if edges is None else np.asarray(edges, np.float32)
        table = None if table is None else np.asarray(table, np.float32)
        T = table.shape[0] if T is None else T
        NB = edges.size - 1 if NB is None else NB
        path = str(d / "in.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iiiiii", rec.shape[0], lig.shape[0], T, NB, 0 if edges is None else edges.size, 0 if table is None else table.size))
            f.write(np.float32(center).tobytes())
            for xyz, ty in ((rec, rt), (lig, lt)):
                f.write(np.ascontiguousarray(xyz, np.float32).tobytes() + np.ascontiguousarray(ty, np.int32).tobytes())
            f.write((b"" if edges is None else edges.tobytes()) + (b"" if table is None else table.tobytes()))
        return parse(subprocess.run([exe, path], capture_output=True, text=True))
    run.cmd = lambda *a: parse(subprocess.run([exe] + [str(v) for v in a], capture_output=True, text=True))
    return run


def test_refusals_of_the_host_preparation(prep):
    rec, rt, lig, lt, _, _, _, edges, table = toy(1, 40, 30)
    err = lambda *a, **k: " ".join(prep(*a, **k)[1].get("error", ["<none>"]))
    assert prep(rec, rt, lig, lt, edges, table)[0] == 0

    def mod(a, i, v):
        b = np.array(a, copy=True)
        b[i] = v
        return b
    # the edges
    assert err(rec, rt, lig, lt, edges, table, NB=0) == "need 1 <= NB <= 64" == err(rec, rt, lig, lt, edges, table, NB=65)
    assert err(rec, rt, lig, lt, None, table, NB=5) == "edges is NULL"
    assert err(rec, rt, lig, lt, mod(edges, 2, np.nan), table) == "edges: edge 2 is not finite" == err(rec, rt, lig, lt, mod(edges, 2, np.inf), table)
    assert err(rec, rt, lig, lt, mod(edges, 3, edges[2]), table) == "edges: edge 3 is not above edge 2"
    assert err(rec, rt, lig, lt, mod(edges, 1, edges[0] / 2), table) == "edges: edge 1 is not above edge 0"
    assert err(rec, rt, lig, lt, mod(edges, 0, -0.25), table) == "edges: edge 0 is below 0"
    assert err(rec, rt, lig, lt, mod(edges, 5, 16.5), table) == "edges: the last edge is above 16"
    assert prep(rec, rt, lig, lt, mod(mod(edges, 0, 0.0), 5, 16.0), table)[0] == 0
    # the table
    assert err(rec, rt, lig, lt, edges, None, T=3) == "table is NULL"
    assert err(rec, rt, lig, lt, edges, table, T=0) == "need 1 <= T <= 256" == err(rec, rt, lig, lt, edges, table, T=257)
    for v in (np.nan, np.inf, 1024.5, -1025.0):
        assert err(rec, rt, lig, lt, edges, mod(table, (1, 2, 3), v)) == f"table: entry {(1 * 3 + 2) * 5 + 3} is not in [-1024, 1024]"
    assert prep(rec, rt, lig, lt, edges, mod(mod(table, (0, 0, 0), 1024.0), (2, 2, 4), -1024.0))[0] == 0
    # the types, receptor first
    assert err(rec, mod(rt, 7, 3), lig, mod(lt, 2, -1), edges, table) == "rec_type: atom 7 has type 3 outside [0, 3)"
    assert err(rec, rt, lig, mod(lt, 2, -1), edges, table) == "lig_type: atom 2 has type -1 outside [0, 3)"
    # the atoms come before everything
    assert err(mod(rec, (3, 1), np.nan), rt, lig, lt, edges, table, NB=0) == "rec_atoms: atom 3 is not finite"
    wide = mod(rec, 0, 4000.0)      # 534^3 cells of 7.5 A > 2^24
    assert "more than 2^24 cells of the last edge" in err(wide, rt, lig, lt, mod(edges, 5, 7.5), table)


def test_transposition_quantisation_and_squared_edges_of_the_host_preparation(prep):
    from dfmdock_amd import pairpot as PP
    rec, rt, lig, lt, _, _, _, edges, table = toy(2, 50, 20, T=4, NB=6)
    table[0, 1, 2], table[1, 0, 2] = 7.0, -1024.0      # asymmetric for sure
    table[2, 3, 0], table[3, 2, 0] = np.float32(1.5 / Q), np.float32(2.5 / Q)      # ties: to even
    rc, out = prep(rec, rt, lig, lt, edges, table)
    assert rc == 0
    got = np.array([int(v) for v in out["table_q"]], np.int64).reshape(4, 4, 6)      # [tb][ta][bin]
    want = PP.quantise(table)                                                       # [ta][tb][bin]
    assert np.array_equal(got, want.transpose(1, 0, 2)) and not np.array_equal(got, want)
    assert got[3, 2, 0] == 2 and got[2, 3, 0] == 2 and got[0, 1, 2] == -(1 << 30)
    e2 = [float.fromhex(v) for v in out["e2"]]
    assert len(e2) == 128 and e2[:7] == PP.edges2(edges).tolist() and all(v == np.inf for v in e2[7:])
    # the receptor's type and slab offset ride in the cell order
    order = np.array([int(v) for v in out["order"]])
    assert np.array_equal(np.sort(order), np.arange(50))
    par = np.array([int(v) for v in out["rec_par"]]).reshape(50, 4)
    assert np.array_equal(par[:, 0], rt[order]) and np.array_equal(par[:, 1], rt[order] * 4 * 6) and not par[:, 2:].any()


def test_pair_bound_at_its_edge_and_the_chunk_rule(prep):
    """pairs <= Al min(Ar, 27 max_cell_atoms) must not exceed 2^31 - 1: then counts fits int32 and |energy_q| <= pairs 2^30 < 2^61."""
    top = (1 << 31) - 1
    assert prep.cmd("bound", top, 1, top)[1]["bound"] == ["2147483647", "1"]
    assert prep.cmd("bound", 1 << 30, 2, 1 << 30)[1]["bound"] == ["2147483648", "0"]
    assert prep.cmd("bound", 32767, 65536, 32767)[1]["bound"][1] == "1" and prep.cmd("bound", 32768, 65536, 32768)[1]["bound"][1] == "0"
    # 27 cells bound the pairs when the receptor is spread out
    assert prep.cmd("bound", 1 << 24, 1 << 20, 10)[1]["bound"] == [str(270 << 20), "1"]
    assert top * (1 << 30) < 1 << 61
    # the chunk: 64 MiB of counts plus per-atom output, whichever is asked for; without either the launch's 32768
    chunk = lambda *a: int(prep.cmd("chunk", *a)[1]["chunk"][0])
    assert chunk(2400, 20, 30, 0, 0) == 32768 and chunk(2400, 20, 30, 1, 0) == (64 << 20) // (2400 * 8)
    assert chunk(2400, 20, 30, 0, 1) == (64 << 20) // (20 * 20 * 30 * 4) and chunk(2400, 20, 30, 1, 1) == (64 << 20) // (20 * 20 * 30 * 4 + 2400 * 8)
    assert chunk(100, 256, 64, 0, 1) == 4 and chunk(1 << 24, 256, 64, 1, 1) == 1 and chunk(1, 1, 1, 1, 1) == 32768


def test_struct_layout_and_exports(tmp_path):
    """dfm_pairpot_out as gcc lays it out against the ctypes mirror; the new symbols are exported and listed; argument checks run before
    any device work."""
    from dfmdock_amd import _lib
    c_name, cls = "dfm_pairpot_out", _lib.PairpotOutC
    body = f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[c_name]) == C.sizeof(cls) == 32 and [f for f, _ in cls._fields_] == ["energy_q", "n_pairs", "lig_q", "counts"]
    for f, _ in cls._fields_:
        assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_pairpot_create", "dfm_pairpot_destroy", "dfm_pairpot_info", "dfm_pose_pairpot", "dfm_pose_pairpot_chunked", "dfm_pairpot_last_timing",
              "dfm_pairpot_last_phases"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and (getattr(lib, s).argtypes or s == "dfm_pairpot_destroy")
    from test_abi_cpu import header_symbols
    assert sorted(_lib.EXPORTS) == header_symbols()
    assert lib.dfm_pairpot_create(None, 1, None, None, 1, None, None, None, 1, 1, None, None, 0) is None
    assert b"m is NULL" in lib.dfm_last_error()
    assert lib.dfm_pose_pairpot(None, 1, None, None, None) == -1 and b"h is NULL" in lib.dfm_last_error()
    assert lib.dfm_pairpot_last_timing(None, None) == -1 and lib.dfm_pairpot_last_phases(None, None, None) == -1
    assert lib.dfm_pairpot_info(None, None, None, None, None, None, None) == -1


def test_the_audits_see_both_instantiations():
    """k_pairpot_pose and both instantiations of k_pairpot are in the shipped gfx950 code object (so the scratch / LDS / op_sel audits of
    test_abi_cpu.py run over them), use no scratch, and k_pairpot holds the two staged float4 arrays and the squared edges in LDS."""
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_pairpot.hip")).read()
    assert set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)) == {"k_pairpot_pose", "k_pairpot"}
    td = tempfile.mkdtemp()
    try:
        lib = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, lib)
        subprocess.run([os.path.join(tools, "llvm-objdump"), "--offloading", lib], cwd=td, check=True, capture_output=True)
        found = {}
        for f in sorted(os.listdir(td)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", os.path.join(td, f)], capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                for n, pat in (("k_pairpot_pose", r"\d+k_pairpot_poseE"), ("k_pairpot<true>", r"\d+k_pairpotILb1EE"), ("k_pairpot<false>", r"\d+k_pairpotILb0EE")):
                    if re.search(pat, name):
                        found[n] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in ("private_segment_fixed_size", "group_segment_fixed_size"))
        assert found == {"k_pairpot_pose": (0, 0), "k_pairpot<true>": (0, 3072), "k_pairpot<false>": (0, 3072)}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)


def seeded_potential(path=None, seed=0):
    """A seeded table file for tests: 20 residue types and a catch-all, 30 bins to 15 A, asymmetric, both signs.  Not a potential of
    any merit."""
    from dfmdock_amd import pairpot as PP
    rng = np.random.default_rng(seed)
    names = [r + ":*" for r in ("ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR",
                                "TRP", "TYR", "VAL")] + ["@N"]
    pot = {"edges": np.linspace(0.0, 15.0, 31).astype(np.float32), "table": rng.uniform(-1.0, 1.0, (21, 21, 30)).astype(np.float32), "type_names": names}
    if path is not None:
        PP.save(path, pot["edges"], pot["table"], names)
    return pot


def test_driver_inputs_and_selection_helpers(tmp_path):
    from dfmdock_amd import cli, driver
    from dfmdock_amd import pairpot as PP
    from dfmdock_amd import sterics as ST
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, _, _ = cli.load_pair(rec_pdb, lig_pdb, feat)
    pot = seeded_potential(str(tmp_path / "pot.npz"))
    ra, rt, la, lt, cen, lk, nu = driver.pairpot_inputs(rec, lig, 0, pot)
    sa = driver.sterics_inputs(rec, lig, 0)
    assert np.array_equal(ra, sa[0]) and np.array_equal(la, sa[1]) and np.array_equal(cen, sa[2]) and nu == 0      # every residue is one of the 20
    assert rt.shape == (ra.shape[0],) and lt.dtype == np.int32 and lt.max() < 21 and np.array_equal(lk, ST.heavy_atoms(lig["atoms"]))
    # a file whose names fit only part of the atoms: the others are left out and counted
    part = dict(pot, type_names=["@N"] + [f"X{i}:*" for i in range(20)])
    ra2, rt2, la2, lt2, _, lk2, nu2 = driver.pairpot_inputs(rec, lig, 0, part)
    assert 0 < ra2.shape[0] < ra.shape[0] and not rt2.any() and nu2 == (ra.shape[0] - ra2.shape[0]) + (la.shape[0] - la2.shape[0])
    with pytest.raises(ValueError):
        driver.pairpot_inputs(rec, lig, 0, dict(pot, type_names=[f"X{i}:*" for i in range(21)]))
    assert driver._check_pairpot(None, "energy") is None
    with pytest.raises(ValueError):
        driver._check_pairpot(None, "pairpot")
    by, p2 = driver._check_pairpot(str(tmp_path / "pot.npz"), "pairpot")
    assert by is True and p2["type_names"] == pot["type_names"] and np.array_equal(p2["table"], pot["table"])
    assert driver._check_pairpot(pot, "energy")[0] is False
    for bad in (dict(pot, edges=[0, 17]), dict(pot, table=pot["table"][:, :, :5]), dict(pot, type_names=pot["type_names"][:3])):
        with pytest.raises(ValueError):
            driver._check_pairpot(bad, "energy")
    driver._check_rank("pairpot", 1.0)
    pd = {"energy": np.array([1.5, -2.25]), "n_pairs": np.array([40, 9]), "n_untyped": 3, "T": 21, "NB": 30, "cutoff": 15.0}
    assert driver._pose_pairpot(pd, 1) == {"energy": -2.25, "n_pairs": 9, "n_untyped": 3, "T": 21, "NB": 30, "cutoff": 15.0}
    json.dumps(driver._pose_pairpot(pd, 0))
    off = driver._Run(None, type("G", (), {"lig_pos0": None}), None, None, None, "fp32", {"pairpot": None})      # off: no stage of _finish runs it
    off.k = 3
    [a.run(off) for a in driver.ANALYSES if a.name in off.opts]
    assert (off.k, off.key, off.data) == (3, None, {}) and not off.any() and driver._pairpot_result(None, 3) == {}


def test_every_summary_describes_the_kept_pose(tmp_path, monkeypatch):
    """_finish with the engine stubbed: under rank "pairpot" the `pair_potential`, `consensus` and `interface_energy` objects, `index` and
    the returned transform all belong to the one kept pose; ties go to the lower index; the clash filter's poses are out."""
    from dfmdock_amd import cli, driver
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, _, _ = cli.load_pair(rec_pdb, lig_pdb, feat)
    n = 5
    energy = np.float32([-5.0, -1.0, -2.0, -3.0, -4.0])      # energy keeps 0
    cons_score = np.array([0.1, 0.2, 0.9, 0.3, 0.4])         # consensus keeps 2
    total = np.array([3.0, 2.0, 1.0, -7.0, 0.5])             # interface keeps 3
    ppe = np.array([0.5, -6.0, 2.0, 1.0, -6.0])              # pairpot keeps 1 (the tie with 4 goes to the lower index)
    cols = {"energy": energy, "rot_update": 0.01 * np.arange(3 * n, dtype=np.float32).reshape(n, 3),
            "tr_update": np.arange(3 * n, dtype=np.float32).reshape(n, 3)}
    cd = lambda: {"consensus": cons_score.copy(), "n_contacts": np.arange(10, 10 + n), "M": n, "cutoff": 5.5}
    ed = {"rep": np.arange(n) + 0.5, "att": -np.arange(n) - 0.25, "elec": np.zeros(n), "total": total, "n_pairs": np.arange(100, 100 + n)}
    pd = {"energy": ppe, "energy_q": np.rint(ppe * Q).astype(np.int64), "n_pairs": np.arange(200, 200 + n), "n_untyped": 2, "T": 21, "NB": 30, "cutoff": 15.0}
    monkeypatch.setattr(driver, "ensemble_consensus", lambda *a, **k: cd())
    monkeypatch.setattr(driver, "ensemble_interface_energy", lambda *a, **k: dict(ed))
    monkeypatch.setattr(driver, "ensemble_pairpot", lambda *a, **k: dict(pd))

    class Gx:
        lig_pos0 = np.asarray(lig["bb_coords"], np.float32)

        def close(self):
            pass

    class Hp:
        family = 0
    model = type("M", (), {"hp": Hp})()
    pot = seeded_potential()

    def finish(rank, consensus, interface, pairpot, bad=None):
        cons = (rank, 5.5, 1.0) if consensus or rank == "consensus" else None
        ie = driver._check_interface(interface, rank, None, 8.0)
        pp_ = driver._check_pairpot(pot if pairpot else None, rank)
        if bad is not None:
            monkeypatch.setattr(driver, "_screen", lambda *a: ({"flags": bad, "n_clash": np.zeros(n, int), "n_contact": np.ones(n, int), "min_dist": np.ones(n),
                                                              "threshold": 1.0, "ensemble_mean": 0.0, "ensemble_std": 0.0, "clash_cutoff": 3.0,
                                                              "contact_cutoff": 5.0, "filtered": True, "fallback": False}, bad))
        run = driver._Run(model, Gx(), rec, lig, cols, "fp32", dict(consensus=cons, sterics=(True, 3.0, 5.0) if bad is not None else None, interface=ie,
                                                                    pairpot=pp_))
        run.key = energy
        return driver._finish(run, (np.argmin, "energy"), lambda k: {})
    for rank, want, by in (("energy", 0, "energy"), ("consensus", 2, "consensus"), ("interface", 3, "interface"), ("pairpot", 1, "pairpot")):
        r = finish(rank, True, True, True)
        assert r["index"] == want and np.array_equal(r["rot_update"], cols["rot_update"][want]) and r["energy"] == float(energy[want])
        assert r["pair_potential"] == {"energy": float(ppe[want]), "n_pairs": 200 + want, "n_untyped": 2, "T": 21, "NB": 30, "cutoff": 15.0}
        assert r["pairpot_data"]["energy"][r["index"]] == r["pair_potential"]["energy"]
        assert r["consensus"]["score"] == cons_score[want] and r["consensus"]["ranked_by"] == by and r["consensus"]["n_contacts"] == 10 + want
        assert r["interface_energy"]["total"] == total[want] and r["interface_energy"]["ranked_by"] == by and r["interface_energy"]["n_pairs"] == 100 + want
        assert set(r["trajectories"]) >= {"energy", "rot_update", "tr_update"}
    # the option alone; without it no key of it
    r = finish("pairpot", False, False, True)
    assert r["index"] == 1 and "consensus" not in r and "interface_energy" not in r and r["pair_potential"]["energy"] == -6.0
    r = finish("energy", False, False, True)
    assert r["index"] == 0 and r["pair_potential"]["energy"] == 0.5 and "trajectories" in r
    r = finish("interface", False, False, False)
    assert r["index"] == 3 and "pair_potential" not in r and "pairpot_data" not in r
    # the clash filter removes the pairpot pick: the other pose of the tie is kept
    bad = np.array([False, True, False, False, False])
    r = finish("pairpot", True, True, True, bad)
    assert r["index"] == 4 and r["pair_potential"]["energy"] == -6.0 and r["pair_potential"]["n_pairs"] == 204 and r["consensus"]["score"] == 0.4


def test_cli_flags_parse_default_off_and_reach_the_driver(tmp_path, monkeypatch, capsys):
    from dfmdock_amd import cli, driver, pdbio
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    pot_path = str(tmp_path / "pot.npz")
    pot = seeded_potential(pot_path)
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert a.pair_potential is None and a.rank == "energy" and a.pairpot_residues is None and a.pair_counts is None and cli.pairpot_kwargs(a) == {}
        a = cli.parse_args([cmd] + base + ["--pair-potential", pot_path])
        kw = cli.pairpot_kwargs(a)
        assert set(kw) == {"pair_potential", "rank"} and kw["rank"] == "energy" and kw["pair_potential"]["type_names"] == pot["type_names"]
        a = cli.parse_args([cmd] + base + ["--pair-potential", pot_path, "--rank", "pairpot", "--pairpot-residues", "r.txt", "--pair-counts", "c.npz"])
        assert cli.pairpot_kwargs(a)["rank"] == "pairpot" and not a.interface_energy and not a.consensus
        for bad in (["--rank", "pairpot"], ["--pairpot-residues", "r.txt"], ["--pair-counts", "c.npz"]):      # no file: refused
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c", "--pair-potential", pot_path])      # sweep is left alone: the DB5 files hold backbones only
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))
    obj = {"energy": -12.5, "n_pairs": 812, "n_untyped": 0, "T": 21, "NB": 30, "cutoff": 15.0}
    tj = {"energy": np.zeros(6, np.float32), "rot_update": 0.1 * np.arange(18, dtype=np.float32).reshape(6, 3), "tr_update": np.arange(18, dtype=np.float32).reshape(6, 3)}

    def dock_pair(model, rec, lig, rec_x, lig_x, **kw):
        seen.update(kw)
        res = {"energy": -1.5, "precision": "mfma16", "rot_update": tj["rot_update"][4], "tr_update": tj["tr_update"][4], "selfcheck": None}
        if kw.get("pair_potential") is not None:
            res.update(pair_potential=obj, index=4, trajectories={"energy": tj["energy"]}, pairpot_data=tj)      # the poses ride with the pair-potential data
        if kw.get("top_k"):
            res.update(models=[{"rank": 1, "index": 4, "energy": 0.0, "cluster_size": 3, "pair_potential": obj},
                               {"rank": 2, "index": 2, "energy": 0.0, "cluster_size": 2, "pair_potential": dict(obj, energy=-3.0)}], cluster_of=np.zeros(6, int))
        return res

    def residue_pairpot(model, rec, lig, rot, tr, p):
        seen["residue_call"] = (np.asarray(rot).tolist(), np.asarray(tr).tolist(), p["type_names"])
        keys = [tuple(k) for k in lig["residues"]]
        v = np.zeros(len(keys), np.int64)
        v[2] = -(5 << 18)
        return keys, v

    def ensemble_pairpot(model, rec, lig, rot, tr, p, per_atom=False, counts=False):
        seen["counts_call"] = (np.asarray(rot).tolist(), counts)
        n = np.asarray(rot).shape[0]
        c = np.zeros((n, 21, 21, 30), np.int32)
        c[:, 1, 2, 3] = np.arange(1, n + 1)
        return {"counts": c, "n_pairs": np.arange(1, n + 1, dtype=np.int64), "energy_q": np.zeros(n, np.int64)}
    monkeypatch.setattr(driver, "dock_pair", dock_pair)
    monkeypatch.setattr(driver, "residue_pairpot", residue_pairpot)
    monkeypatch.setattr(driver, "ensemble_pairpot", ensemble_pairpot)
    args = ["dock", rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb")]
    assert cli.main(args) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "pair_potential" not in plain and "index" not in plain and not any(k.startswith(("pair", "rank")) for k in seen)
    seen.clear()
    assert cli.main(args + ["--pair-potential", pot_path, "--rank", "pairpot", "--top-k", "2", "--pairpot-residues", str(tmp_path / "res.txt"),
                            "--pair-counts", str(tmp_path / "cnt.npz")]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["rank"] == "pairpot" and seen["pair_potential"]["type_names"] == pot["type_names"] and "interface_energy" not in seen
    assert line["pair_potential"] == obj and line["index"] == 4 and {k: v for k, v in line.items() if k in plain and k not in ("rot_update", "tr_update")} == \
        {k: v for k, v in plain.items() if k not in ("rot_update", "tr_update")}
    assert [m["pair_potential"]["energy"] for m in line["models"]] == [-12.5, -3.0]
    assert seen["residue_call"] == (tj["rot_update"][4].tolist(), tj["tr_update"][4].tolist(), pot["type_names"])
    assert os.path.samefile(line["pairpot_residues"], tmp_path / "res.txt") and os.path.samefile(line["pair_counts"], tmp_path / "cnt.npz")
    k = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))["residues"][2]
    assert (tmp_path / "res.txt").read_text().splitlines()[1:] == [f"{k[0]}:{k[1]} {k[3]} -1.250000"]
    # the kept pose first, then the models in their order
    assert seen["counts_call"] == (tj["rot_update"][[4, 4, 2]].tolist(), True)
    with np.load(tmp_path / "cnt.npz", allow_pickle=False) as z:
        assert z["counts"].shape == (3, 21, 21, 30) and z["counts"][:, 1, 2, 3].tolist() == [1, 2, 3] and z["index"].tolist() == [4, 4, 2]
        assert z["type_names"].tolist() == pot["type_names"] and np.array_equal(z["edges"], pot["edges"])


def test_pair_counts_with_restraints_engine_stubbed(tmp_path, monkeypatch, capsys):
    """`dock --restraints R --pair-potential F --pair-counts C` through the real cli and the real dock_pair with the engine stubbed: a
    restrained run's `trajectories` hold no transforms, so the counts' poses come from the pair-potential data itself."""
    from dfmdock_amd import cli, driver, engine
    from dfmdock_amd import restraints as RS
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    pot_path = str(tmp_path / "pot.npz")
    pot = seeded_potential(pot_path)
    n = 6
    rot = 0.1 * np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    tr = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    ppe = np.array([0.5, 2.0, -6.0, 1.0, -6.0, 3.0])      # pairpot keeps 2 (the tie with 4 goes to the lower index)
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()

    class Complex:
        def __init__(self, model, rec_x, lig_x, rec_bb, lig_bb):
            self.lig_pos0 = np.asarray(lig_bb, np.float32)

        def set_restraints(self, groups, params):
            seen["restraints"] = len(groups)

        def sample(self, B, **kw):
            assert B == n and kw["restraints"] is True
            return {"energy": np.float32([-5, -1, -2, -3, -4, -0.5]), "rot_update": rot, "tr_update": tr, "lig_pos": np.repeat(self.lig_pos0[None], n, 0)}

        def restraint_eval(self, lig_pos):
            return {"energy": np.zeros(n, np.float32), "n_satisfied": np.int32([1, 0, 0, 1, 0, 0])}

        def close(self):
            pass

    def ensemble_pairpot(model, rec, lig, rot_update, tr_update, p, per_atom=False, counts=False):
        m = np.asarray(rot_update).reshape(-1, 3).shape[0]
        if counts:
            seen["counts_call"] = np.asarray(rot_update).tolist()
            c = np.zeros((m, 21, 21, 30), np.int32)
            c[:, 0, 0, 0] = 7
            return {"counts": c, "n_pairs": np.full(m, 7, np.int64), "energy_q": np.zeros(m, np.int64)}
        assert m == n
        return {"energy": ppe, "energy_q": np.rint(ppe * Q).astype(np.int64), "n_pairs": np.arange(200, 200 + n), "n_untyped": 0, "T": 21, "NB": 30, "cutoff": 15.0}
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))
    monkeypatch.setattr(engine, "Complex", Complex)
    monkeypatch.setattr(RS, "read_restraints", lambda path, rec, lig: ["group"])
    monkeypatch.setattr(driver, "ensemble_pairpot", ensemble_pairpot)
    base = ["dock", rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb"), "--no-selfcheck", "--num-samples", str(n),
            "--restraints", "r.txt", "--pair-potential", pot_path, "--pair-counts", str(tmp_path / "cnt.npz")]
    # the restraint rule keeps its pose (satisfied first, then energy: 0); the counts are of that pose
    assert cli.main(base) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["restraints"] == 1 and line["index"] == 0 and line["restraints_satisfied"] == 1 and line["pair_potential"]["energy"] == 0.5
    assert seen["counts_call"] == [rot[0].tolist()]
    with np.load(tmp_path / "cnt.npz", allow_pickle=False) as z:
        assert z["index"].tolist() == [0] and z["counts"].shape == (1, 21, 21, 30) and z["counts"][0, 0, 0, 0] == 7
    # rank pairpot overrides the restraint rule
    assert cli.main(base + ["--rank", "pairpot"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["index"] == 2 and line["pair_potential"] == {"energy": -6.0, "n_pairs": 202, "n_untyped": 0, "T": 21, "NB": 30, "cutoff": 15.0}
    assert seen["counts_call"] == [rot[2].tolist()] and line["rot_update"] == [float(v) for v in rot[2]]
    with np.load(tmp_path / "cnt.npz", allow_pickle=False) as z:
        assert z["index"].tolist() == [2]
