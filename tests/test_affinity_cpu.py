"""The float64 definition of the residue contacts by class (dfmdock_amd/affinity.py), its host finishes, the limits and the preparation of
dfm_poseprep.h (tests/rescon_prep_main.cpp under the address and undefined-behaviour sanitizers) and the plumbing through the pair drivers
and the command line, on the CPU.  The GPU call is held against this definition in tests/test_gpu_affinity.py.  No test depends on the
published coefficients, class tables or reference areas being right: the arithmetic is pinned with arbitrary ones."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_pair
from conftest import ROOT, db5_complex, db5_ids

KEYS = ("ic", "n_pairs", "n_rec_res", "n_lig_res", "rec_degree", "lig_degree", "contact_bits")


def toy(seed, Ar=60, Al=45, Rr=14, Lr=9, P=5, sep=3.0):
    rng = np.random.default_rng(seed)
    rec = (4.0 * rng.standard_normal((Ar, 3))).astype(np.float32)
    lig = (4.0 * rng.standard_normal((Al, 3)) + np.float32([sep, 0, 0])).astype(np.float32)
    rot, tr = (0.4 * rng.standard_normal((P, 3))).astype(np.float32), (1.5 * rng.standard_normal((P, 3))).astype(np.float32)
    return (rec, rng.integers(0, Rr, Ar).astype(np.int32), rng.integers(0, 3, Rr).astype(np.uint8), lig, rng.integers(0, Lr, Al).astype(np.int32),
            rng.integers(0, 3, Lr).astype(np.uint8), lig.astype(np.float64).mean(0).astype(np.float32), rot, tr)


def brute_force(rec, rres, rcls, lig, lres, lcls, cen, rot, tr, cutoff=5.5):
    """Independent of the definition's vector code: every one of the Ar * Al distances in Python floats' arithmetic, a Python set of
    residue pairs."""
    from dfmdock_amd import pdbio
    ct = float(np.float32(cutoff))
    out = []
    for p in range(len(rot)):
        R = pdbio.axis_angle_to_matrix(np.asarray(rot[p]).reshape(3)).astype(np.float64)
        c = cen.astype(np.float64)
        X = (lig.astype(np.float64) - c) @ R.T + c + tr[p].astype(np.float64)
        pairs = set()
        for a in range(len(lig)):
            for b in range(len(rec)):
                dx, dy, dz = float(X[a, 0]) - float(rec[b, 0]), float(X[a, 1]) - float(rec[b, 1]), float(X[a, 2]) - float(rec[b, 2])
                if np.sqrt((dx * dx + dy * dy) + dz * dz) < ct:
                    pairs.add((int(rres[b]), int(lres[a])))
        ic = [0] * 6
        for i, j in pairs:
            lo, hi = sorted((int(rcls[i]), int(lcls[j])))
            ic[lo * (5 - lo) // 2 + hi] += 1
        out.append((pairs, ic))
    return out


def test_definition_against_brute_force():
    from dfmdock_amd import affinity as AF
    total = 0
    for seed in (1, 2, 3):
        cx = toy(seed, Rr=(14, 33, 65)[seed - 1])
        got = AF.residue_contacts(*cx, per_residue=True, bits=True)
        plain = AF.residue_contacts(*cx, per_residue=True, bits=True, shortcut=False)
        for k in KEYS:
            assert got[k].tobytes() == plain[k].tobytes() and got[k].dtype == (np.uint32 if k == "contact_bits" else np.int32), k
        Rr, Lr = len(cx[2]), len(cx[5])
        assert got["contact_bits"].shape == (5, Lr, (Rr + 31) // 32)
        for p, (pairs, ic) in enumerate(brute_force(*cx)):
            total += len(pairs)
            assert got["ic"][p].tolist() == ic and got["n_pairs"][p] == len(pairs) == sum(ic)
            assert got["n_rec_res"][p] == len({i for i, _ in pairs}) and got["n_lig_res"][p] == len({j for _, j in pairs})
            assert got["rec_degree"][p].tolist() == [sum(1 for i, _ in pairs if i == r) for r in range(Rr)]
            assert got["lig_degree"][p].tolist() == [sum(1 for _, j in pairs if j == r) for r in range(Lr)]
            assert [tuple(v) for v in AF.pairs_of(got["contact_bits"][p]).tolist()] == sorted(pairs, key=lambda q: (q[1], q[0]))
            assert np.array_equal(AF.unpack_bits(got["contact_bits"][p], Rr), AF.unpack_bits(AF.pack_bits(AF.unpack_bits(got["contact_bits"][p], Rr)), Rr))
        assert np.array_equal(AF.popcount(got["contact_bits"]), got["n_pairs"])
    assert total > 100
    # strict: d == cutoff is no pair, the float32 below is; NaN / inf poses give zeros
    below = np.nextafter(np.float32(5.5), np.float32(0))
    z = np.zeros((1, 3), np.float32)
    o = AF.residue_contacts(np.float32([[0, 0, 0]]), [0], [1], np.float32([[5.5, 0, 0], [0, below, 0]]), [0, 1], [0, 2], np.zeros(3, np.float32), z, z,
                            per_residue=True)
    assert o["lig_degree"][0].tolist() == [0, 1] and o["ic"][0].tolist() == [0, 0, 0, 0, 1, 0]
    cx = toy(4)
    rot, tr = cx[7].copy(), cx[8].copy()
    rot[1, 0], tr[3, 2] = np.nan, np.inf
    o = AF.residue_contacts(*cx[:7], rot, tr, per_residue=True, bits=True)
    clean = AF.residue_contacts(*cx, per_residue=True, bits=True)
    for k in KEYS:
        assert not o[k][[1, 3]].any() and np.array_equal(o[k][[0, 2, 4]], clean[k][[0, 2, 4]])


def test_invariances():
    from dfmdock_amd import affinity as AF
    rec, rres, rcls, lig, lres, lcls, cen, rot, tr = toy(7)
    rng = np.random.default_rng(8)
    base = AF.residue_contacts(rec, rres, rcls, lig, lres, lcls, cen, rot, tr, per_residue=True)
    assert base["n_pairs"].sum() > 50
    # the order of the atoms within the arrays
    pr, pl = rng.permutation(len(rec)), rng.permutation(len(lig))
    o = AF.residue_contacts(rec[pr], rres[pr], rcls, lig[pl], lres[pl], lcls, cen, rot, tr, per_residue=True)
    for k in KEYS[:6]:
        assert np.array_equal(o[k], base[k]), k
    # the names of the residues: new index = q[old]
    qr, ql = rng.permutation(len(rcls)), rng.permutation(len(lcls))
    rc2, lc2 = np.zeros_like(rcls), np.zeros_like(lcls)
    rc2[qr], lc2[ql] = rcls, lcls
    o = AF.residue_contacts(rec, qr[rres], rc2, lig, ql[lres], lc2, cen, rot, tr, per_residue=True)
    for k in KEYS[:4]:
        assert np.array_equal(o[k], base[k]), k
    assert np.array_equal(o["rec_degree"][:, qr], base["rec_degree"]) and np.array_equal(o["lig_degree"][:, ql], base["lig_degree"])
    # classes 0 <-> 2: AA <-> CC and AP <-> PC, AC and PP stay
    o = AF.residue_contacts(rec, rres, 2 - rcls, lig, lres, 2 - lcls, cen, rot, tr)
    assert np.array_equal(o["ic"], base["ic"][:, [5, 4, 2, 3, 1, 0]]) and np.array_equal(o["n_pairs"], base["n_pairs"])


def test_db5_recipe():
    """The DB5 recipe of tests/test_gpu_sterics.py with classes from the committed sequences through IC_CLASS: 17 012 residue pairs over 384
    poses, 4 of them empty, AA 4592, AP 4398, AC 3922, PP 970, PC 2102, CC 1028; no sequence letter is outside the 20."""
    from dfmdock_amd import affinity as AF
    from dfmdock_amd import pdbio
    rng = np.random.default_rng(0)
    ic, empty, missed, poses = np.zeros(6, np.int64), 0, 0, 0
    for cid in db5_ids():
        c = db5_complex(cid)
        rot, tr = np.zeros((16, 3), np.float32), np.zeros((16, 3), np.float32)
        for p in range(16):      # per pose an axis, an angle in [0, 0.3) and a translation of 2 A per axis; pose 0 is the identity
            ax = rng.standard_normal(3)
            ax /= np.linalg.norm(ax)
            ang = rng.uniform(0, 0.3)
            t = 2.0 * rng.standard_normal(3)
            if p == 0:
                ang, t = 0.0, np.zeros(3)
            rot[p], tr[p] = (ax * ang).astype(np.float32), t.astype(np.float32)
        rec, lig = pdbio.full_backbone(c["rec_pos"]).reshape(-1, 3), pdbio.full_backbone(c["lig_pos"]).reshape(-1, 3)
        rcls, m1 = AF.residue_classes(list(c["rec_seq"]), AF.IC_CLASS)
        lcls, m2 = AF.residue_classes(list(c["lig_seq"]), AF.IC_CLASS)
        cen = np.asarray(c["lig_pos"], np.float64)[:, 1].mean(0).astype(np.float32)
        o = AF.residue_contacts(rec, np.arange(len(rec)) // 5, rcls, lig, np.arange(len(lig)) // 5, lcls, cen, rot, tr)
        ic += o["ic"].sum(0)
        empty, missed, poses = empty + int((o["n_pairs"] == 0).sum()), missed + m1 + m2, poses + 16
    print(ic.tolist(), empty, missed)
    assert poses == 384 and missed == 0 and int(ic.sum()) == 17012 and empty == 4 and ic.tolist() == [4592, 4398, 3922, 970, 2102, 1028]


def test_host_finishes_on_hand_computed_cases(tmp_path):
    from dfmdock_amd import affinity as AF
    from dfmdock_amd import surface as SF
    # the tables hold the 20 names once each; MSE is MET; a one-letter code is widened
    assert sorted(AF.IC_CLASS) == sorted(AF.NIS_CLASS) == sorted(AF.REF_ASA) == sorted(AF.ONE_LETTER.values()) and len(AF.IC_CLASS) == 20
    cls, missed = AF.residue_classes(["mse", "M", "XYZ", " asp "], {"MET": 1, "ASP": 2}, other=0)
    assert cls.tolist() == [1, 1, 0, 2] and missed == 1 and cls.dtype == np.uint8
    assert AF.residue_classes(["XYZ"], {"MET": 1}, other=2)[0].tolist() == [2]
    # dg with arbitrary coefficients, every operation in float64 and in the stated order
    ic = np.array([[7, 5, 3, 2, 11, 4], [0, 0, 0, 0, 0, 0]])      # AA AP AC PP PC CC
    coef = (0.5, -0.25, 2.0, 0.125, 0.75, -1.5, 3.0)              # CC AC PP AP nis_a nis_c intercept
    want_c = ((0.5 * 4 + -0.25 * 3) + 2.0 * 2) + 0.125 * 5
    assert AF.dg_contacts(ic, coef).tolist() == [want_c, 0.0]
    assert AF.dg(ic, [40.0, 10.0], [20.0, 30.0], coef).tolist() == [((want_c + 0.75 * 40.0) + -1.5 * 20.0) + 3.0, ((0.0 + 7.5) - 45.0) + 3.0]
    assert np.isnan(AF.dg(ic[:1], [np.nan], [1.0], coef)[0])
    awkward = (0.1, 0.2, 0.3, 0.7, 1e-3, 1e3, -1e-7)
    a, q = 33.3, 17.9
    assert AF.dg(ic[:1], a, q, awkward)[0] == ((((0.1 * 4.0 + 0.2 * 3.0) + 0.3 * 2.0) + 0.7 * 5.0) + 1e-3 * a) + 1e3 * q + -1e-7
    with pytest.raises(ValueError):
        AF.dg(ic, [1.0, 1.0], [1.0, 1.0], coef[:6])
    assert len(AF.COEF) == 7
    # kd
    assert AF.kd(0.0) == 1.0 and AF.kd(-2.0, 10.0) == np.exp(-2.0 / (0.0019858775 * (10.0 + 273.15)))
    assert AF.kd(np.array([-1.0, -3.0])).tolist() == [np.exp(-1.0 / (0.0019858775 * (25.0 + 273.15))), np.exp(-3.0 / (0.0019858775 * (25.0 + 273.15)))]
    # nis_percent with an arbitrary table, reference areas and threshold
    table, ref = {"AAA": 0, "BBB": 1, "CCC": 2, "DDD": 2}, {"AAA": 100.0, "BBB": 200.0, "CCC": 50.0, "DDD": 10.0, "EEE": 10.0}
    rn, ln = ["AAA", "BBB", "CCC"], ["aaa", "DDD", "EEE", "FFF"]
    rs = np.array([[10.0, 19.9, 5.0], [9.99, 400.0, 4.99], [0.0, 0.0, 0.0]])
    ls = np.array([[50.0, 0.9, 9.0, 9.0], [0.0, 1.0, 9.0, 9.0], [9.9, 0.99, 99.0, 99.0]])
    got = AF.nis_percent(rs, ls, rn, ln, ref_asa=ref, threshold=0.1, table=table)
    # pose 0: AAA 0.1 on, BBB 0.0995 off, CCC 0.1 on | aaa on, DDD 0.09 off; EEE has no class and FFF no reference area: never -> 2 A, 0 P, 1 C
    # pose 1: BBB on, DDD 0.1 on -> 0 A, 1 P, 1 C;  pose 2: nothing on the surface
    assert got[0].tolist() == [100.0 * 2.0 / 3.0, 0.0, 100.0 * 1.0 / 3.0] and got[1].tolist() == [0.0, 50.0, 50.0] and np.isnan(got[2]).all()
    assert got.shape == (3, 3)
    with pytest.raises(ValueError):
        AF.nis_percent(rs, ls[:2], rn, ln, ref, 0.1, table)
    # complex_residue_sasa: (exposed - buried) points per radius value times the value's area, values ascending
    radius = np.float32([1.7, 1.52, 1.7, 1.52, 1.8])
    res, exposed = np.array([0, 0, 1, 1, 3]), np.array([10, 20, 30, 40, 50])
    buried = np.array([[1, 2, 3, 4, 5], [0, 0, 0, 0, 50]])
    ar = SF.class_areas(np.float32([1.52, 1.7, 1.8]), 1.4, 128)
    got = AF.complex_residue_sasa(exposed, buried, radius, res, 4, 1.4, 128)
    want = np.array([[(0.0 + 18 * ar[0]) + 9 * ar[1], (0.0 + 36 * ar[0]) + 27 * ar[1], 0.0, ((0.0 + 0.0) + 0.0) + 45 * ar[2]],
                     [(0.0 + 20 * ar[0]) + 10 * ar[1], (0.0 + 40 * ar[0]) + 30 * ar[1], 0.0, 0.0]])
    assert got.tolist() == want.tolist()
    # the residue file
    rk, lk = [("A", 10, " ", "ALA"), ("A", 11, "B", "ARG")], [("B", 5, " ", "GLU"), ("B", 6, " ", "TYR")]
    AF.write_contact_residues(str(tmp_path / "p.txt"), rk, lk, [[1, 0], [0, 1]])
    assert (tmp_path / "p.txt").read_text().splitlines()[1:] == ["A:11B ARG  B:5 GLU", "A:10 ALA  B:6 TYR"]
    AF.write_contact_residues(str(tmp_path / "e.txt"), rk, lk, np.zeros((0, 2), np.int32))
    assert len((tmp_path / "e.txt").read_text().splitlines()) == 1


def test_every_value_error_of_the_checkers():
    from dfmdock_amd import affinity as AF
    rec, rres, rcls, lig, lres, lcls, cen, rot, tr = toy(5)
    assert AF.check_cutoff(5.5) == 5.5 and AF.check_cutoff(16.0) == 16.0 and AF.check_cutoff(0.1) == float(np.float32(0.1))
    for bad in (0.0, -1.0, 16.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="cutoff"):
            AF.check_cutoff(bad)
    r, c = AF.check_residues(rres, len(rec), rcls, "rec")
    assert r.dtype == np.int32 and c.dtype == np.uint8

    def mod(a, i, v):
        q = np.asarray(a).astype(np.int64)
        q[i] = v
        return q
    for args, word in (((rres[:-1], len(rec), rcls), "one residue index per atom"), ((rres, len(rec), np.zeros(0, np.uint8)), "1 <= n_res <= 4096"),
                       ((rres, len(rec), np.zeros(4097, np.uint8)), "1 <= n_res <= 4096"), ((rres, len(rec), rcls.reshape(2, -1)), "1 <= n_res <= 4096"),
                       ((mod(rres, 3, len(rcls)), len(rec), rcls), "atom 3 has residue 14 outside"), ((mod(rres, 0, -1), len(rec), rcls), "atom 0 has residue -1"),
                       ((rres, len(rec), mod(rcls, 2, 3)), "residue 2 has class 3"), ((rres, len(rec), mod(rcls, 0, -1)), "residue 0 has class -1")):
        with pytest.raises(ValueError, match=word):
            AF.check_residues(*args, "rec")
    AF.check_residues(np.zeros(3, np.int32), 3, np.zeros(4096, np.uint8))
    assert AF.check_poses(1) == 1 and AF.check_poses(65536) == 65536
    for bad in (0, 65537):
        with pytest.raises(ValueError, match="65536"):
            AF.check_poses(bad)
    with pytest.raises(ValueError, match="rot and tr"):
        AF.residue_contacts(rec, rres, rcls, lig, lres, lcls, cen, rot, tr[:-1])
    with pytest.raises(ValueError, match="lig_res"):
        AF.residue_contacts(rec, rres, rcls, lig, lres[:-1], lcls, cen, rot, tr)
    with pytest.raises(ValueError, match="cutoff"):
        AF.residue_contacts(rec, rres, rcls, lig, lres, lcls, cen, rot, tr, cutoff=17.0)


def test_struct_layout_and_exports(tmp_path):
    """dfm_rescon_out as gcc lays it out against the ctypes mirror; the new symbols are exported and listed; argument checks run before
    any device work."""
    from dfmdock_amd import _lib
    c_name, cls = "dfm_rescon_out", _lib.ResconOutC
    body = f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[c_name]) == C.sizeof(cls) == 56
    for f, _ in cls._fields_:
        assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_rescon_create", "dfm_rescon_destroy", "dfm_rescon_info", "dfm_pose_rescon", "dfm_pose_rescon_chunked", "dfm_rescon_last_timing"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and (getattr(lib, s).argtypes or s == "dfm_rescon_destroy")
    from test_abi_cpu import header_symbols
    assert sorted(_lib.EXPORTS) == header_symbols()
    assert lib.dfm_rescon_create(None, 1, None, None, 1, None, 1, None, None, 1, None, None, 5.5) is None and b"m is NULL" in lib.dfm_last_error()
    assert lib.dfm_pose_rescon(None, 1, None, None, None) == -1 and b"h is NULL" in lib.dfm_last_error()
    assert lib.dfm_rescon_last_timing(None, None) == -1 and lib.dfm_rescon_info(None, None, None, None, None, None) == -1


def test_the_kernels_are_in_the_shipped_code_object():
    """The three kernels of kernels_rescon.hip are in the code object (so the scratch / LDS / op_sel audits of test_abi_cpu.py run over
    them), use no scratch, and k_rescon holds one staged float4 array in LDS."""
    import re
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(os.path.join(tools, "llvm-readelf")), "the ROCm llvm tools that built the library read its notes"
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_rescon.hip")).read()
    names = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))
    assert names == {"k_rescon_pose", "k_rescon", "k_rescon_finish"}
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
                for n in names:
                    if re.search(r"\d+" + n + r"E", name):
                        found[n] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in ("private_segment_fixed_size", "group_segment_fixed_size"))
        assert found == {"k_rescon_pose": (0, 0), "k_rescon": (0, 1024), "k_rescon_finish": (0, 0)}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    d = tmp_path_factory.mktemp("rescon_prep")
    exe = str(d / "rescon_prep")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "rescon_prep_main.cpp"), "-o", exe])

    def run(rec, rres, rcls, lig, lres, lcls, center=(0, 0, 0), cutoff=5.5, budget=64 << 20):
        path = str(d / "in.bin")
        n = (rec.shape[0], lig.shape[0], len(rcls), len(lcls))
        with open(path, "wb") as f:
            f.write(struct.pack("<iiii", *n) + np.float32(cutoff).tobytes() + np.float32(center).tobytes() + struct.pack("<q", budget))
            for xyz, res, cls in ((rec, rres, rcls), (lig, lres, lcls)):
                f.write(np.ascontiguousarray(xyz, np.float32).tobytes() + np.ascontiguousarray(res, np.int32).tobytes() + np.ascontiguousarray(cls, np.uint8).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.stderr == "", r.stderr      # a sanitizer report
        return r.returncode, {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    return run


def test_host_preparation_under_the_sanitizers(prep):
    """The residue indices follow the atoms through both sorts, the class masks match, the chunk size matches the budget, and every limit
    has its message."""
    i64 = lambda out, k: np.array([int(v) for v in out[k]], np.int64)
    for Rr, Al in ((1, 1), (31, 63), (32, 64), (33, 65), (65, 130)):
        rec, rres, rcls, lig, lres, lcls, cen, _, _ = toy(Rr, Ar=150, Al=Al, Rr=Rr, Lr=max(1, Al // 3))
        rc, out = prep(rec, rres, rcls, lig, lres, lcls, cen)
        assert rc == 0, out
        order, index = i64(out, "order"), i64(out, "lig_index")
        assert np.array_equal(np.sort(order), np.arange(150)) and np.array_equal(np.sort(index), np.arange(Al))
        assert np.array_equal(i64(out, "rec_res"), rres[order]) and np.array_equal(i64(out, "lig_res"), lres[index])
        assert np.array_equal(np.array([float(v) for v in out["rec_x"]], np.float32), rec[order, 0])      # next to the atom it belongs to
        W = (Rr + 31) // 32
        masks = np.zeros((3, W), np.uint64)
        for i, c in enumerate(rcls):
            masks[c, i >> 5] |= np.uint64(1 << (i & 31))
        assert np.array_equal(i64(out, "masks"), masks.reshape(-1).astype(np.int64)) and int(out["words"][0]) == W
        Lr = len(lcls)
        assert [int(v) for v in out["chunk"]] == [min(32768, max(1, (64 << 20) // (Lr * W * 4)))] * 2
    # the budget: 4096 x 4096 residues are 2 MiB of bitmap per pose
    rec, rres, rcls, lig, lres, lcls, cen, _, _ = toy(9)
    big = np.zeros(4096, np.uint8)
    for budget, want in ((64 << 20, 32), (2 << 20, 1), (1, 1), ((2 << 20) * 5 + 7, 5)):
        rc, out = prep(rec, rres, big, lig, lres, big, cen, budget=budget)
        assert rc == 0 and [int(v) for v in out["chunk"]] == [32, want]
    rc, out = prep(rec, rres, rcls, lig, lres, lcls, cen, budget=1 << 40)
    assert [int(v) for v in out["chunk"]] == [32768, 32768]
    # the limits, in the creator's order
    err = lambda *a, **k: " ".join(prep(*a, **k)[1].get("error", ["<none>"]))

    def mod(a, i, v):
        q = a.copy()
        q[i] = v
        return q
    assert err(rec, rres, rcls[:0], lig, lres, lcls, cen) == "rec: need 1 <= residues <= 4096"
    assert err(rec, rres, np.zeros(4097, np.uint8), lig, lres, lcls, cen) == "rec: need 1 <= residues <= 4096"
    assert err(rec, rres, rcls, lig, lres, np.zeros(4097, np.uint8), cen) == "lig: need 1 <= residues <= 4096"
    assert err(rec, mod(rres, 5, 14), rcls, lig, lres, lcls, cen) == "rec_res: atom 5 has residue 14 outside [0, 14)"
    assert err(rec, mod(rres, 0, -1), rcls, lig, lres, lcls, cen) == "rec_res: atom 0 has residue -1 outside [0, 14)"
    assert err(rec, rres, rcls, lig, mod(lres, 44, 9), lcls, cen) == "lig_res: atom 44 has residue 9 outside [0, 9)"
    assert err(rec, rres, mod(rcls, 13, 3), lig, lres, lcls, cen) == "rec_class: residue 13 has class 3, not 0, 1 or 2"
    assert err(rec, rres, rcls, lig, lres, mod(lcls, 0, 255), cen) == "lig_class: residue 0 has class 255, not 0, 1 or 2"
    for cut in (0.0, 16.5, np.nan, -3.0):
        assert err(rec, rres, rcls, lig, lres, lcls, cen, cutoff=cut) == "cutoff must be in (0, 16]"
    assert prep(rec, rres, rcls, lig, lres, lcls, cen, cutoff=16.0)[0] == 0
    bad = rec.copy()
    bad[3, 1] = np.nan
    assert err(bad, rres, rcls, lig, lres, lcls, cen) == "rec_atoms: atom 3 is not finite"


def _pair(tmp_path):
    from dfmdock_amd import cli
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    return cli.load_pair(rec_pdb, lig_pdb, feat)[:2], (rec_pdb, lig_pdb, feat)


def test_driver_inputs(tmp_path):
    from dfmdock_amd import affinity as AF
    from dfmdock_amd import driver
    (rec, lig), _ = _pair(tmp_path)
    ra, rres, rcls, la, lres, lcls, cen, rk, lk, missed = driver.rescon_inputs(rec, lig, 0)
    assert missed == (0, 0)
    odd = dict(rec, atoms=[dict(a, res_name="SEP") if a["res_id"] == rec["atoms"][0]["res_id"] else a for a in rec["atoms"]])
    o2 = driver.rescon_inputs(odd, lig, 0)
    assert o2[9] == (1, 0) and o2[2][0] == 0 and o2[7][0][3] == "SEP"      # a name outside the 20 counts as apolar, and is counted
    sa = driver.sterics_inputs(rec, lig, 0)
    assert np.array_equal(ra, sa[0]) and np.array_equal(la, sa[1]) and np.array_equal(cen, sa[2])
    AF.check_residues(rres, len(ra), rcls, "rec")
    AF.check_residues(lres, len(la), lcls, "lig")
    assert len(rk) == len(rcls) == rres.max() + 1 and len(lk) == len(lcls) == lres.max() + 1 and rres.dtype == np.int32
    assert rcls.tolist() == [AF.IC_CLASS.get(k[3], 0) for k in rk] and (np.diff(rres) >= 0).all()
    assert driver._check_affinity(False, 5.5) is None and driver._check_affinity(True, 6.0) == (6.0,)
    with pytest.raises(ValueError):
        driver._check_affinity(True, 20.0)
    ad = {"ic": np.array([[1, 2, 3, 4, 5, 6], [0] * 6]), "n_pairs": np.array([21, 0]), "n_rec_res": np.array([9, 0]), "n_lig_res": np.array([8, 0]),
          "nis_apolar": np.array([40.0, np.nan]), "nis_charged": np.array([25.0, np.nan]), "dg": np.array([-9.5, np.nan]), "kd": np.array([1e-7, np.nan]),
          "cutoff": 5.5}
    assert driver._pose_affinity(ad, 0) == {"ic": [1, 2, 3, 4, 5, 6], "n_pairs": 21, "n_rec_res": 9, "n_lig_res": 8, "nis_apolar": 40.0,
                                           "nis_charged": 25.0, "dg": -9.5, "kd": 1e-7, "cutoff": 5.5}
    assert driver._pose_affinity(ad, 1)["dg"] is None and json.loads(json.dumps(driver._pose_affinity(ad, 1)))["kd"] is None
    assert driver._affinity_result(None, 3) == {}


def test_pair_drivers_share_one_path(tmp_path, monkeypatch):
    """_finish with the engine stubbed: `affinity` describes the kept pose, `affinity_data` holds every trajectory, every model gains the
    object, and without the option nothing is added."""
    from dfmdock_amd import driver
    (rec, lig), _ = _pair(tmp_path)
    n = 5
    energy = np.float32([-1.0, -5.0, -2.0, -3.0, -4.0])
    cols = {"energy": energy, "rot_update": 0.01 * np.arange(3 * n, dtype=np.float32).reshape(n, 3), "tr_update": np.arange(3 * n, dtype=np.float32).reshape(n, 3)}
    ad = {"ic": np.arange(6 * n).reshape(n, 6), "n_pairs": np.arange(6 * n).reshape(n, 6).sum(1), "n_rec_res": np.arange(n), "n_lig_res": np.arange(n) + 1,
          "nis_apolar": np.linspace(30, 40, n), "nis_charged": np.linspace(20, 25, n), "dg": -np.arange(n) - 7.0, "kd": np.full(n, 1e-6),
          "dg_contacts": np.arange(n) * 0.5, "cutoff": 6.0}
    seen = {}

    def pose_affinity(model, rec_, lig_, rot, tr, cutoff, probe, points, surface=None):
        seen["args"] = (np.asarray(rot).shape, np.asarray(tr).shape, cutoff)
        seen["surface"] = surface
        return dict(ad)
    monkeypatch.setattr(driver, "pose_affinity", pose_affinity)
    monkeypatch.setattr(driver, "cluster_trajectories", lambda *a, **k: {"center": np.array([1, 3]), "size": np.array([3, 2]), "cluster_of": np.array([1, 0, 0, 1, 0])})

    class Gx:
        lig_pos0 = np.asarray(lig["bb_coords"], np.float32)

        def close(self):
            pass
    model = type("M", (), {"hp": type("Hp", (), {"family": 0})})()
    def fin(clu=None, **opts):
        run = driver._Run(model, Gx(), rec, lig, cols, "fp32", opts)
        run.key = energy
        return driver._finish(run, (np.argmin, "energy"), lambda k: {}, clu)
    r = fin()
    assert "affinity" not in r and "affinity_data" not in r and "index" not in r and "args" not in seen
    r = fin(affinity=driver._check_affinity(True, 6.0), clu=(2, 4.0, "energy"))
    assert seen["args"] == ((n, 3), (n, 3), 6.0) and r["index"] == 1 and r["affinity"] == driver._pose_affinity(ad, 1)
    assert r["affinity_data"]["dg_contacts"].tolist() == ad["dg_contacts"].tolist() and set(r["trajectories"]) == {"energy", "rot_update", "tr_update"}
    assert [m["index"] for m in r["models"]] == [1, 3] and all(m["affinity"] == driver._pose_affinity(ad, m["index"]) for m in r["models"])
    json.dumps(r["affinity"])
    assert seen["surface"] is None
    # with the surface option at the estimate's own probe and points ONE surface call serves both; with others each makes its own
    calls = []

    def ensemble_surface(model, rec_, lig_, rot, tr, probe, points, per_atom=False):
        calls.append((probe, points, per_atom))
        return {"bsa": np.arange(n) * 100.0, "bsa_rec": np.arange(n) * 50.0, "bsa_lig": np.arange(n) * 50.0, "probe": probe, "sphere_points": points,
                "tag": len(calls)}
    monkeypatch.setattr(driver, "ensemble_surface", ensemble_surface)
    r = fin(affinity=driver._check_affinity(True, 5.5), surface=driver._check_surface(True, None, 1.4, 128))
    assert calls == [(float(np.float32(1.4)), 128, True)] and seen["surface"]["tag"] == 1 and r["bsa"] == 100.0 and r["affinity"]["n_pairs"] == int(ad["n_pairs"][1])
    calls.clear()
    r = fin(affinity=driver._check_affinity(True, 5.5), surface=driver._check_surface(True, None, 1.2, 64))
    assert calls == [(float(np.float32(1.2)), 64, False)] and seen["surface"] is None and r["sphere_points"] == 64


def test_cli_flags_parse_default_off_and_reach_the_driver(tmp_path, monkeypatch, capsys):
    from dfmdock_amd import cli, driver
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert not a.affinity and a.contact_residues is None and cli.affinity_kwargs(a) == {}
        assert cli.affinity_kwargs(cli.parse_args([cmd] + base + ["--affinity"])) == dict(affinity=True, affinity_cutoff=5.5)
        assert cli.affinity_kwargs(cli.parse_args([cmd] + base + ["--affinity", "--affinity-cutoff", "6.5"])) == dict(affinity=True, affinity_cutoff=6.5)
        assert cli.parse_args([cmd] + base + ["--contact-residues", "x.txt"]).affinity
        for bad in (["--affinity-cutoff", "6"], ["--affinity", "--affinity-cutoff", "17"], ["--affinity", "--affinity-cutoff", "nan"],
                    ["--affinity", "--affinity-cutoff", "0"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c", "--affinity"])
    (rec, lig), (rec_pdb, lig_pdb, feat) = _pair(tmp_path)
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))
    af = {"ic": [3, 2, 1, 0, 4, 5], "n_pairs": 15, "n_rec_res": 7, "n_lig_res": 6, "nis_apolar": 38.5, "nis_charged": 27.25, "dg": -9.125, "kd": 2.5e-7,
          "cutoff": 5.5}

    def pair(model, rec, lig, rec_x, lig_x, **kw):
        seen.update(kw)
        res = {"energy": -1.5, "precision": "mfma16", "rot_update": np.zeros(3, np.float32), "tr_update": np.ones(3, np.float32), "selfcheck": None,
               "t_begin": 0.1, "index": 0, "trajectories": {"energy": np.zeros(1)}}
        if kw.get("affinity"):
            res.update(affinity=af, index=4, affinity_data={"unclassified": (0, 2) if kw["affinity_cutoff"] == 6.0 else (0, 0)})
        return res
    rk, lk = driver.rescon_inputs(rec, lig, 0)[7:9]

    def ensemble_contacts(model, rec, lig, rot, tr, cutoff, bits=False):
        from dfmdock_amd import affinity as AF
        seen["contacts_call"] = (np.asarray(rot).tolist(), np.asarray(tr).tolist(), cutoff, bits)
        m = np.zeros((len(lk), len(rk)), bool)
        m[2, 40], m[0, 3] = True, True
        return {"contact_bits": AF.pack_bits(m)[None], "rec_keys": rk, "lig_keys": lk}
    monkeypatch.setattr(driver, "dock_pair", pair)
    monkeypatch.setattr(driver, "refine_pair", pair)
    monkeypatch.setattr(driver, "ensemble_contacts", ensemble_contacts)
    for cmd in ("dock", "refine"):
        args = [cmd, rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb")]
        seen.clear()
        assert cli.main(args) == 0
        plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert "affinity" not in plain and not any(k.startswith("affinity") for k in seen)
        assert cli.main(args + ["--contact-residues", str(tmp_path / "pairs.txt"), "--affinity-cutoff", "6"]) == 0
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert seen["affinity"] is True and seen["affinity_cutoff"] == 6.0 and line["affinity"] == af and line["index"] == 4
        assert line["affinity_unclassified"] == [0, 2]
        assert {k: v for k, v in line.items() if k in plain and k != "index"} == {k: v for k, v in plain.items() if k != "index"}
        assert seen["contacts_call"] == ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 6.0, True) and os.path.samefile(line["contact_residues"], tmp_path / "pairs.txt")
        fmt = lambda k: f"{k[0]}:{k[1]} {k[3]}"
        assert (tmp_path / "pairs.txt").read_text().splitlines()[1:] == [f"{fmt(rk[3])}  {fmt(lk[0])}", f"{fmt(rk[40])}  {fmt(lk[2])}"]
