"""The float64 definition of the interface energy (dfmdock_amd/ifenergy.py), its host finishes, the parameter and overflow checks of
dfm_poseprep.h (tests/iface_prep_main.cpp under the address and undefined-behaviour sanitizers) and the command-line plumbing, on the
CPU.  The GPU call is held against this definition in tests/test_gpu_ifenergy.py."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_pair
from conftest import ROOT

Z3 = np.zeros((1, 3), np.float32)
Q = 2.0 ** 20
CARBON = np.float32([1.9080, np.sqrt(np.float64(0.0860)), 0.0])


def one(rec, rp, lig, lp, center=(0, 0, 0), rot=Z3, tr=Z3, **kw):
    from dfmdock_amd import ifenergy as IE
    f = lambda a, n: np.asarray(a, np.float32).reshape(-1, n)
    return IE.interface_energy(f(rec, 3), f(rp, 3), f(lig, 3), f(lp, 3), np.asarray(center, np.float32), rot, tr, per_atom=True, **kw)


def test_hand_computed_pairs():
    # one C-C pair at r = Rmin: s2 = 1 exactly, so rep = e and att = -2 e with e = sqrt_eps^2 of the float32 sqrt_eps
    rmin = 2.0 * float(CARBON[0])
    e = float(CARBON[1]) * float(CARBON[1])
    o = one([[0, 0, 0]], [CARBON], [[rmin, 0, 0]], [CARBON])
    assert o["n_pairs"].tolist() == [1] and o["rep_q"][0] == round(e * Q) and o["att_q"][0] == round(-2.0 * e * Q) and o["elec_q"][0] == 0
    assert abs(e - 0.0860) < 1e-8 and o["lig_vdw_q"].tolist() == [[int(o["rep_q"][0] + o["att_q"][0])]] and o["rep_q"].dtype == np.int64
    # exactly r2 == cutoff^2 is no pair (strict); the next float below is one
    below = np.nextafter(np.float32(8.0), np.float32(0.0))
    o = one([[0, 0, 0]], [CARBON], [[8.0, 0, 0], [0, below, 0]], [CARBON, CARBON])
    assert o["n_pairs"].tolist() == [1] and o["lig_vdw_q"][0, 0] == 0 and o["lig_vdw_q"][0, 1] != 0
    o = one([[0, 0, 0]], [CARBON], [[5.0, 0, 0], [0, np.nextafter(np.float32(5.0), np.float32(0.0)), 0]], [CARBON, CARBON], cutoff=5.0)
    assert o["n_pairs"].tolist() == [1] and o["lig_vdw_q"][0, 0] == 0
    # coincident atoms: r2 = 0 lands on the soft floor (soft Rm)^2 and on the elec floor m^2
    a, b = np.float32([1.5, 0.5, 1.0]), np.float32([2.0, 0.25, -0.5])
    o = one([[1, 2, 3]], [a], [[1, 2, 3]], [b])
    Rm = 3.5
    f = float(np.float32(0.6)) * Rm
    s2 = (Rm * Rm) / (f * f)
    s6 = (s2 * s2) * s2
    assert o["rep_q"][0] == round(0.125 * (s6 * s6) * Q) and o["att_q"][0] == round(-2.0 * (0.125 * s6) * Q)
    assert o["elec_q"][0] == round(((332.0637 / 4.0) * (-0.5)) / 9.0 * Q) and o["n_pairs"][0] == 1
    # like charges repel, unlike attract, by the same magnitude; no charge: elec_q == 0 whatever the rest
    plus, minus, none = np.float32([1.8, 0.4, 1.0]), np.float32([1.8, 0.4, -1.0]), np.float32([1.8, 0.4, 0.0])
    like, unlike = one([[0, 0, 0]], [plus], [[4, 0, 0]], [plus]), one([[0, 0, 0]], [plus], [[4, 0, 0]], [minus])
    assert like["elec_q"][0] == round((332.0637 / 4.0) / 16.0 * Q) == -unlike["elec_q"][0] and like["rep_q"][0] == unlike["rep_q"][0]
    assert one([[0, 0, 0]], [plus], [[4, 0, 0]], [none])["elec_q"][0] == 0 and one([[0, 0, 0]], [none], [[1, 0, 0]], [minus])["elec_q"][0] == 0
    # inside elec_min_dist the Coulomb term stays at its value there
    near = one([[0, 0, 0]], [plus], [[2, 0, 0]], [plus])
    assert near["elec_q"][0] == round((332.0637 / 4.0) / 9.0 * Q)
    # a non-finite pose gets zeros; the others are not disturbed
    o = one([[0, 0, 0]], [plus], [[4, 0, 0]], [plus], rot=np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0]]), tr=np.float32([[0, 0, 0], [0, 0, 0], [np.inf, 0, 0]]))
    assert o["n_pairs"].tolist() == [1, 0, 0] and o["elec_q"][0] == like["elec_q"][0] and not o["lig_vdw_q"][1:].any()


def toy(seed=0, Ar=7, Al=5):
    rng = np.random.default_rng(seed)
    rec, lig = (4.0 * rng.random((Ar, 3))).astype(np.float32), (4.0 * rng.random((Al, 3)) + 2.0).astype(np.float32)
    par = lambda n: np.stack([rng.uniform(1.5, 2.1, n), rng.uniform(0.2, 0.5, n), rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], n)], 1).astype(np.float32)
    rot, tr = (0.4 * rng.standard_normal((3, 3))).astype(np.float32), rng.standard_normal((3, 3)).astype(np.float32)
    return rec, par(Ar), lig, par(Al), lig.mean(0), rot, tr


def test_triple_loop_in_python_floats_equals_the_vectorised_definition():
    from dfmdock_amd import ifenergy as IE
    from dfmdock_amd import sterics as ST
    rec, rp, lig, lp, cen, rot, tr = toy()
    kw = dict(cutoff=6.0, soft=0.7, elec_min_dist=2.0, dielectric_slope=3.0)
    got = IE.interface_energy(rec, rp, lig, lp, cen, rot, tr, per_atom=True, **kw)
    cut, soft, m, slope = (float(np.float32(v)) for v in (6.0, 0.7, 2.0, 3.0))
    pairs = 0
    for p in range(3):
        X = ST.pose_atoms(lig, cen, rot[p], tr[p])
        tot, vdw, el = [0, 0, 0], [0] * 5, [0] * 5
        for a in range(5):
            for b in range(7):
                dx, dy, dz = (float(X[a, k]) - float(rec[b, k]) for k in range(3))
                r2 = (dx * dx + dy * dy) + dz * dz
                if not r2 < cut * cut:
                    continue
                Rm = float(lp[a, 0]) + float(rp[b, 0])
                f = soft * Rm
                r2v = f * f if r2 < f * f else r2
                s2 = (Rm * Rm) / r2v
                s6 = (s2 * s2) * s2
                e = float(lp[a, 1]) * float(rp[b, 1])
                r2c = m * m if r2 < m * m else r2
                q = [round(e * (s6 * s6) * Q), round(-2.0 * (e * s6) * Q), round(((332.0637 / slope) * (float(lp[a, 2]) * float(rp[b, 2]))) / r2c * Q)]
                tot = [t + v for t, v in zip(tot, q)]
                vdw[a] += q[0] + q[1]
                el[a] += q[2]
                pairs += 1
        assert [int(got[k][p]) for k in ("rep_q", "att_q", "elec_q")] == tot and got["lig_vdw_q"][p].tolist() == vdw and got["lig_elec_q"][p].tolist() == el
    assert int(got["n_pairs"].sum()) == pairs and 20 < pairs < 105


def test_the_bounding_box_shortcut_changes_nothing():
    from dfmdock_amd import ifenergy as IE
    rec, rp, lig, lp, cen, rot, tr = toy(3, 300, 90)
    rec = (rec * np.float32(8.0)).astype(np.float32)      # a 32 A box: most receptor atoms are out of reach of the ligand
    tr = np.concatenate([tr, np.float32([[60, 0, 0]])])      # and one pose out of reach altogether
    rot = np.concatenate([rot, np.zeros((1, 3), np.float32)])
    a = IE.interface_energy(rec, rp, lig, lp, cen, rot, tr, per_atom=True)
    b = IE.interface_energy(rec, rp, lig, lp, cen, rot, tr, per_atom=True, shortcut=False)
    assert a["n_pairs"][:3].min() > 0 and a["n_pairs"][3] == 0 and all(a[k].tobytes() == b[k].tobytes() for k in a)
    X = lig.astype(np.float64)
    sa, sb, sr = IE.near_r2(rec, X, 8.0)
    fa, fb, fr = IE.near_r2(rec, X, 8.0, shortcut=False)
    assert np.array_equal(sa, fa) and np.array_equal(sb, fb) and sr.tobytes() == fr.tobytes() and 0 < sr.size < 300 * 90


def pdb_line(k, name, res, chain, num, xyz, el, het=False):
    return "%-6s%5d %-4s %3s %s%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s\n" % (
        "HETATM" if het else "ATOM", k, name if len(name) == 4 else " " + name, res, chain, num, xyz[0], xyz[1], xyz[2], 1.0, 0.0, el)


def test_atom_parameters_on_a_written_pdb(tmp_path):
    from dfmdock_amd import ifenergy as IE
    from dfmdock_amd import pdbio
    from dfmdock_amd import sterics as ST
    rows = [("N", "MET", "A", 1, "N"), ("CA", "MET", "A", 1, "C"), ("C", "MET", "A", 1, "C"), ("O", "MET", "A", 1, "O"), ("SD", "MET", "A", 1, "S"),
            ("H", "MET", "A", 1, "H"),
            ("N", "ASP", "A", 2, "N"), ("OD1", "ASP", "A", 2, "O"), ("OD2", "ASP", "A", 2, "O"),
            ("OE1", "GLU", "A", 3, "O"), ("OE2", "GLU", "A", 3, "O"), ("NZ", "LYS", "A", 4, "N"), ("NH1", "ARG", "A", 5, "N"), ("NH2", "ARG", "A", 5, "N"),
            ("NE", "ARG", "A", 5, "N"), ("O", "GLY", "A", 6, "O"), ("OXT", "GLY", "A", 6, "O"), ("ZN", "GLY", "A", 6, "ZN"), ("SE", "MSE", "A", 7, ""),
            ("P", "SEP", "A", 8, "P"), ("N", "ALA", "B", 1, "N"), ("O", "ALA", "B", 1, "O"), ("N", "ALA", "B", 2, "N")]
    path = tmp_path / "x.pdb"
    path.write_text("".join(pdb_line(k + 1, *r[:4], (k, 0, 0), r[4]) for k, r in enumerate(rows)) + pdb_line(99, "O", "HOH", "A", 9, (0, 0, 0), "O", True))
    atoms = pdbio.read_pdb(str(path))
    idx = ST.heavy_atoms(atoms)
    par = IE.atom_parameters(atoms)
    assert par.dtype == np.float32 and par.shape == (22, 3) and np.array_equal(par, IE.atom_parameters(atoms, idx))
    by = {(atoms[i]["chain"], atoms[i]["res_id"], atoms[i]["name"]): par[n] for n, i in enumerate(idx)}
    lj = lambda rh, eps: [np.float32(rh), np.float32(np.sqrt(np.float64(eps)))]
    assert by[("A", 1, "N")].tolist() == lj(1.8240, 0.1700) + [1.0] and by[("B", 1, "N")][2] == 1.0 and by[("A", 2, "N")][2] == 0 and by[("B", 2, "N")][2] == 0
    assert by[("A", 1, "CA")].tolist() == lj(1.9080, 0.0860) + [0.0] and by[("A", 1, "O")].tolist() == lj(1.6612, 0.2100) + [0.0]
    assert by[("A", 1, "SD")].tolist() == lj(2.0, 0.25) + [0.0] and by[("A", 7, "SE")].tolist() == lj(2.0, 0.25) + [0.0]
    assert by[("A", 8, "P")].tolist() == lj(2.1, 0.2) + [0.0] and by[("A", 6, "ZN")].tolist() == lj(2.0, 0.2) + [0.0]
    assert [by[("A", 2, n)][2] for n in ("OD1", "OD2")] == [-0.5, -0.5] and [by[("A", 3, n)][2] for n in ("OE1", "OE2")] == [-0.5, -0.5]
    assert by[("A", 4, "NZ")][2] == 1.0 and [by[("A", 5, n)][2] for n in ("NH1", "NH2", "NE")] == [0.5, 0.5, 0.0]
    assert [by[("A", 6, n)][2] for n in ("O", "OXT")] == [-0.5, -0.5] and by[("B", 1, "O")][2] == 0
    IE.check_params(par, 22)


def test_total_residue_sums_and_checks(tmp_path):
    from dfmdock_amd import ifenergy as IE
    rep, att, elec = np.array([10.0, 0.5]), np.array([-3.0, -8.0]), np.array([2.0, -4.0])
    assert IE.WEIGHTS == (0.18, 1.0, 0.5) and IE.total(rep, att, elec).tolist() == [(0.18 * 10.0 + -3.0) + 1.0, (0.18 * 0.5 + -8.0) + -2.0]
    assert IE.total(rep, att, elec, (1, 0, 0)).tolist() == rep.tolist() and IE.total(1.0, 2.0, 3.0, (1, 1, 1)) == 6.0
    assert "NOT fitted" in IE.total.__doc__
    for bad in ((1, 2), (1, 2, np.nan)):
        with pytest.raises(ValueError):
            IE.total(rep, att, elec, bad)
    assert IE.kcal(np.int64([1 << 20, -(1 << 19)])).tolist() == [1.0, -0.5]
    assert IE.quantise([0.5 / Q, 1.5 / Q, 2.5 / Q, -0.5 / Q, -1.5 / Q]).tolist() == [0, 2, 2, 0, -2]      # ties to even
    res = np.array([0, 0, 1, 2, 2, 2])
    assert IE.residue_energy(np.int64([5, -7, 3, 0, 1, 1]), res, 4).tolist() == [-2, 3, 2, 0]
    assert IE.residue_energy(np.int64([[1, 1, 1, 1, 1, 1], [2, 0, 0, 0, 0, -2]]), res, 3).tolist() == [[2, 1, 3], [2, 0, -2]]
    out = tmp_path / "e.txt"
    IE.write_energy_residues(str(out), [("B", 7, " ", "LYS"), ("B", 8, "A", "GLY"), ("B", 9, " ", "ASP")], np.int64([-(3 << 19), 0, 0]), np.int64([1 << 20, 0, -1]))
    assert out.read_text().splitlines()[1:] == ["B:7 LYS -1.500000 1.000000", "B:9 ASP 0.000000 -0.000001"]
    for kw in (dict(cutoff=0.0), dict(cutoff=17.0), dict(soft=0.4), dict(soft=1.5), dict(elec_min_dist=0.5), dict(dielectric_slope=0.0), dict(cutoff=np.nan)):
        with pytest.raises(ValueError):
            IE.check_scalars(**kw)
    assert IE.check_scalars() == (8.0, float(np.float32(0.6)), 3.0, 4.0)
    ok = np.float32([[1.9, 0.3, 0.5]])
    for bad in ([[0.0, 0.3, 0.5]], [[8.5, 0.3, 0.5]], [[1.9, -0.1, 0.5]], [[1.9, 2.5, 0.5]], [[1.9, 0.3, 4.5]], [[np.nan, 0.3, 0.5]], [[1.9, 0.3]]):
        with pytest.raises(ValueError):
            IE.check_params(np.float32(bad), 1)
    assert IE.check_params(ok, 1) is not None


def test_struct_layout_and_exports(tmp_path):
    """dfm_iface_out as gcc lays it out against the ctypes mirror; the new symbols are exported and listed; argument checks run before
    any device work."""
    from dfmdock_amd import _lib
    c_name, cls = "dfm_iface_out", _lib.IfaceOutC
    body = f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[c_name]) == C.sizeof(cls) == 48
    for f, _ in cls._fields_:
        assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_iface_create", "dfm_iface_destroy", "dfm_iface_info", "dfm_pose_iface_energy", "dfm_pose_iface_energy_chunked", "dfm_iface_last_timing"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and (getattr(lib, s).argtypes or s == "dfm_iface_destroy")
    from test_abi_cpu import header_symbols
    assert sorted(_lib.EXPORTS) == header_symbols()
    assert lib.dfm_iface_create(None, 1, None, None, None, None, 1, None, None, None, None, None, 8.0, 0.6, 3.0, 4.0) is None
    assert b"m is NULL" in lib.dfm_last_error()
    assert lib.dfm_pose_iface_energy(None, 1, None, None, None) == -1 and b"h is NULL" in lib.dfm_last_error()
    assert lib.dfm_iface_last_timing(None, None) == -1 and lib.dfm_iface_info(None, None, None, None, None) == -1


def test_the_audits_see_the_new_kernels():
    """Both kernels of kernels_iface.hip are in the shipped code object (so the scratch / LDS / op_sel audits of test_abi_cpu.py run over
    them), use no scratch, and k_iface holds the two staged float4 arrays in LDS."""
    import re
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_iface.hip")).read()
    names = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))
    assert names == {"k_iface_pose", "k_iface"}
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
        assert found == {"k_iface_pose": (0, 0), "k_iface": (0, 2048)}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    d = tmp_path_factory.mktemp("iface_prep")
    exe = str(d / "iface_prep")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "iface_prep_main.cpp"), "-o", exe])

    def run(rec, rp, lig, lp, scalars=(8.0, 0.6, 3.0, 4.0), center=(0, 0, 0)):
        path = str(d / "in.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<ii", rec.shape[0], lig.shape[0]))
            f.write(np.float32(scalars).tobytes() + np.float32(center).tobytes())
            for xyz, par in ((rec, rp), (lig, lp)):
                f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
                for k in range(3):
                    f.write(np.ascontiguousarray(par[:, k], np.float32).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.stderr == "", r.stderr      # a sanitizer report
        return r.returncode, {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    return run


def test_parameter_checks_of_the_host_preparation(prep):
    rec, rp, lig, lp, _, _, _ = toy(1, 40, 30)

    def mod(par, i, k, v):
        q = par.copy()
        q[i, k] = v
        return q
    err = lambda *a, **k: " ".join(prep(*a, **k)[1].get("error", ["<none>"]))
    rc, out = prep(rec, rp, lig, lp)
    assert rc == 0 and out["bound"][3] == "1"
    # the parameters ride in the receptor's cell order
    order = np.array([int(v) for v in out["order"]])
    assert np.array_equal(np.sort(order), np.arange(40))
    want = np.concatenate([rp[order], np.zeros((40, 1), np.float32)], 1).reshape(-1)
    assert np.array_equal(np.array([float(v) for v in out["rec_par"]], np.float32), want)
    for i, k, v, name in ((5, 0, 0.0, "rec_rmin_half: atom 5 is not in (0, 8]"), (5, 0, 8.5, "rec_rmin_half: atom 5 is not in (0, 8]"),
                          (7, 0, np.nan, "rec_rmin_half: atom 7 is not in (0, 8]"), (6, 1, -0.1, "rec_sqrt_eps: atom 6 is not in [0, 2]"),
                          (6, 1, 2.5, "rec_sqrt_eps: atom 6 is not in [0, 2]"), (1, 2, 4.5, "rec_charge: atom 1 is not in [-4, 4]"),
                          (1, 2, -np.inf, "rec_charge: atom 1 is not in [-4, 4]")):
        assert err(rec, mod(rp, i, k, v), lig, lp) == name
        assert err(rec, rp, lig, mod(lp, i, k, v)) == name.replace("rec_", "lig_")
    for ok_par in (mod(rp, 0, 0, 8.0), mod(rp, 0, 1, 0.0), mod(rp, 0, 1, 2.0), mod(rp, 0, 2, -4.0), mod(rp, 0, 0, 1e-30)):
        assert prep(rec, ok_par, lig, lp)[0] == 0
    for sc, name in (((0.0, 0.6, 3.0, 4.0), "cutoff must be in (0, 16]"), ((16.5, 0.6, 3.0, 4.0), "cutoff must be in (0, 16]"),
                     ((np.nan, 0.6, 3.0, 4.0), "cutoff must be in (0, 16]"), ((8.0, 0.49, 3.0, 4.0), "soft must be in [0.5, 1]"),
                     ((8.0, 1.01, 3.0, 4.0), "soft must be in [0.5, 1]"), ((8.0, 0.6, 0.99, 4.0), "elec_min_dist must be finite and >= 1"),
                     ((8.0, 0.6, np.inf, 4.0), "elec_min_dist must be finite and >= 1"), ((8.0, 0.6, 3.0, 0.0), "dielectric_slope must be finite and > 0"),
                     ((8.0, 0.6, 3.0, -1.0), "dielectric_slope must be finite and > 0"), ((8.0, 0.6, 3.0, np.inf), "dielectric_slope must be finite and > 0")):
        assert err(rec, rp, lig, lp, sc) == name
    for sc in ((16.0, 0.5, 1.0, 4.0), (0.5, 1.0, 100.0, 1e-3)):
        assert prep(rec, rp, lig, lp, sc)[0] == 0
    bad = rec.copy()
    bad[3, 1] = np.nan
    assert err(bad, rp, lig, lp) == "rec_atoms: atom 3 is not finite"


def test_overflow_bound_of_the_host_preparation(prep):
    """pairs <= Al min(Ar, 27 max_cell_atoms); |sum| <= pairs (term (1 + 2^-30) 2^20 + 2) quanta must stay below 2^62."""
    f64 = lambda out: [float(v) for v in out["bound"][:3]]
    # the limits: sqrt_eps 2 x 2 at soft 0.5 -> rep + att <= 4 (4096 + 128) = 16896 kcal/mol; charges 4 x 4 at m = 1, slope 1 -> 5313.02
    lim = lambda n: np.tile(np.float32([[8.0, 2.0, 4.0]]), (n, 1))
    point = lambda n: np.tile(np.float32([[1.0, 2.0, 3.0]]), (n, 1))
    sc = (16.0, 0.5, 1.0, 1.0)
    rc, out = prep(point(50), lim(50), point(20), lim(20), sc)
    term, pairs, total = f64(out)
    assert rc == 0 and term == 16896.0 and pairs == 1000.0 and out["bound"][4] == "50"
    assert abs(total - 1000.0 * (16896.0 * 2.0 ** 20 + 2.0)) <= 1e-8 * total and total >= 1000.0 * (16896.0 * 2.0 ** 20 + 2.0)
    # one term of the definition at those limits is inside the bound
    from dfmdock_amd import ifenergy as IE
    rq, aq, eq = IE.pair_terms(np.zeros(1), lim(1), lim(1), 0.5, 1.0, 1.0)
    assert abs(int(rq[0]) + int(aq[0])) <= term * 2.0 ** 20 + 2 and abs(int(eq[0])) <= term * 2.0 ** 20 + 2 and int(rq[0]) == 1 << 34
    # a small slope makes Coulomb the larger term
    rc, out = prep(point(50), lim(50), point(20), lim(20), (16.0, 0.5, 1.0, 0.125))
    assert rc == 0 and f64(out)[0] == 332.0637 / 0.125 * 16.0
    # without charges and with soft = 1 the bound is 3 e
    unch = np.tile(np.float32([[2.0, 0.5, 0.0]]), (50, 1))
    rc, out = prep(point(50), unch, point(20), unch[:20], (8.0, 1.0, 3.0, 4.0))
    assert rc == 0 and f64(out)[0] == 0.75
    # 27 cells bound the pairs when the receptor is spread out: 512 atoms on an 8 x 8 x 8 lattice of 8 A cells, one per cell
    g = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(8.0) + np.float32(1.0)
    rc, out = prep(g, lim(512), point(20), lim(20), (8.0, 0.5, 1.0, 1.0))
    assert rc == 0 and out["bound"][4] == "1" and f64(out)[1] == 20.0 * 27.0
    # 2^14 x 2^14 coincident atoms at the limits: 2^28 pairs of 2^34.04 quanta reach 2^62 - rejected; half the ligand passes
    n = 1 << 14
    rc, out = prep(point(n), lim(n), point(n), lim(n), sc)
    assert rc == 4 and out["bound"][3] == "0" and f64(out)[1] == float(n) * n and f64(out)[2] >= 2.0 ** 62
    rc, out = prep(point(n), lim(n), point(n // 2), lim(n // 2), sc)
    assert rc == 0 and out["bound"][3] == "1" and 2.0 ** 61 < f64(out)[2] < 2.0 ** 62
    # a slope so small that one Coulomb term alone overflows: not finite, rejected
    rc, out = prep(point(2), lim(2), point(2), lim(2), (16.0, 0.5, 1.0, 1e-45))
    assert rc == 4 and out["bound"][3] == "0"


def test_driver_inputs_and_selection_helpers(tmp_path):
    from dfmdock_amd import cli, driver
    from dfmdock_amd import ifenergy as IE
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, _, _ = cli.load_pair(rec_pdb, lig_pdb, feat)
    ra, rp, la, lp, cen = driver.iface_inputs(rec, lig, 0)
    sa = driver.sterics_inputs(rec, lig, 0)
    assert np.array_equal(ra, sa[0]) and np.array_equal(la, sa[1]) and np.array_equal(cen, sa[2])
    assert rp.shape == (ra.shape[0], 3) and lp.shape == (la.shape[0], 3) and rp.dtype == np.float32 and rp[0, 2] == 1.0 and lp[0, 2] == 1.0
    IE.check_params(rp, ra.shape[0])
    assert driver._check_interface(False, "energy", None, 8.0) is None
    assert driver._check_interface(True, "energy", None, 8.0) == (False, IE.WEIGHTS, 8.0)
    assert driver._check_interface(False, "interface", (1, 2, 3), 6.5) == (True, (1.0, 2.0, 3.0), 6.5)
    for bad in (dict(ie_weights=(1, 2)), dict(ie_cutoff=20.0), dict(ie_weights=(1, np.nan, 1))):
        with pytest.raises(ValueError):
            driver._check_interface(True, "energy", **dict(dict(ie_weights=None, ie_cutoff=8.0), **bad))
    driver._check_rank("interface", 1.0)
    with pytest.raises(ValueError):
        driver._check_rank("physics", 1.0)
    ed = {"rep": np.array([1.0, 2.0]), "att": np.array([-3.0, -1.0]), "elec": np.array([0.5, 0.0]), "total": np.array([-2.5, -0.5]), "n_pairs": np.array([40, 9])}
    assert driver._pose_interface(ed, 1) == {"rep": 2.0, "att": -1.0, "elec": 0.0, "total": -0.5, "n_pairs": 9}
    json.dumps(driver._pose_interface(ed, 0))
    off = driver._Run(None, type("G", (), {"lig_pos0": None}), None, None, None, "fp32", {"interface": None})      # off: no stage of _finish runs it
    off.k = 3
    [a.run(off) for a in driver.ANALYSES if a.name in off.opts]
    assert (off.k, off.key, off.data) == (3, None, {}) and not off.any() and driver._interface_result(None, 3, None) == {}


def test_every_summary_describes_the_kept_pose(tmp_path, monkeypatch):
    """_finish with the engine stubbed: whichever rank moves the kept pose, the `consensus` and `interface_energy` objects, `index` and
    the returned transform all belong to that one pose."""
    from dfmdock_amd import cli, driver
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, _, _ = cli.load_pair(rec_pdb, lig_pdb, feat)
    n = 5
    energy = np.float32([-5.0, -1.0, -2.0, -3.0, -4.0])      # energy keeps 0
    cons_score = np.array([0.1, 0.2, 0.9, 0.3, 0.4])         # consensus keeps 2
    total = np.array([3.0, 2.0, 1.0, -7.0, 0.5])             # interface keeps 3
    cols = {"energy": energy, "rot_update": 0.01 * np.arange(3 * n, dtype=np.float32).reshape(n, 3),
            "tr_update": np.arange(3 * n, dtype=np.float32).reshape(n, 3)}
    cd = lambda: {"consensus": cons_score.copy(), "n_contacts": np.arange(10, 10 + n), "M": n, "cutoff": 5.5}
    ed = {"rep": np.arange(n) + 0.5, "att": -np.arange(n) - 0.25, "elec": np.zeros(n), "total": total, "n_pairs": np.arange(100, 100 + n)}
    monkeypatch.setattr(driver, "ensemble_consensus", lambda *a, **k: cd())
    monkeypatch.setattr(driver, "ensemble_interface_energy", lambda *a, **k: dict(ed))

    class Gx:
        lig_pos0 = np.asarray(lig["bb_coords"], np.float32)

        def close(self):
            pass

    class Hp:
        family = 0
    model = type("M", (), {"hp": Hp})()

    def finish(rank, consensus, interface, bad=None):
        cons = (rank, 5.5, 1.0) if consensus or rank == "consensus" else None
        ie = driver._check_interface(interface, rank, None, 8.0)
        if bad is not None:
            monkeypatch.setattr(driver, "_screen", lambda *a: ({"flags": bad, "n_clash": np.zeros(n, int), "n_contact": np.ones(n, int), "min_dist": np.ones(n),
                                                              "threshold": 1.0, "ensemble_mean": 0.0, "ensemble_std": 0.0, "clash_cutoff": 3.0,
                                                              "contact_cutoff": 5.0, "filtered": True, "fallback": False}, bad))
        run = driver._Run(model, Gx(), rec, lig, cols, "fp32", dict(consensus=cons, sterics=(True, 3.0, 5.0) if bad is not None else None, interface=ie))
        run.key = energy
        return driver._finish(run, (np.argmin, "energy"), lambda k: {})
    for rank, want, by in (("energy", 0, "energy"), ("consensus", 2, "consensus"), ("interface", 3, "interface")):
        r = finish(rank, True, True)
        assert r["index"] == want and np.array_equal(r["rot_update"], cols["rot_update"][want]) and r["energy"] == float(energy[want])
        assert r["consensus"]["score"] == cons_score[want] == r["consensus_data"]["consensus"][r["index"]]
        assert r["consensus"]["n_contacts"] == 10 + want and r["consensus"]["ranked_by"] == by and r["consensus"]["fallback"] is False
        assert r["interface_energy"]["total"] == total[want] == r["interface_data"]["total"][r["index"]] and r["interface_energy"]["n_pairs"] == 100 + want
        assert r["interface_energy"]["ranked_by"] == by
        assert r["consensus"]["rank"] == 1 + int((cons_score > cons_score[want]).sum()) and r["interface_energy"]["rank"] == 1 + int((total < total[want]).sum())
    # one option without the other
    r = finish("interface", False, False)
    assert r["index"] == 3 and "consensus" not in r and r["interface_energy"]["ranked_by"] == "interface"
    r = finish("consensus", False, False)
    assert r["index"] == 2 and "interface_energy" not in r
    # the clash filter removes the interface pick: the next lowest total is kept, and ranks count the poses that are left
    bad = np.array([False, False, False, True, False])
    r = finish("interface", True, True, bad)
    assert r["index"] == 4 and r["interface_energy"]["total"] == 0.5 and r["interface_energy"]["rank"] == 1 and r["consensus"]["score"] == 0.4


def test_cli_flags_parse_default_off_and_reach_the_driver(tmp_path, monkeypatch, capsys):
    from dfmdock_amd import cli, driver, pdbio
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert not a.interface_energy and a.rank == "energy" and a.energy_residues is None and cli.interface_kwargs(a) == {}
        a = cli.parse_args([cmd] + base + ["--interface-energy"])
        assert cli.interface_kwargs(a) == dict(interface_energy=True, ie_weights=None, ie_cutoff=8.0, rank="energy")
        a = cli.parse_args([cmd] + base + ["--rank", "interface", "--ie-weights", "1", "0.5", "0.25", "--ie-cutoff", "6"])
        assert cli.interface_kwargs(a) == dict(interface_energy=True, ie_weights=[1.0, 0.5, 0.25], ie_cutoff=6.0, rank="interface") and not a.consensus
        assert cli.parse_args([cmd] + base + ["--energy-residues", "x.txt"]).interface_energy
        for bad in (["--ie-cutoff", "6"], ["--ie-weights", "1", "1", "1"], ["--interface-energy", "--ie-cutoff", "17"], ["--interface-energy", "--ie-cutoff", "nan"],
                    ["--interface-energy", "--ie-weights", "1", "nan", "1"], ["--rank", "physics"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c", "--interface-energy"])      # sweep is left alone: the DB5 files hold backbones only
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))
    ie = {"rep": 12.5, "att": -30.25, "elec": -1.5, "total": -28.75, "n_pairs": 812, "rank": 1, "weights": [0.18, 1.0, 0.5], "cutoff": 8.0,
          "ranked_by": "interface"}

    def dock_pair(model, rec, lig, rec_x, lig_x, **kw):
        seen.update(kw)
        res = {"energy": -1.5, "precision": "mfma16", "rot_update": np.zeros(3, np.float32), "tr_update": np.ones(3, np.float32), "selfcheck": None}
        if kw.get("interface_energy"):
            res.update(interface_energy=ie, index=4)
        return res

    def residue_interface_energy(model, rec, lig, rot, tr, cutoff):
        seen["residue_call"] = (np.asarray(rot).tolist(), np.asarray(tr).tolist(), cutoff)
        keys = [tuple(k) for k in lig["residues"]]
        v = np.zeros(len(keys), np.int64)
        v[2] = -(5 << 18)
        return keys, v, -v * 2
    monkeypatch.setattr(driver, "dock_pair", dock_pair)
    monkeypatch.setattr(driver, "residue_interface_energy", residue_interface_energy)
    args = ["dock", rec_pdb, lig_pdb, "--ckpt", "c.ckpt", "--features", feat, "--out", str(tmp_path / "o.pdb")]
    assert cli.main(args) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "interface_energy" not in plain and "index" not in plain and not any(k.startswith(("ie_", "interface", "rank")) for k in seen)
    seen.clear()
    assert cli.main(args + ["--rank", "interface", "--energy-residues", str(tmp_path / "res.txt")]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["interface_energy"] is True and seen["rank"] == "interface" and seen["ie_weights"] is None and seen["ie_cutoff"] == 8.0
    assert "consensus" not in seen and line["interface_energy"] == ie and line["index"] == 4 and {k: v for k, v in line.items() if k in plain} == plain
    assert seen["residue_call"] == ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 8.0) and os.path.samefile(line["energy_residues"], tmp_path / "res.txt")
    k = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))["residues"][2]
    assert (tmp_path / "res.txt").read_text().splitlines()[1:] == [f"{k[0]}:{k[1]} {k[3]} -1.250000 2.500000"]
