"""The float64 definition of Cn symmetric docking (dfmdock_amd/symmetry.py), the copies of an n-mer, the refusals of the pair drivers
and the command line's options - no GPU.

Closure gate: after the full projection T'^n = identity within 1e-9 A and theta' = theta* within 1e-9 rad (measured over 2000 random
monomers, n = 2 .. 8: 2.2e-12 A)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _chain(M, rng):
    return 8.0 * rng.standard_normal((M, 3, 3)) + 20.0 * rng.standard_normal(3)


def _turn(y, theta, u, point, screw=0.0):
    from dfmdock_amd.restraints import axis_angle_to_matrix
    u = np.asarray(u, np.float64) / np.linalg.norm(u)
    return (np.asarray(y, np.float64) - point) @ axis_angle_to_matrix(theta * u).T + point + screw * u


@pytest.mark.parametrize("M", [9, 24, 87])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_projection_closes(n, M):
    from dfmdock_amd import symmetry as SY
    rng = np.random.default_rng(1000 * n + M)
    thetas = list(rng.uniform(0.05, np.pi - 0.05, 12)) + ([np.pi, np.pi] if n == 2 else [])
    for center in ("ca", "all_atoms"):
        for theta in thetas:
            y = _chain(M, rng)
            x = _turn(y, theta, rng.standard_normal(3), y.reshape(-1, 3).mean(0) + 12.0 * rng.standard_normal(3), 4.0 * rng.standard_normal())
            ev = SY.evaluate(y, x, n, center=center, last=True)
            assert abs(ev["theta"] - theta) <= 1e-9 and ev["fit_rmsd"] <= 1e-9 and ev["m"] >= 1
            x2, _, _ = SY.apply_step(x, ev, center=center)
            np.testing.assert_allclose(x2, ev["projected"], atol=1e-12)
            e2 = SY.evaluate(y, x2, n, center=center)
            assert SY.closure(y, e2["Q"], e2["tau"], n) <= 1e-9
            assert abs(e2["theta"] - ev["theta_star"]) <= 1e-9 and abs(e2["screw"]) <= 1e-9 and e2["m"] == ev["m"]
            assert np.abs(e2["Q"] @ e2["axis_point"] + e2["tau"] - e2["axis_point"]).max() <= 1e-9      # a point of the axis
            assert abs(ev["sym_rmsd"] - np.sqrt(np.mean(np.sum((x2 - x) ** 2, -1)))) <= 1e-12


def test_symmetric_pose_has_a_zero_step():
    from dfmdock_amd import symmetry as SY
    rng = np.random.default_rng(5)
    for n in range(2, 9):
        for m in (k for k in range(1, n // 2 + 1) if np.gcd(k, n) == 1):
            y = _chain(24, rng)
            x = _turn(y, 2 * np.pi * m / n, rng.standard_normal(3), y.reshape(-1, 3).mean(0) + 15.0 * rng.standard_normal(3))
            for last in (False, True):
                ev = SY.evaluate(y, x, n, last=last)
                assert ev["m"] == m and np.abs(ev["step"]).max() <= 1e-9 and ev["sym_rmsd"] <= 1e-9
                assert SY.closure(y, ev["Q"], ev["tau"], n) <= 1e-9


def test_step_gains_clip_and_snap():
    from dfmdock_amd import symmetry as SY
    rng = np.random.default_rng(6)
    y = _chain(24, rng)
    u = np.array([0.0, 0.6, 0.8])
    x = _turn(y, 2 * np.pi / 3 - 0.9, u, y.reshape(-1, 3).mean(0) + [14.0, 0, 0], 25.0)
    p = SY.SymmetryParams()
    ev = SY.evaluate(y, x, 3, p)
    np.testing.assert_allclose(ev["axis"], u, atol=1e-12)
    assert ev["screw"] == pytest.approx(25.0, abs=1e-9)
    np.testing.assert_allclose(ev["step"][:3], -10.0 * u, atol=1e-9)       # 12.5 A clipped to max_tr
    np.testing.assert_allclose(ev["step"][3:], 0.3 * u, atol=1e-9)         # 0.45 rad clipped to max_rot
    free = SY.evaluate(y, x, 3, SY.SymmetryParams(gain_rot=0.25, gain_tr=0.1, max_rot=1.0, max_tr=100.0))
    np.testing.assert_allclose(free["step"], np.concatenate([-2.5 * u, 0.225 * u]), atol=1e-9)
    snap = SY.evaluate(y, x, 3, p, last=True)
    np.testing.assert_allclose(snap["step"], np.concatenate([-25.0 * u, 0.9 * u]), atol=1e-9)
    np.testing.assert_array_equal(SY.evaluate(y, x, 3, SY.SymmetryParams(snap_last=0), last=True)["step"], ev["step"])
    # no axis: a zero step, m = 0, theta = 0; a non-finite pose: NaN
    none = SY.evaluate(y, y + [3.0, 0, 0], 3)
    assert none["m"] == 0 and none["theta"] == 0.0 and not none["step"].any() and np.isnan(none["screw"]) and np.isnan(none["axis"]).all()
    bad = x.copy()
    bad[3, 1, 0] = np.inf
    nan = SY.evaluate(y, bad, 3)
    assert nan["m"] == 0 and np.isnan(nan["step"]).all() and np.isnan(nan["theta"]) and np.isnan(nan["fit_rmsd"])
    for kw in (dict(gain_rot=0.0), dict(gain_tr=1.01), dict(max_rot=0.0), dict(max_tr=float("inf")), dict(t_start=float("nan"))):
        with pytest.raises(ValueError):
            SY.SymmetryParams(**kw)
    with pytest.raises(ValueError):
        SY.evaluate(y, x[:-1], 3)


def test_m_selection():
    from dfmdock_amd import symmetry as SY
    assert SY.select_m(0.1, 2) == (1, np.pi) and SY.select_m(3.0, 2)[0] == 1
    assert SY.select_m(3.1, 3)[0] == 1                                   # n = 3: m = 1 only
    assert [SY.select_m(t, 5)[0] for t in (0.2, 1.8, 1.9, 3.1)] == [1, 1, 2, 2]
    assert [SY.select_m(t, 6)[0] for t in (0.2, 3.0)] == [1, 1]          # 2 and 3 are no generators of C6
    assert [SY.select_m(t, 8)[0] for t in (0.3, 1.5, 1.6, 3.0)] == [1, 1, 3, 3]
    assert SY.select_m(np.pi / 2, 8) == (1, 2.0 * np.pi * 1 / 8)         # an exact tie between pi / 4 and 3 pi / 4: the smaller m
    assert abs(np.pi / 2 - 2.0 * np.pi * 1 / 8) == abs(np.pi / 2 - 2.0 * np.pi * 3 / 8)
    assert [SY.select_m(t, 12)[0] for t in (0.1, 2.0, 3.0)] == [1, 5, 5] and SY.select_m(1.0, 24)[0] == 5
    for n in (0, 1, 25, 2.5, "3"):
        with pytest.raises(ValueError):
            SY.check_order(n)


def test_parse_symmetry():
    from dfmdock_amd import symmetry as SY
    assert [SY.parse_symmetry(s) for s in ("C3", "3", "c2", " C24 ", 5)] == [3, 3, 2, 24, 5]
    for s in ("C1", "D3", "C25", "", "C", "3.5", "-3"):
        with pytest.raises(ValueError):
            SY.parse_symmetry(s)


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_copy_poses(n):
    from dfmdock_amd import pdbio, symmetry as SY
    from dfmdock_amd.fit import fit_poses
    from dfmdock_amd.restraints import axis_angle_to_matrix
    rng = np.random.default_rng(n)
    y = _chain(24, rng)
    x0 = (y - y.reshape(-1, 3).mean(0)) @ axis_angle_to_matrix(rng.standard_normal(3)).T + 30.0 * rng.standard_normal(3)      # the ligand as given
    m = 2 if n == 5 else (3 if n == 8 else 1)
    x = _turn(y, 2 * np.pi * m / n, rng.standard_normal(3), y.reshape(-1, 3).mean(0) + 15.0 * rng.standard_normal(3))
    c = x0[:, 1].mean(0)
    rot, tr, rmsd, _ = fit_poses(x0, x[None], c)
    assert rmsd[0] <= 1e-9
    rots, trs = SY.copy_poses(y, x0, rot[0], tr[0], c, n)
    assert rots.shape == trs.shape == (n - 1, 3)
    np.testing.assert_array_equal(rots[0], rot[0]); np.testing.assert_array_equal(trs[0], tr[0])
    asm = SY.assemble(y, x0, rot[0], tr[0], c, n)
    assert asm.shape == (n,) + y.shape
    assert np.abs(asm[1] - x).max() <= 1e-9                               # copy 1 reproduces the pose
    Q, tau, _ = SY.fit_transform(y, x)
    for k in range(1, n):                                                 # copy k is T^k of the receptor
        Qk, tk = SY.transform_power(Q, tau, k)
        assert np.abs(asm[k] - (y @ Qk.T + tk)).max() <= 1e-9
    assert np.abs(asm[n - 1] @ Q.T + tau - y).max() <= 1e-9               # copy n reproduces the receptor
    # every pose places its copy through the drivers' all-atom call too
    for k in range(n - 1):
        aa = pdbio.apply_pose_all_atom(x0.reshape(-1, 3), x0, rots[k], trs[k], center="ca")
        assert np.abs(aa.reshape(-1, 3, 3) - asm[k + 1]).max() <= 1e-9


def test_ctypes_symmetry_structs_have_the_c_layout(tmp_path):
    from dfmdock_amd import _lib
    names = {"dfm_symmetry_params": _lib.SymmetryParamsC, "dfm_symmetry_out": _lib.SymmetryOutC}
    probes = {"dfm_symmetry_params": ["gain_tr", "t_start", "snap_last"], "dfm_symmetry_out": ["axis_point", "order_m", "step"]}
    body = "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
    body += "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, fs in probes.items() for f in fs)
    body += 'printf("flag %u\\n", (unsigned)DFM_F_SYMMETRY);'
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    for n, cls in names.items():
        assert int(got[n]) == C.sizeof(cls), n
        for f in probes[n]:
            assert int(got[f"{n}.{f}"]) == getattr(cls, f).offset, (n, f)
    assert int(got["flag"]) == _lib.DFM_F_SYMMETRY == 1 << 15
    assert {"dfm_complex_set_symmetry", "dfm_symmetry_eval"} <= set(_lib.EXPORTS)


def _pdb_pair(tmp_path):
    from symmetry_fixtures import write_homodimer
    from dfmdock_amd import pdbio
    a, a2, feat, other = write_homodimer(str(tmp_path))
    load = lambda p: pdbio.backbone_from_atoms(pdbio.read_pdb(p))
    return load(a), load(a2), load(other)


def test_driver_refusals(tmp_path):
    """Every refusal comes before the engine is touched: model = None never gets used."""
    from dfmdock_amd import driver
    rec, lig, other = _pdb_pair(tmp_path)
    ok = driver._check_symmetry(rec, lig, 3, None, 0.1)
    assert ok["n"] == 3 and ok["input_rmsd"] <= 1e-9
    assert driver._check_symmetry(rec, lig, None, None, 0.1) is None
    for fn in (driver.dock_pair, driver.refine_pair):
        with pytest.raises(ValueError, match="sequences differ"):
            fn(None, rec, other, None, None, symmetry=3)
        two = dict(rec, residues=[("A",) + tuple(k[1:]) if i < 12 else ("C",) + tuple(k[1:]) for i, k in enumerate(rec["residues"])])
        with pytest.raises(ValueError, match="more than one chain id"):
            fn(None, two, lig, None, None, symmetry=3)
        with pytest.raises(ValueError, match="more than one chain id"):
            fn(None, rec, dict(two, bb_coords=lig["bb_coords"]), None, None, symmetry=3)
        bent = dict(lig, bb_coords=lig["bb_coords"] + np.where(np.arange(24)[:, None, None] < 12, 0.0, 0.5))
        with pytest.raises(ValueError, match="rigid images"):
            fn(None, rec, bent, None, None, symmetry=3)
        with pytest.raises(ValueError, match="symmetry_tolerance"):
            fn(None, rec, lig, None, None, symmetry=3, symmetry_tolerance=-1.0)
        with pytest.raises(ValueError, match="order"):
            fn(None, rec, lig, None, None, symmetry=1)
        with pytest.raises(ValueError, match="needs symmetry"):
            from dfmdock_amd.symmetry import SymmetryParams
            fn(None, rec, lig, None, None, symmetry_params=SymmetryParams())
    assert driver._check_symmetry(rec, bent, 3, None, 1.0)["input_rmsd"] > 0.1


def test_cli_parsing():
    from dfmdock_amd import cli
    base = ["A.pdb", "A2.pdb", "--ckpt", "m.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base + ["--symmetry", "C3", "--symmetry-gain", "0.25", "--symmetry-t-start", "0.6",
                                           "--symmetry-tolerance", "0.3", "--no-symmetry-snap", "--seed", "7"])
        assert a.cmd == cmd and a.pdb_2 == "A2.pdb" and a.seed == 7      # the command's own parser read the rest
        kw = cli.symmetry_kwargs(a)
        p = kw["symmetry_params"]
        assert kw["symmetry"] == 3 and kw["symmetry_tolerance"] == 0.3
        assert (p.gain_rot, p.gain_tr, p.t_start, p.snap_last, p.max_rot, p.max_tr) == (0.25, 0.25, 0.6, 0, 0.3, 10.0)
        d = cli.symmetry_kwargs(cli.parse_args([cmd, "--symmetry", "4"] + base))      # anywhere behind the command
        assert d["symmetry"] == 4 and d["symmetry_params"].snap_last == 1 and d["symmetry_params"].gain_rot == 0.5 and "symmetry_tolerance" not in d
        assert cli.symmetry_kwargs(cli.parse_args([cmd] + base)) == {}
        for bad in (["--symmetry", "D2"], ["--symmetry", "C1"], ["--symmetry", "C3", "--symmetry-gain", "0"],
                    ["--symmetry", "C3", "--symmetry-gain", "1.5"], ["--symmetry", "C3", "--symmetry-tolerance", "-1"],
                    ["--symmetry-gain", "0.5"], ["--no-symmetry-snap"], ["--symmetry"], ["--symm", "C3"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
        sub = [x for x in cli.build_parser()._actions if x.dest == "cmd"][0].choices[cmd]
        assert all(o in sub.format_help() for o in ("--symmetry Cn", "--symmetry-gain", "--symmetry-t-start", "--symmetry-tolerance",
                                                    "--no-symmetry-snap"))
    for argv in (["sweep", "--db5", "d", "--ckpt", "c", "--symmetry", "C3"], ["selfcheck"] + base + ["--symmetry", "C3"]):      # out of scope there
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
