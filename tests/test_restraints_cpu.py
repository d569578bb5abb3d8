"""Interface restraints on the host: the restraint-file parser, the float64 numpy definition (dfmdock_amd/restraints.py) - gradient and
torque against finite differences, clipping, the tie rule, the step and its bookkeeping - and the C ABI additions (struct layout,
exported symbols)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, complex_for


def _groups(R, L, rng, G=12):
    from dfmdock_amd.restraints import RestraintGroup
    return [RestraintGroup(tuple((int(rng.integers(R)), int(rng.integers(L))) for _ in range(1 + g % 4)),
                           float(rng.uniform(3.0, 9.0)), float(rng.uniform(0.5, 2.0))) for g in range(G)]


def _pose(rng, R=30, L=20):
    rec = rng.normal(size=(R, 3, 3)) * 8.0
    lig = rng.normal(size=(L, 3, 3)) * 6.0 + np.array([14.0, 3.0, -2.0])
    return rec, lig


def _moved(lig, v, center="ca"):
    """The ligand moved rigidly by v = (translation, rotation vector) about the centroid."""
    from dfmdock_amd.restraints import apply_step
    return apply_step(lig, v, center=center)[0]


@pytest.mark.parametrize("center", ["ca", "all_atoms"])
def test_force_and_torque_are_minus_the_gradient_of_U(center):
    """F = -dU/d(translation), T = -dU/d(rotation vector about c), by central differences of U in float64."""
    from dfmdock_amd import restraints as RS
    rng = np.random.default_rng(1)
    rec, lig = _pose(rng)
    groups = _groups(30, 20, rng)
    e = RS.evaluate(groups, rec, lig, center=center)
    assert e["energy"] > 0 and e["n_satisfied"] < len(groups)
    h = 1e-6
    num = np.zeros(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        num[k] = -(RS.energy(groups, rec, _moved(lig, d, center)) - RS.energy(groups, rec, _moved(lig, -d, center))) / (2 * h)
    np.testing.assert_allclose(e["force"], num[:3], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(e["torque"], num[3:], rtol=1e-6, atol=1e-5)


def test_step_is_clipped():
    from dfmdock_amd import restraints as RS
    rng = np.random.default_rng(2)
    rec, lig = _pose(rng)
    groups = _groups(30, 20, rng)
    big = RS.evaluate(groups, rec, lig, RS.RestraintParams(k_tr=10.0, k_rot=1.0, max_tr=2.0, max_rot=0.1))
    assert np.linalg.norm(big["step"][:3]) == pytest.approx(2.0) and np.linalg.norm(big["step"][3:]) == pytest.approx(0.1)
    np.testing.assert_allclose(big["step"][:3] / 2.0, big["force"] / np.linalg.norm(big["force"]))      # direction kept
    small = RS.evaluate(groups, rec, lig, RS.RestraintParams(k_tr=1e-6, k_rot=1e-8))
    np.testing.assert_allclose(small["step"], np.concatenate([1e-6 * small["force"], 1e-8 * small["torque"]]))


def test_satisfied_zero_weight_and_tie_rule():
    from dfmdock_amd import restraints as RS
    from dfmdock_amd.restraints import RestraintGroup
    rec = np.zeros((3, 3, 3))
    rec[:, 1] = [[0, 0, 0], [10, 0, 0], [0, 0, 30]]
    lig = np.zeros((3, 3, 3))
    lig[:, 1] = [[5, 0, 0], [0, 5, 0], [0, 0, 20]]
    # ligand 0 is 5 A from receptors 0 and 1 (an exact tie): the first listed pair is the arg-min
    e1 = RS.evaluate([RestraintGroup(((1, 0), (0, 0)), 4.0)], rec, lig)
    e2 = RS.evaluate([RestraintGroup(((0, 0), (1, 0)), 4.0)], rec, lig)
    assert e1["arg"][0] == 0 and e2["arg"][0] == 0
    assert e1["energy"] == e2["energy"] == pytest.approx(1.0)
    np.testing.assert_allclose(e1["force"], [2.0, 0, 0])          # pulled towards receptor 1 (x = 10)
    np.testing.assert_allclose(e2["force"], [-2.0, 0, 0])         # ... towards receptor 0
    # satisfied groups and zero weights contribute nothing; both still count by v_g alone
    e = RS.evaluate([RestraintGroup(((0, 1),), 6.0), RestraintGroup(((2, 2),), 4.0, 0.0), RestraintGroup(((2, 2),), 11.0, 0.0)], rec, lig)
    assert e["n_satisfied"] == 2 and e["energy"] == 0.0 and not e["force"].any() and not e["torque"].any()


@pytest.mark.parametrize("center", ["ca", "all_atoms"])
def test_step_bookkeeping_replays_the_pose(center):
    """Steps applied one after the other, with rot_update / tr_update composed as the sampler does, equal the start pose moved once by
    the accumulated (rot_update, tr_update) about the start pose's centroid."""
    from dfmdock_amd import restraints as RS
    rng = np.random.default_rng(3)
    rec, lig0 = _pose(rng)
    groups = _groups(30, 20, rng)
    ru, tu = np.zeros(3), np.zeros(3)
    pose = lig0.copy()
    for _ in range(12):
        st = RS.evaluate(groups, rec, pose, RS.RestraintParams(k_tr=0.05, k_rot=5e-3, max_rot=0.4), center=center)["step"]
        pose, ru, tu = RS.apply_step(pose, st, ru, tu, center=center)
    assert np.abs(pose - lig0).max() > 1.0
    np.testing.assert_allclose(RS.replay_pose(lig0, ru, tu, center=center), pose, atol=1e-9)
    assert RS.evaluate(groups, rec, pose)["energy"] < RS.evaluate(groups, rec, lig0)["energy"]


def test_rot_compose_and_matrix_round_trip():
    from dfmdock_amd import restraints as RS
    rng = np.random.default_rng(4)
    for _ in range(50):
        a = rng.normal(size=3) * rng.uniform(0, 1.0)
        b = rng.normal(size=3) * rng.uniform(0, 1.0)
        np.testing.assert_allclose(RS.axis_angle_to_matrix(RS.matrix_to_axis_angle(RS.axis_angle_to_matrix(a))), RS.axis_angle_to_matrix(a),
                                   atol=1e-12)
        np.testing.assert_allclose(RS.axis_angle_to_matrix(RS.rot_compose(a, b)), RS.axis_angle_to_matrix(b) @ RS.axis_angle_to_matrix(a),
                                   atol=1e-12)


def test_pack_and_its_checks():
    from dfmdock_amd.restraints import RestraintGroup, pack
    gs, pairs, up, w = pack([RestraintGroup(((0, 1),), 8.0), RestraintGroup(((2, 3), (4, 5)), 6.0, 0.5)], R=5, L=6)
    assert gs.tolist() == [0, 1, 3] and pairs.tolist() == [[0, 1], [2, 3], [4, 5]] and up.tolist() == [8.0, 6.0] and w.tolist() == [1.0, 0.5]
    assert gs.dtype == np.int32 and pairs.dtype == np.int32 and up.dtype == np.float32
    for bad in ([RestraintGroup(((5, 0),), 8.0)], [RestraintGroup(((0, 6),), 8.0)], [RestraintGroup(((0, 0),), 0.0)],
                [RestraintGroup(((0, 0),), 1.0, -0.1)], [RestraintGroup((), 1.0)]):
        with pytest.raises(ValueError):
            pack(bad, R=5, L=6)
    assert pack([])[0].tolist() == [0]


_REC = """\
ATOM      1  N   ALA A  10       0.000   0.000   0.000  1.00  0.00           N
ATOM      2  CA  ALA A  10       1.000   0.000   0.000  1.00  0.00           C
ATOM      3  C   ALA A  10       2.000   0.000   0.000  1.00  0.00           C
ATOM      4  N   GLY A  11       3.000   0.000   0.000  1.00  0.00           N
ATOM      5  CA  GLY A  11       4.000   0.000   0.000  1.00  0.00           C
ATOM      6  C   GLY A  11       5.000   0.000   0.000  1.00  0.00           C
ATOM      7  N   SER A  11A      6.000   0.000   0.000  1.00  0.00           N
ATOM      8  CA  SER A  11A      7.000   0.000   0.000  1.00  0.00           C
ATOM      9  C   SER A  11A      8.000   0.000   0.000  1.00  0.00           C
ATOM     10  N   LEU A  12       9.000   0.000   0.000  1.00  0.00           N
ATOM     11  CA  LEU A  12      10.000   0.000   0.000  1.00  0.00           C
ATOM     12  N   VAL A  13      12.000   0.000   0.000  1.00  0.00           N
ATOM     13  CA  VAL A  13      13.000   0.000   0.000  1.00  0.00           C
ATOM     14  C   VAL A  13      14.000   0.000   0.000  1.00  0.00           C
ATOM     15  N   THR C   1      15.000   0.000   0.000  1.00  0.00           N
ATOM     16  CA  THR C   1      16.000   0.000   0.000  1.00  0.00           C
ATOM     17  C   THR C   1      17.000   0.000   0.000  1.00  0.00           C
"""


def _lig_pdb(n=8, chain="B", start=100):
    lines = []
    k = 1
    for r in range(n):
        for a, nm in enumerate(("N", "CA", "C")):
            lines.append("ATOM  %5d  %-3s ALA %s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C" % (k, nm, chain, start + r, 20.0 + r, a, 0.0))
            k += 1
    return "\n".join(lines) + "\n"


@pytest.fixture()
def chains(tmp_path):
    from dfmdock_amd import pdbio
    (tmp_path / "rec.pdb").write_text(_REC)
    (tmp_path / "lig.pdb").write_text(_lig_pdb())
    return pdbio.backbone_from_atoms(pdbio.read_pdb(str(tmp_path / "rec.pdb"))), pdbio.backbone_from_atoms(pdbio.read_pdb(str(tmp_path / "lig.pdb")))


def test_backbone_keeps_the_residue_order(chains):
    rec, lig = chains
    # LEU A 12 has no C: dropped; the insertion code is part of the key
    assert [(k[0], k[1], k[2]) for k in rec["residues"]] == [("A", 10, " "), ("A", 11, " "), ("A", 11, "A"), ("A", 13, " "), ("C", 1, " ")]
    assert len(rec["residues"]) == len(rec["seq"]) == rec["bb_coords"].shape[0]
    assert len(lig["residues"]) == 8 and lig["residues"][0][:2] == ("B", 100)


def test_parser_chains_icodes_ranges_comments_weights(chains):
    from dfmdock_amd.restraints import parse_restraints
    rec, lig = chains
    text = """# header comment

A:10  B:100  8.0
A:11A,C:1   B:101-B:103   6.5  0.25   # ambiguous: 2 x 3 pairs
A:11-A:13   B:107         12          # range across an insertion code and a dropped residue
"""
    g = parse_restraints(text, rec, lig)
    assert len(g) == 3
    assert g[0].pairs == ((0, 0),) and g[0].upper == 8.0 and g[0].weight == 1.0
    assert g[1].pairs == ((2, 1), (2, 2), (2, 3), (4, 1), (4, 2), (4, 3)) and g[1].upper == 6.5 and g[1].weight == 0.25
    assert g[2].pairs == ((1, 7), (2, 7), (3, 7)) and g[2].upper == 12.0


@pytest.mark.parametrize("line,needle", [
    ("A:99  B:100  8", "A:99 is not in the structure"),
    ("A:12  B:100  8", "A:12 has no complete backbone"),
    ("A:10  B:100X  8", "B:100X is not in the structure"),
    ("A:10  Z:1  8", "Z:1 is not in the structure"),
    ("A:10  B:100  0", "upper bound must be > 0"),
    ("A:10  B:100  8  -1", "weight must be >= 0"),
    ("A:10  B:100", "expected REC_RESIDUES"),
    ("A10  B:100  8", "cannot read receptor residue 'A10'"),
    ("A:13-A:10  B:100  8", "must run forward"),
    ("A:10-C:1  B:100  8", "must run forward within one chain"),
])
def test_parser_errors_name_the_residue(chains, line, needle):
    from dfmdock_amd.restraints import parse_restraints
    rec, lig = chains
    with pytest.raises(ValueError) as ei:
        parse_restraints("# ok\n" + line + "\n", rec, lig)
    assert needle in str(ei.value) and "line 2" in str(ei.value)


def test_parser_on_the_cli_fixture_pdbs(tmp_path):
    """Residue names of the PDB files tests/cli_fixtures.py writes map back to the indices of the complex."""
    from cli_fixtures import golden_7cei, write_pair
    from dfmdock_amd import pdbio
    from dfmdock_amd.restraints import native_contact_groups, parse_restraints
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, _ = write_pair(str(tmp_path), cx, rs, ls)
    rec = pdbio.backbone_from_atoms(pdbio.read_pdb(rec_pdb))
    lig = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))
    assert len(rec["residues"]) == len(rs) and len(lig["residues"]) == len(ls)
    want = native_contact_groups(cx["rec_pos"], cx["lig_pos"], 6, seed=4)
    assert len(want) == 6 and all(g.upper == 8.0 and len(g.pairs) == 1 for g in want)
    name = lambda k: f"{k[0]}:{k[1]}{k[2].strip()}"
    text = "".join(f"{name(rec['residues'][g.pairs[0][0]])} {name(lig['residues'][g.pairs[0][1]])} 8.0\n" for g in want)
    assert parse_restraints(text, rec, lig) == want
    # the contacts are contacts of the native pose, and the draw is seeded
    y, x = cx["rec_pos"][:, 1].astype(np.float64), cx["lig_pos"][:, 1].astype(np.float64)
    assert all(np.linalg.norm(x[g.pairs[0][1]] - y[g.pairs[0][0]]) < 8.0 for g in want)
    assert native_contact_groups(cx["rec_pos"], cx["lig_pos"], 6, seed=4) == want != native_contact_groups(cx["rec_pos"], cx["lig_pos"], 6, seed=5)


def test_rank_rule():
    from dfmdock_amd.restraints import rank_key
    energy = np.array([-5.0, -9.0, -7.0, -7.5, -7.5])
    sat = np.array([3, 2, 3, 3, 3])
    assert rank_key(energy, sat) == 3          # most satisfied first, then the lowest energy, the first of equal ones


def test_restraint_structs_have_the_c_layout(tmp_path):
    from dfmdock_amd import _lib
    src = tmp_path / "sz.c"
    body = 'printf("size %zu\\n", sizeof(dfm_restraint_params));'
    fields = [f for f, _ in _lib.RestraintParamsC._fields_]
    body += "".join(f'printf("{f} %zu\\n", offsetof(dfm_restraint_params, {f}));' for f in fields)
    body += 'printf("flag %u\\n", (unsigned)DFM_F_RESTRAINTS);'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_lib.RestraintParamsC)
    assert fields == ["k_tr", "k_rot", "max_tr", "max_rot", "t_start"]
    for f in fields:
        assert int(got[f]) == getattr(_lib.RestraintParamsC, f).offset, f
    assert int(got["flag"]) == _lib.DFM_F_RESTRAINTS == 1 << 14


def test_restraint_symbols_are_exported():
    from dfmdock_amd import _lib
    lib = _lib.lib()
    for s in ("dfm_complex_set_restraints", "dfm_restraint_eval"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert " T dfm_complex_set_restraints" in out and " T dfm_restraint_eval" in out


def test_driver_rows_keep_the_reference_schema_without_restraints():
    from dfmdock_amd import driver
    assert driver.CSV_FIELDS == ["id", "index", "c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ", "energy", "num_clashes"]
    assert driver.RESTRAINT_FIELDS == ["restraint_energy", "restraints_satisfied"]


def test_cli_accepts_the_restraint_options():
    from dfmdock_amd import cli
    a = cli.build_parser().parse_args(["dock", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz", "--restraints", "x.txt",
                                      "--restraint-rank", "energy"])
    assert a.restraints == "x.txt" and a.restraint_rank == "energy"
    a = cli.build_parser().parse_args(["dock", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz"])
    assert a.restraints is None and a.restraint_rank == "satisfied"
    s = cli.build_parser().parse_args(["sweep", "--db5", "d", "--ckpt", "m.ckpt", "--native-restraints", "3"])
    assert s.native_restraints == 3 and s.restraint_cutoff == 8.0
