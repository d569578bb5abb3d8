"""Consensus contact scoring without a GPU: the float64 definition (dfmdock_amd/consensus.py) on hand-made cases with known answers, its
invariances, the consensus contacts as restraints, the command-line flags and the C ABI's new struct and symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def residue(ca, spread=1.0):
    """One residue [9]: N and C `spread` A either side of CA along x."""
    ca = np.asarray(ca, np.float32)
    return np.concatenate([ca - np.float32([spread, 0, 0]), ca, ca + np.float32([spread, 0, 0])]).astype(np.float32)


def toy():
    """Receptor: 3 residues 20 A apart on the y axis.  Ligand of 2 residues; pose 0 puts ligand 0 next to receptor 0 and ligand 1 next to
    receptor 1, pose 1 only ligand 0 next to receptor 0, pose 2 is far from everything, pose 3 puts ligand 1 next to receptor 2."""
    rec = np.stack([residue([0, 20.0 * i, 0]) for i in range(3)])
    far = [500.0, 500.0, 500.0]
    lig = np.stack([np.stack([residue([0, 0, 4.0]), residue([0, 20.0, 4.0])]),
                    np.stack([residue([0, 0, 4.0]), residue(far)]),
                    np.stack([residue(far), residue([520.0, 500.0, 500.0])]),
                    np.stack([residue(far), residue([0, 40.0, 4.0])])])
    return rec, lig


def test_known_answers_two_poses_sharing_one_contact():
    from dfmdock_amd import consensus as CS
    from dfmdock_amd.cluster import rank_order
    rec, lig = toy()
    o = CS.consensus(rec, lig[:3])
    assert o["M"] == 3 and o["cutoff"] == 5.5
    np.testing.assert_array_equal(o["count"], [[2, 0], [0, 1], [0, 0]])
    np.testing.assert_array_equal(o["rec_count"], [2, 1, 0])
    np.testing.assert_array_equal(o["lig_count"], [2, 1])
    np.testing.assert_array_equal(o["n_contacts"], [2, 1, 0])
    np.testing.assert_array_equal(o["score_sum"], [3, 2, 0])
    assert o["count"].dtype == np.int32 and o["n_contacts"].dtype == np.int32 and o["score_sum"].dtype == np.int64
    np.testing.assert_array_equal(o["consensus"][:2], [3 / (3 * 2), 2 / (3 * 1)])
    assert np.isnan(o["consensus"][2])      # no contact: NaN, ranked last
    np.testing.assert_array_equal(rank_order(-o["consensus"], 3), [1, 0, 2])
    np.testing.assert_array_equal(o["freq"], o["count"] / 3)
    # the strict cutoff: atoms exactly 4.0 apart
    assert CS.contacts(rec, lig[:1], cutoff=4.0).sum() == 0 and CS.contacts(rec, lig[:1], cutoff=4.000001).sum() == 2
    # the shared finish
    np.testing.assert_array_equal(CS.finish(o["score_sum"], o["n_contacts"], 3)[:2], o["consensus"][:2])


def test_non_members_are_scored_but_not_counted():
    from dfmdock_amd import consensus as CS
    rec, lig = toy()
    o = CS.consensus(rec, lig, members=[True, True, False, False])
    assert o["M"] == 2
    np.testing.assert_array_equal(o["count"], [[2, 0], [0, 1], [0, 0]])      # pose 3's contact (2, 1) is not counted
    np.testing.assert_array_equal(o["n_contacts"], [2, 1, 0, 1])
    np.testing.assert_array_equal(o["score_sum"], [3, 2, 0, 0])              # ... and scores 0 against the members' counts
    np.testing.assert_array_equal(o["consensus"][[0, 1, 3]], [3 / 4, 2 / 2, 0.0])
    with pytest.raises(ValueError, match="no pose is a member"):
        CS.consensus(rec, lig, members=[False] * 4)
    with pytest.raises(ValueError):
        CS.consensus(rec, lig, members=[True] * 3)
    with pytest.raises(ValueError):
        CS.consensus(rec, lig, cutoff=0.0)


def test_nan_coordinates_disturb_no_other_pose():
    from dfmdock_amd import consensus as CS
    rec, lig = toy()
    clean = CS.consensus(rec, lig)
    dirty = lig.copy()
    dirty[1, 0, 4] = np.nan      # one coordinate of ligand residue 0 of pose 1
    o = CS.consensus(rec, dirty)
    assert o["n_contacts"][1] == 0 and np.isnan(o["consensus"][1])
    np.testing.assert_array_equal(o["n_contacts"][[0, 2, 3]], clean["n_contacts"][[0, 2, 3]])
    np.testing.assert_array_equal(o["count"], [[1, 0], [0, 1], [0, 1]])
    allnan = np.full_like(lig, np.nan)
    z = CS.consensus(rec, allnan)
    assert z["count"].sum() == 0 and np.isnan(z["consensus"]).all()


def _random_case(seed, P=12, R=9, L=70):
    rng = np.random.default_rng(seed)
    rec = (rng.standard_normal((R, 3, 3)) * 4).astype(np.float32)
    lig = (rng.standard_normal((P, L, 3, 3)) * 4 + rng.standard_normal((P, 1, 1, 3)) * 3).astype(np.float32)
    return rec, lig


def test_count_is_additive_and_permutation_invariant():
    from dfmdock_amd import consensus as CS
    rec, lig = _random_case(1)
    full = CS.consensus(rec, lig)
    assert 0 < full["count"].sum() < lig.shape[0] * 9 * 70
    a, b = np.arange(12) < 5, np.arange(12) >= 5
    oa, ob = CS.consensus(rec, lig, members=a), CS.consensus(rec, lig, members=b)
    for k in ("count", "rec_count", "lig_count"):
        np.testing.assert_array_equal(oa[k] + ob[k], full[k])
    np.testing.assert_array_equal(oa["score_sum"] + ob["score_sum"], full["score_sum"])
    perm = np.random.default_rng(2).permutation(12)
    op = CS.consensus(rec, lig[perm])
    for k in ("count", "rec_count", "lig_count"):
        np.testing.assert_array_equal(op[k], full[k])
    for k in ("n_contacts", "score_sum", "consensus"):
        np.testing.assert_array_equal(op[k], full[k][perm])
    # bits round trip, L not a multiple of 64
    c = CS.contacts(rec, lig)
    bits = CS.pack_bits(c)
    assert bits.shape == (12, 9, 2) and bits.dtype == np.uint64
    back, high = CS.unpack_bits(bits, 70)
    assert high == 0 and np.array_equal(back, c)
    assert bool(bits[0, 0, 1] >> np.uint64(5) & np.uint64(1)) == bool(c[0, 0, 69])
    f = CS.from_contacts(back)
    for k in ("count", "score_sum", "n_contacts"):
        np.testing.assert_array_equal(f[k], full[k])


def test_top_contacts_tie_order_pick_and_members():
    from dfmdock_amd import consensus as CS
    count = np.array([[3, 5, 0], [5, 1, 3]], np.int32)
    np.testing.assert_array_equal(CS.top_contacts(count, 4), [[0, 1], [1, 0], [0, 0], [1, 2]])      # ties in row-major order
    np.testing.assert_array_equal(CS.top_contacts(count, 10, min_count=3), [[0, 1], [1, 0], [0, 0], [1, 2]])
    assert CS.top_contacts(count, 0).shape == (0, 2) and CS.top_contacts(np.zeros((2, 2), np.int32), 5).shape == (0, 2)
    g = CS.contact_groups(count, 5, 2, upper=7.5)
    assert [x.pairs for x in g] == [((0, 1),), ((1, 0),)] and g[0].upper == 7.5 and g[0].weight == 1.0
    s, e = np.array([0.5, np.nan, 0.75, 0.75, 0.75]), np.array([1.0, -9.0, 2.0, -1.0, -1.0])
    assert CS.pick(s, e) == 3      # highest consensus, then lower energy, then lower index
    key = CS.rank_positions(s, e)
    np.testing.assert_array_equal(np.argsort(key), [3, 4, 2, 0, 1])
    assert CS.pick([np.nan, np.nan], [1.0, 0.0]) is None
    np.testing.assert_array_equal(CS.energy_members([3.0, 1.0, 2.0, np.nan], 0.5), [False, True, True, False])
    np.testing.assert_array_equal(CS.energy_members([3.0, 1.0, 2.0], 0.1), [False, True, False])      # at least one
    assert CS.energy_members([3.0, 1.0], 1.0).all()
    with pytest.raises(ValueError):
        CS.energy_members([1.0], 0.0)


def test_restraint_writer_round_trip_on_7cei(tmp_path):
    from cli_fixtures import golden_7cei, write_pair
    from dfmdock_amd import consensus as CS
    from dfmdock_amd import pdbio
    from dfmdock_amd.restraints import RestraintGroup, parse_restraints
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, _ = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig = (pdbio.backbone_from_atoms(pdbio.read_pdb(p)) for p in (rec_pdb, lig_pdb))
    rng = np.random.default_rng(4)
    poses = (np.asarray(lig["bb_coords"], np.float32)[None] + rng.standard_normal((7, 1, 1, 3)).astype(np.float32)).astype(np.float32)
    o = CS.consensus(np.asarray(rec["bb_coords"], np.float32), poses)
    groups = CS.contact_groups(o["count"], o["M"], 12)
    assert len(groups) == 12 and all(len(g.pairs) == 1 and g.upper == 8.0 for g in groups)
    assert [g.weight for g in groups] == sorted((g.weight for g in groups), reverse=True) and groups[0].weight == o["freq"].max()
    path = tmp_path / "consensus.txt"
    CS.write_restraints(str(path), groups, rec, lig, header="top contacts\nsecond line")
    text = path.read_text()
    assert text.startswith("# top contacts\n# second line\n") and len(text.splitlines()) == 14
    assert parse_restraints(text, rec, lig) == groups      # same pairs, bounds and weights, bit for bit
    multi = [RestraintGroup(((0, 1), (0, 2), (3, 1), (3, 2)), 6.5, 0.1 + 0.2)]
    assert parse_restraints(CS.format_restraints(multi, rec, lig), rec, lig) == multi
    with pytest.raises(ValueError):
        CS.format_restraints([RestraintGroup(((0, 1), (3, 2)), 6.5)], rec, lig)


def test_cli_flags_parse_and_default_off():
    from dfmdock_amd import cli
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert a.consensus is False and a.rank == "energy" and a.contact_map is None and a.write_restraints is None
        assert a.consensus_top == 1.0 and a.restraint_top == 10 and a.restraint_upper == 8.0
        assert cli.consensus_kwargs(a) == {}
        a = cli.parse_args([cmd] + base + ["--consensus", "--consensus-top", "0.25"])
        assert cli.consensus_kwargs(a) == dict(consensus=True, rank="energy", consensus_top=0.25)
        for extra in (["--rank", "consensus"], ["--contact-map", "m.npz"], ["--write-restraints", "r.txt", "--restraint-top", "5", "--restraint-upper", "7"]):
            a = cli.parse_args([cmd] + base + extra)
            assert a.consensus is True
        assert a.restraint_top == 5 and a.restraint_upper == 7.0
        for bad in (["--consensus", "--consensus-top", "0"], ["--consensus", "--consensus-top", "1.5"], ["--rank", "size"],
                    ["--write-restraints", "r.txt", "--restraint-top", "0"], ["--write-restraints", "r.txt", "--restraint-upper", "-1"],
                    ["--consensus-top", "0.5"], ["--consensus", "--restraint-top", "5"], ["--consensus", "--restraint-upper", "7"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    s = cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c.ckpt"])
    assert s.consensus is False and s.consensus_top == 1.0
    s = cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c.ckpt", "--consensus", "--consensus-top", "0.5"])
    assert s.consensus is True and s.consensus_top == 0.5
    for bad in (["--consensus-top", "0.5"], ["--consensus", "--consensus-top", "-1"]):      # the option without its flag; out of range
        with pytest.raises(SystemExit):
            cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c.ckpt"] + bad)


def test_sweep_consensus_table():
    from dfmdock_amd import cli
    rows = [{"id": "A", "index": "0", "DockQ": 0.1, "energy": -5.0, "consensus": 0.2, "n_contacts": 4},
            {"id": "A", "index": "1", "DockQ": 0.6, "energy": -1.0, "consensus": 0.9, "n_contacts": 7},
            {"id": "B", "index": "0", "DockQ": 0.3, "energy": -2.0, "consensus": float("nan"), "n_contacts": 0},
            {"id": "B", "index": "1", "DockQ": 0.0, "energy": -1.0, "consensus": float("nan"), "n_contacts": 0}]
    per, table = cli.consensus_table(rows)
    assert per["A"]["index"] == 1 and not per["A"]["fallback"] and per["B"]["index"] == 0 and per["B"]["fallback"]
    assert table["acceptable"]["consensus_top1"] == 1.0 and table["medium"]["consensus_top1"] == 0.5 and table["high"]["consensus_top1"] == 0.0
    _, etable = cli.success_table(rows)
    assert "consensus pick" in cli.format_consensus_table(per, table, etable)


def test_consensus_struct_layout_and_exports(tmp_path):
    """dfm_consensus_out as gcc lays it out against the ctypes mirror; the new symbols are declared, exported and listed."""
    from dfmdock_amd import _lib
    fields = [f for f, _ in _lib.ConsensusOutC._fields_]
    assert fields == ["count", "rec_count", "lig_count", "n_contacts", "score_sum", "bits"]
    body = 'printf("size %zu\\n", sizeof(dfm_consensus_out));' + "".join(
        f'printf("{f} %zu\\n", offsetof(dfm_consensus_out, {f}));' for f in fields)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_lib.ConsensusOutC)
    for f in fields:
        assert int(got[f]) == getattr(_lib.ConsensusOutC, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_pose_consensus", "dfm_consensus_last_timing", "dfm_consensus_chunk_poses"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    from test_abi_cpu import header_symbols
    assert sorted(_lib.EXPORTS) == header_symbols()
    # the chunk size is host arithmetic: 256 MiB of poses and bits
    assert lib.dfm_consensus_chunk_poses(1000, 1000) == (256 << 20) // (1000 * 36 + 1000 * 16 * 8) == 1636
    assert lib.dfm_consensus_chunk_poses(300, 300) == (256 << 20) // (300 * 36 + 300 * 5 * 8) > 10240
    assert lib.dfm_consensus_chunk_poses(1, 1) == 32768 and lib.dfm_consensus_chunk_poses(0, 5) == 0


def test_the_audits_see_the_new_kernels():
    """Every kernel of kernels_consensus.hip is in the shipped code object (so the scratch / LDS / op_sel audits of test_abi_cpu.py run
    over it) and uses no scratch."""
    import re
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_consensus.hip")).read()
    names = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))
    assert names == {"k_contact_bits", "k_contact_count", "k_contact_marginals", "k_contact_score"}
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
            for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", notes, re.S):
                for n in names:
                    if re.search(r"\d+" + n + r"E", m.group(1)):
                        found[n] = int(m.group(2))
        assert found == {n: 0 for n in names}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)
