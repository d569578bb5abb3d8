"""Consensus contact scoring on the GPU (dfm_pose_consensus, kernels_consensus.hip) against its float64 definition
dfmdock_amd/consensus.py, and through the drivers and the command line.

Everything the call returns is an integer.  `bits` must equal the definition's contacts on every residue pair whose float64 distance is
at least 1e-3 A from the cutoff (the border tests/test_gpu_metrics.py grants); a border pair may fall either way, and such pairs may be at
most 0.5 % of the definition's contacts.  count, rec_count, lig_count, n_contacts and score_sum must then equal, exactly, what the
definition's formulas give on the call's own bits, and consensus the shared host finish bit for bit."""
import csv
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, complex_for, db5_complex, db5_ids
from test_gpu_metrics import perturbations

pytestmark = pytest.mark.gpu

BORDER = 1e-3
INT_KEYS = ("count", "rec_count", "lig_count", "n_contacts", "score_sum")


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def check_against_definition(model, rec, poses, cutoff=5.5, members=None, label=""):
    """One call against the definition; returns (pair evaluations, definition contacts, border pairs, poses without a contact, result)."""
    from dfmdock_amd import consensus as CS
    rec, poses = np.asarray(rec, np.float32), np.asarray(poses, np.float32)
    P, R, L = poses.shape[0], rec.reshape(-1, 9).shape[0], poses.shape[1]
    got = model.consensus(rec, poses, cutoff=cutoff, members=members, bits=True)
    mine, high = CS.unpack_bits(got["bits"], L)
    assert got["bits"].shape == (P, R, (L + 63) // 64) and high == 0, (label, "bits set beyond L")
    n_con = n_border = n_empty = 0
    for p in range(P):
        d = CS.min_dist(rec, poses[p])
        with np.errstate(invalid="ignore"):
            want, border = d < cutoff, np.abs(d - cutoff) < BORDER
        n_con += int(want.sum())
        n_border += int(border.sum())
        n_empty += int(want.sum() == 0)
        wrong = (mine[p] != want) & ~border
        assert not wrong.any(), (label, p, np.argwhere(wrong)[:5].tolist(), d[wrong][:5].tolist())
    f = CS.from_contacts(mine, members)
    for k in INT_KEYS:
        assert got[k].dtype == f[k].dtype and np.array_equal(got[k], f[k]), (label, k)
    assert got["M"] == f["M"] and got["consensus"].tobytes() == CS.finish(got["score_sum"], got["n_contacts"], got["M"]).tobytes()
    assert np.array_equal(got["freq"], got["count"] / got["M"])
    print(f"{label}: P {P} R {R} L {L} contacts {n_con} border {n_border} empty poses {n_empty}")
    return P * R * L, n_con, n_border, n_empty, got


def test_parity_with_the_definition_on_db5(model):
    """Gate 1.  The recipe of test_gpu_metrics.py: 24 DB5 backbones in fixture order x 16 seeded rigid perturbations from one
    default_rng(0) stream, cutoff 5.5, every pose a member.  The definition alone gives 14 577 248 pair evaluations, 10 521 contacts,
    18 border pairs (0.17 %) and 22 poses without any contact on this recipe (counted on the CPU)."""
    rng = np.random.default_rng(0)
    tot = np.zeros(4, np.int64)
    for cid in db5_ids():
        c = db5_complex(cid)
        tot += check_against_definition(model, c["rec_pos"], perturbations(c["lig_pos"], rng), label=cid)[:4]
    print(f"pair evaluations {tot[0]}, contacts {tot[1]}, border pairs {tot[2]}, poses without a contact {tot[3]}")
    assert tot[0] == 14577248 and tot[1] == 10521
    assert tot[2] <= 0.005 * tot[1]


def _ensemble(case, P, seed, spread=3.0):
    """P poses of a golden complex: the native ligand under small rigid translations (most poses keep contacts)."""
    cx = complex_for(case)
    rng = np.random.default_rng(seed)
    lig = np.asarray(cx["lig_pos"], np.float32)
    poses = (lig[None] + (spread * rng.standard_normal((P, 1, 1, 3))).astype(np.float32)).astype(np.float32)
    return np.asarray(cx["rec_pos"], np.float32), poses


def test_invariances_are_exact(model):
    """Gate 2."""
    rec, poses = _ensemble("fwd_7CEI_p0", 96, 1)
    full = model.consensus(rec, poses, bits=True)
    assert full["count"].sum() > 0 and (full["n_contacts"] > 0).sum() > 48
    perm = np.random.default_rng(2).permutation(96)
    op = model.consensus(rec, poses[perm], bits=True)
    for k in ("count", "rec_count", "lig_count"):
        assert np.array_equal(op[k], full[k]), k
    for k in ("n_contacts", "score_sum", "consensus", "bits"):
        assert op[k].tobytes() == full[k][perm].tobytes(), k
    # count of a call = the sum over a split of its members
    a = np.arange(96) % 3 == 0
    oa, ob = model.consensus(rec, poses, members=a), model.consensus(rec, poses, members=~a)
    for k in ("count", "rec_count", "lig_count", "score_sum"):
        assert np.array_equal(oa[k] + ob[k], full[k]), k
    assert oa["M"] + ob["M"] == 96 and np.array_equal(oa["n_contacts"], full["n_contacts"])
    # a non-member's score = that of the same pose appended to a members-only call
    only = model.consensus(rec, np.concatenate([poses[a], poses[~a][:5]]), members=np.arange(a.sum() + 5) < a.sum())
    assert np.array_equal(only["count"], oa["count"])
    assert np.array_equal(only["score_sum"][a.sum():], oa["score_sum"][~a][:5]) and np.array_equal(only["score_sum"][: a.sum()], oa["score_sum"][a])
    # every output pointer but one NULL gives that one unchanged
    from dfmdock_amd import _lib as L
    lp, rp = np.ascontiguousarray(poses.reshape(96, -1, 9)), np.ascontiguousarray(rec.reshape(-1, 9))
    f = lambda x: x.ctypes.data_as(L.F32P)
    types = {"count": C.c_int32, "rec_count": C.c_int32, "lig_count": C.c_int32, "n_contacts": C.c_int32, "score_sum": C.c_int64, "bits": C.c_uint64}
    for k, t in types.items():
        buf = np.zeros_like(full[k])
        out = L.ConsensusOutC()
        setattr(out, k, buf.ctypes.data_as(C.POINTER(t)))
        assert L.lib().dfm_pose_consensus(model._h, 96, rp.shape[0], lp.shape[1], f(rp), f(lp), None, 5.5, C.byref(out)) == 0, k
        assert np.array_equal(buf, full[k]), k
    out = L.ConsensusOutC()
    assert L.lib().dfm_pose_consensus(model._h, 96, rp.shape[0], lp.shape[1], f(rp), f(lp), None, 5.5, C.byref(out)) == 0


def test_more_than_one_chunk(model):
    """Gate 3: the 1000 + 1000 complex, two chunks and a few poses of a third, against the same poses in single-chunk calls."""
    from dfmdock_amd import engine
    cx = complex_for("fwd_c5_1000_1000")
    rec, lig = np.asarray(cx["rec_pos"], np.float32), np.asarray(cx["lig_pos"], np.float32)
    Pc = engine.consensus_chunk_poses(1000, 1000)
    P = 2 * Pc + 37
    rng = np.random.default_rng(7)
    poses = np.empty((P, 1000, 3, 3), np.float32)
    poses[:] = lig[None]
    poses += (4.0 * rng.standard_normal((P, 1, 1, 3))).astype(np.float32)
    members = rng.random(P) < 0.7
    print(f"chunk {Pc} poses, call of {P} poses = {-(-P // Pc)} chunks")
    assert -(-P // Pc) == 3
    big = model.consensus(rec, poses, members=members, bits=True)
    assert big["count"].sum() > 0 and (big["n_contacts"] > 0).sum() > P // 4
    count = np.zeros_like(big["count"])
    rc, lc = np.zeros_like(big["rec_count"]), np.zeros_like(big["lig_count"])
    cuts = [0, Pc - 5, 2 * Pc - 9, P]      # pieces that are single chunks and do not end where the big call's chunks end
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        assert hi - lo <= Pc
        m = members[lo:hi] if members[lo:hi].any() else None
        o = model.consensus(rec, poses[lo:hi], members=m, bits=True)
        assert o["bits"].tobytes() == big["bits"][lo:hi].tobytes() and np.array_equal(o["n_contacts"], big["n_contacts"][lo:hi])
        count += o["count"]; rc += o["rec_count"]; lc += o["lig_count"]
    assert np.array_equal(count, big["count"]) and np.array_equal(rc, big["rec_count"]) and np.array_equal(lc, big["lig_count"])
    # score_sum against the summed count, pose by pose on a sample, from the bits
    from dfmdock_amd import consensus as CS
    for p in rng.choice(P, 24, replace=False).tolist() + [0, Pc - 1, Pc, 2 * Pc - 1, 2 * Pc, P - 1]:
        c, _ = CS.unpack_bits(big["bits"][p:p + 1], 1000)
        assert int(count[c[0]].sum(dtype=np.int64)) == int(big["score_sum"][p]) and int(c.sum()) == int(big["n_contacts"][p]), p
    assert big["M"] == int(members.sum())


def test_sizes(model):
    """Gate 4: L not a multiple of 64, R = 1, L = 1, P = 1 and a 9 + 7 complex, against the definition."""
    rng = np.random.default_rng(3)
    cx = complex_for("fwd_syn_9_7")
    rec97, lig97 = np.asarray(cx["rec_pos"], np.float32), np.asarray(cx["lig_pos"], np.float32)
    poses97 = (lig97[None] + (2.0 * rng.standard_normal((20, 1, 1, 3))).astype(np.float32)).astype(np.float32)
    assert check_against_definition(model, rec97, poses97, label="9 + 7")[1] > 0
    assert check_against_definition(model, rec97, poses97[:1], label="P = 1")[0] == 63
    assert check_against_definition(model, rec97[:1], poses97, label="R = 1")[0] == 20 * 7
    assert check_against_definition(model, rec97, poses97[:, :1], label="L = 1")[0] == 20 * 9
    assert check_against_definition(model, rec97[:1], poses97[:1, :1], label="1 x 1 x 1")[0] == 1
    for R, L in ((70, 65), (64, 64), (65, 127), (130, 193)):
        rec = (6.0 * rng.standard_normal((R, 1, 3)) + rng.standard_normal((R, 3, 3))).astype(np.float32)
        poses = (6.0 * rng.standard_normal((11, L, 1, 3)) + rng.standard_normal((11, L, 3, 3))).astype(np.float32)
        members = np.arange(11) % 2 == 0
        n = check_against_definition(model, rec, poses, members=members, label=f"{R} + {L}")
        assert n[1] > 50
        n = check_against_definition(model, rec, poses, cutoff=9.25, label=f"{R} + {L} cutoff 9.25")
    # NaN and infinite coordinates: no contact there, every other pose as it was
    clean = model.consensus(rec97, poses97)
    dirty = poses97.copy()
    dirty[3] = np.nan
    dirty[5, 2, 1, 0] = np.inf
    dirty[7, 4, 0, 2] = np.nan
    got = check_against_definition(model, rec97, dirty, label="NaN poses")[4]
    keep = np.ones(20, bool)
    keep[[3, 5, 7]] = False
    assert got["n_contacts"][3] == 0 and np.isnan(got["consensus"][3])
    assert np.array_equal(got["n_contacts"][keep], clean["n_contacts"][keep])
    # a far-away ensemble: nothing in contact
    far = model.consensus(rec97, poses97 + np.float32(1000.0))
    assert far["count"].sum() == 0 and (far["n_contacts"] == 0).all() and np.isnan(far["consensus"]).all()


def test_a_sampled_ensemble_and_the_pair_driver(model, tmp_path):
    """Gate 5: 256 refinement trajectories from the native pose of 7CEI, then the pair drivers with and without consensus."""
    from cli_fixtures import golden_7cei, write_pair
    from dfmdock_amd import cli, driver, engine
    from dfmdock_amd import consensus as CS
    from dfmdock_amd.cluster import rank_order, rebuild_backbone
    cx, rs, ls = golden_7cei()
    gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    r = gx.refine(B=256, t_begin=0.1, num_steps=8, seed=4, mfma16=True)
    gx.close()
    n = check_against_definition(model, cx["rec_pos"], r["lig_pos"], label="7CEI refine ensemble")
    assert n[1] > 256 and n[2] <= 0.005 * n[1]
    half = check_against_definition(model, cx["rec_pos"], r["lig_pos"], members=CS.energy_members(r["energy"], 0.5), label="best half")[4]
    assert half["M"] == 128
    # the pair drivers
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    kw = dict(num_samples=24, num_steps=8, seed=2, max_batch=16, selfcheck=False)
    plain = driver.refine_pair(model, rec, lig, rec_x, lig_x, t_begin=0.1, out_pdb=str(tmp_path / "plain.pdb"), **kw)
    off = driver.refine_pair(model, rec, lig, rec_x, lig_x, t_begin=0.1, out_pdb=str(tmp_path / "off.pdb"), consensus=False, **kw)
    scored = driver.refine_pair(model, rec, lig, rec_x, lig_x, t_begin=0.1, out_pdb=str(tmp_path / "scored.pdb"), consensus=True, **kw)
    kept = driver.refine_pair(model, rec, lig, rec_x, lig_x, t_begin=0.1, out_pdb=str(tmp_path / "kept.pdb"), rank="consensus", **kw)

    def same(a, b):
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], dict):
                same(a[k], b[k]) if a[k] is not None and b[k] is not None else None
            else:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    same(plain, off)
    assert "consensus" not in plain and "consensus_data" not in plain
    pdb = lambda name: open(tmp_path / name, "rb").read()
    assert pdb("plain.pdb") == pdb("off.pdb") == pdb("scored.pdb")      # scoring alone changes nothing that is written
    same(plain, {k: v for k, v in scored.items() if k not in ("consensus", "consensus_data")})
    cd = scored["consensus_data"]
    poses = rebuild_backbone(np.asarray(lig["bb_coords"], np.float32), plain["trajectories"]["rot_update"], plain["trajectories"]["tr_update"])
    want = model.consensus(np.asarray(rec["bb_coords"], np.float32), poses)
    for k in INT_KEYS:
        assert np.array_equal(cd[k], want[k]), k
    assert not np.isnan(cd["consensus"]).all()
    order = rank_order(-cd["consensus"], 24)
    s = scored["consensus"]
    assert s["ranked_by"] == "energy" and not s["fallback"] and s["M"] == 24 and s["cutoff"] == 5.5
    assert s["rank"] == int(np.nonzero(order == plain["index"])[0][0]) + 1 and s["n_contacts"] == int(cd["n_contacts"][plain["index"]])
    first = kept["index"]
    assert first == CS.pick(cd["consensus"], plain["trajectories"]["energy"])
    assert cd["consensus"][first] == cd["consensus"][order[0]] and kept["consensus"]["ranked_by"] == "consensus"
    # `rank` is the kept pose's position under rank_order(-consensus) (ties to the lower index), whatever pick()'s energy tie-break did
    assert kept["consensus"]["score"] == float(cd["consensus"][first]) and kept["consensus"]["rank"] == int(np.nonzero(order == first)[0][0]) + 1
    assert kept["energy"] == float(plain["trajectories"]["energy"][first])
    assert np.array_equal(kept["rot_update"], plain["trajectories"]["rot_update"][first])
    # dock_pair: free runs of seeded weights; with clustering the consensus order is the key, and the default stays what it was
    dkw = dict(num_samples=12, num_steps=6, seed=3, max_batch=8, selfcheck=False)
    d0 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "d0.pdb"), **dkw)
    d1 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "d1.pdb"), consensus=False, rank="energy", **dkw)
    d2 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "d2.pdb"), consensus=True, **dkw)
    same(d0, d1)
    assert pdb("d0.pdb") == pdb("d1.pdb") == pdb("d2.pdb")
    same(d0, {k: v for k, v in d2.items() if k not in ("consensus", "consensus_data", "index", "trajectories")})
    # rank="consensus" in dock_pair.  Free runs of seeded weights need not touch the receptor at 5.5 A, so the cutoff is taken from the
    # ensemble itself: of the trajectories' closest approaches to the receptor (+ 2 A), the first cutoff at which the consensus pick is
    # not the energy pick.  Both branches of the driver are then asserted, none left to what the data happens to give.
    traj = d2["trajectories"]
    k0 = int(np.argmin(traj["energy"]))
    assert d2["index"] == k0 and d2["energy"] == float(traj["energy"][k0]) and np.array_equal(d2["rot_update"], traj["rot_update"][k0])
    rec_bb = np.asarray(rec["bb_coords"], np.float32)
    dposes = rebuild_backbone(np.asarray(lig["bb_coords"], np.float32), traj["rot_update"], traj["tr_update"])
    closest = np.sort([float(np.nanmin(CS.min_dist(rec_bb, p))) for p in dposes])
    print("closest approach of the 12 free trajectories (A):", np.round(closest, 2).tolist(), "energy pick", k0)
    cut = want3 = None
    for c in closest + 2.0:
        w = model.consensus(rec_bb, dposes, cutoff=float(c))
        k = CS.pick(w["consensus"], traj["energy"])
        if k is not None and k != k0:
            cut, want3 = float(np.float32(c)), w
            break
    assert cut is not None, "no cutoff separates the consensus pick from the energy pick on this ensemble"
    d3 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "d3.pdb"), rank="consensus", consensus_cutoff=cut, top_k=3,
                          cluster_radius=3.0, **dkw)
    c3 = d3["consensus_data"]["consensus"]
    k3 = CS.pick(want3["consensus"], traj["energy"])
    print(f"cutoff {cut:.3f} A: consensus pick {k3} (score {c3[k3]:.4f}), energy pick {k0} (score {c3[k0]})")
    assert np.array_equal(c3, want3["consensus"], equal_nan=True) and d3["consensus"]["cutoff"] == cut
    assert not d3["consensus"]["fallback"] and d3["consensus"]["ranked_by"] == "consensus" and d3["index"] == k3 != k0
    assert d3["consensus"]["score"] == float(c3[k3]) and d3["consensus"]["rank"] == int(np.nonzero(rank_order(-c3, 12) == k3)[0][0]) + 1
    assert d3["energy"] == float(traj["energy"][k3]) != d0["energy"]
    assert np.array_equal(d3["rot_update"], traj["rot_update"][k3]) and np.array_equal(d3["tr_update"], traj["tr_update"][k3])
    from dfmdock_amd import pdbio
    aa = pdbio.apply_pose_all_atom(lig["aa_coords"], lig["bb_coords"], traj["rot_update"][k3], traj["tr_update"][k3], center="ca")
    assert np.array_equal(d3["lig_aa_coords"], aa) and pdb("d3.pdb") != pdb("d0.pdb")
    pdbio.write_complex_pdb(str(tmp_path / "want3.pdb"), list(rec["atoms"]), lig["atoms"], aa)
    assert pdb("d3.pdb") == pdb("want3.pdb")
    assert d3["models"][0]["index"] == k3 and pdb("d3_1.pdb") == pdb("d3.pdb")      # leader clustering in consensus order: model 1 is the kept pose
    e3 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "e3.pdb"), top_k=3, cluster_radius=3.0, **dkw)
    assert e3["models"][0]["index"] == k0      # ... and in energy order without it
    # the forced fallback: no pair of any pose is within 1e-3 A, every score NaN, the energy pick stays and the result says so
    d4 = driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=str(tmp_path / "d4.pdb"), rank="consensus", consensus_cutoff=1e-3, top_k=3,
                          cluster_radius=3.0, **dkw)
    assert np.isnan(d4["consensus_data"]["consensus"]).all() and d4["consensus_data"]["count"].sum() == 0
    assert d4["consensus"]["fallback"] and d4["consensus"]["ranked_by"] == "energy" and d4["consensus"]["score"] is None
    assert d4["index"] == k0 and d4["energy"] == d0["energy"] and pdb("d4.pdb") == pdb("d0.pdb") and d4["models"][0]["index"] == k0
    with pytest.raises(ValueError):
        driver.dock_pair(model, rec, lig, rec_x, lig_x, out_pdb=None, rank="size", **dkw)


def test_invalid_arguments(model):
    """Gate 6: DFM_E_INVALID (-1), nothing enqueued, and a message naming the argument."""
    from dfmdock_amd import _lib as L
    rec, poses = _ensemble("fwd_syn_24_16", 6, 1)
    rp, lp = np.ascontiguousarray(rec.reshape(-1, 9)), np.ascontiguousarray(poses.reshape(6, -1, 9))
    f = lambda x: x.ctypes.data_as(L.F32P)
    out = L.ConsensusOutC()
    n_con = np.zeros(6, np.int32)
    out.n_contacts = n_con.ctypes.data_as(L.I32P)
    none = np.zeros(6, np.uint8)
    u8 = none.ctypes.data_as(C.POINTER(C.c_uint8))
    h, o, lib = model._h, C.byref(out), L.lib()
    cases = [((None, 6, 24, 16, f(rp), f(lp), None, 5.5, o), "m is NULL"), ((h, 6, 24, 16, None, f(lp), None, 5.5, o), "rec_pos is NULL"),
             ((h, 6, 24, 16, f(rp), None, None, 5.5, o), "lig_pos is NULL"), ((h, 6, 24, 16, f(rp), f(lp), None, 5.5, None), "out is NULL"),
             ((h, 0, 24, 16, f(rp), f(lp), None, 5.5, o), "P must be in 1 .. 65536"), ((h, 65537, 24, 16, f(rp), f(lp), None, 5.5, o), "P must be in 1 .. 65536"),
             ((h, 6, 0, 16, f(rp), f(lp), None, 5.5, o), "R >= 1"), ((h, 6, 24, 0, f(rp), f(lp), None, 5.5, o), "L >= 1"),
             ((h, 6, 1 << 14, (1 << 13) + 1, f(rp), f(lp), None, 5.5, o), "R x L exceeds 2^27"),
             ((h, 6, 24, 16, f(rp), f(lp), None, float("nan"), o), "cutoff must be finite and > 0"), ((h, 6, 24, 16, f(rp), f(lp), None, float("inf"), o), "cutoff must be finite and > 0"),
             ((h, 6, 24, 16, f(rp), f(lp), None, 0.0, o), "cutoff must be finite and > 0"), ((h, 6, 24, 16, f(rp), f(lp), None, -1.0, o), "cutoff must be finite and > 0"),
             ((h, 6, 24, 16, f(rp), f(lp), u8, 5.5, o), "member: no pose is a member")]
    for args, word in cases:
        assert lib.dfm_pose_consensus(*args) == -1, word
        msg = lib.dfm_last_error().decode()
        print(word, "->", msg)
        assert word in msg, (word, msg)
    assert lib.dfm_consensus_last_timing(None, None) == -1
    assert lib.dfm_pose_consensus(h, 6, 24, 16, f(rp), f(lp), None, 5.5, o) == 0 and n_con.sum() > 0      # the handle still works
    with pytest.raises(ValueError):
        model.consensus(rec, poses, members=np.zeros(6, bool))
    with pytest.raises(ValueError):
        model.consensus(rec, poses, cutoff=-2.0)
    with pytest.raises(ValueError):
        model.consensus(rec, poses, members=np.ones(5, bool))


def test_threads_next_to_a_sampling_handle(model):
    """Gate 7: four host threads on different ensembles while a Complex samples; results equal the serial calls."""
    from dfmdock_amd import engine
    sets = [_ensemble("fwd_7CEI_p0", 300, 11), _ensemble("fwd_syn_64_48_p0", 700, 12), _ensemble("fwd_syn_24_16", 2000, 13),
            _ensemble("fwd_c3_300_300", 128, 14)]
    mem = [None, np.arange(700) % 2 == 0, None, np.arange(128) < 100]
    serial = [model.consensus(r, p, members=m, bits=True) for (r, p), m in zip(sets, mem)]
    assert all(s["count"].sum() > 0 for s in serial)
    cx = complex_for("fwd_syn_24_16")
    gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    ref_s = gx.sample(B=8, num_steps=6, seed=2, mfma16=True)
    res, errs = [None] * 4, []

    def work(i):
        try:
            res[i] = [model.consensus(sets[i][0], sets[i][1], members=mem[i], bits=True) for _ in range(3)]
        except BaseException as e:      # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    s = gx.sample(B=8, num_steps=6, seed=2, mfma16=True)
    for t in th:
        t.join()
    gx.close()
    assert not errs, errs
    assert np.array_equal(s["lig_pos"], ref_s["lig_pos"])
    for i in range(4):
        for r in res[i]:
            for k in INT_KEYS + ("bits", "consensus"):
                assert r[k].tobytes() == serial[i][k].tobytes(), (i, k)
    cp, kn = engine.consensus_last_timing()
    assert cp > 0 and kn > 0


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def test_cli_consensus_artefacts_and_sweep_columns(tmp_path):
    """Gate 8.  `refine` from the native pose gives an ensemble in contact: the three artefacts, the written restraints accepted by a
    second `dock --restraints` run; `dock --consensus` on free runs; `sweep --consensus` adds exactly the two columns."""
    from cli_fixtures import golden_7cei, write_ckpt, write_db5_pt, write_pair
    from dfmdock_amd import pdbio
    from dfmdock_amd.restraints import read_restraints
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    base = [rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--seed", "3", "--max-batch", "8", "--no-selfcheck"]
    small = ["--num-samples", "8", "--num-steps", "6"]
    p0 = _run(["refine"] + base + small, cwd=str(tmp_path))
    assert p0.returncode == 0, p0.stdout + p0.stderr
    plain, plain_pdb = json.loads(p0.stdout.strip().splitlines()[-1]), open(tmp_path / "output.pdb", "rb").read()
    p = _run(["refine"] + base + small + ["--consensus", "--contact-map", "map.npz", "--write-restraints", "cons.txt", "--restraint-top", "6",
                                          "--restraint-upper", "9", "--json", "res.json"], cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert open(tmp_path / "output.pdb", "rb").read() == plain_pdb
    new = {"consensus", "index", "contact_map", "restraints_written", "restraints_written_n"}
    assert {k: v for k, v in line.items() if k not in new or k in plain} == plain and "consensus" not in plain
    assert set(line["consensus"]) == {"score", "rank", "n_contacts", "M", "cutoff", "ranked_by", "fallback"}
    assert line["consensus"]["M"] == 8 and line["consensus"]["cutoff"] == 5.5 and 1 <= line["consensus"]["rank"] <= 8
    m = np.load(tmp_path / "map.npz")
    rec, lig = (pdbio.backbone_from_atoms(pdbio.read_pdb(x)) for x in (rec_pdb, lig_pdb))
    R, L = len(rec["bb_coords"]), len(lig["bb_coords"])
    assert set(m.files) == {"count", "freq", "rec_count", "lig_count", "M", "cutoff", "rec_residues", "lig_residues"}
    assert m["count"].shape == (R, L) and m["count"].dtype == np.int32 and int(m["M"]) == 8 and float(m["cutoff"]) == 5.5
    assert np.array_equal(m["freq"], m["count"] / 8) and m["count"].max() >= 1 and m["rec_count"].shape == (R,) and m["lig_count"].shape == (L,)
    assert len(m["rec_residues"]) == R and len(m["lig_residues"]) == L and str(m["rec_residues"][0]).startswith("A:")
    groups = read_restraints(str(tmp_path / "cons.txt"), rec, lig)
    assert len(groups) == line["restraints_written_n"] == 6 and all(g.upper == 9.0 and len(g.pairs) == 1 for g in groups)
    (i, j), = groups[0].pairs
    assert m["count"][i, j] == m["count"].max() and groups[0].weight == float(m["freq"][i, j])
    assert os.path.exists(tmp_path / "res.json")
    # the loop closes: a second, guided run takes the file
    q = _run(["dock"] + base + small + ["--restraints", "cons.txt", "--consensus", "--rank", "consensus", "--out", "guided.pdb"], cwd=str(tmp_path))
    assert q.returncode == 0, q.stdout + q.stderr
    gl = json.loads(q.stdout.strip().splitlines()[-1])
    assert gl["restraints"] == 6 and (tmp_path / "guided.pdb").exists()
    assert gl["consensus"]["ranked_by"] == ("energy" if gl["consensus"]["fallback"] else "consensus")
    # dock: the flags off leave the line alone, --consensus adds the object
    d0 = _run(["dock"] + base + small + ["--out", "dock.pdb"], cwd=str(tmp_path))
    d1 = _run(["dock"] + base + small + ["--out", "dock1.pdb", "--consensus", "--consensus-top", "0.5", "--contact-map", "dmap.npz",
                                         "--write-restraints", "dcons.txt", "--restraint-top", "4"], cwd=str(tmp_path))
    assert d0.returncode == 0 and d1.returncode == 0, d0.stderr + d1.stderr
    l0, l1 = (json.loads(x.stdout.strip().splitlines()[-1]) for x in (d0, d1))
    assert "consensus" not in l0 and l1["consensus"]["M"] == 4
    assert {k: v for k, v in l1.items() if k not in new | {"output"}} == {k: v for k, v in l0.items() if k != "output"}
    assert open(tmp_path / "dock.pdb", "rb").read() == open(tmp_path / "dock1.pdb", "rb").read()
    # the three artefacts of `dock` itself: the object on the line, the map and the restraint file (free runs of seeded weights may have
    # no contact at all: the map is then all zero and the file holds its header line and no group)
    dm = np.load(tmp_path / "dmap.npz")
    assert set(dm.files) == set(m.files) and dm["count"].shape == (R, L) and int(dm["M"]) == 4 and np.array_equal(dm["freq"], dm["count"] / 4)
    dtext = (tmp_path / "dcons.txt").read_text()
    dgroups = read_restraints(str(tmp_path / "dcons.txt"), rec, lig)
    assert dtext.startswith("# top ") and len(dgroups) == l1["restraints_written_n"] == min(4, int((dm["count"] > 0).sum()))
    assert len(dtext.splitlines()) == 1 + len(dgroups) and all(dm["count"][g.pairs[0]] >= 1 and g.upper == 8.0 for g in dgroups)
    assert os.path.samefile(l1["contact_map"], tmp_path / "dmap.npz") and os.path.samefile(l1["restraints_written"], tmp_path / "dcons.txt")
    # sweep
    d = tmp_path / "db5"
    d.mkdir()
    write_db5_pt(str(d / "7CEI.pt"), "7CEI", cx, rs, ls)
    write_db5_pt(str(d / "SYN1.pt"), "SYN1", complex_for("fwd_syn_24_16"), "A" * 24, "G" * 16)
    sw = ["sweep", "--db5", str(d), "--ckpt", ck, "--num-samples", "6", "--num-steps", "6"]
    s0 = _run(sw + ["--out-csv", "r0.csv"], cwd=str(tmp_path))
    s1 = _run(sw + ["--out-csv", "r1.csv", "--consensus", "--summary", "s.json"], cwd=str(tmp_path))
    assert s0.returncode == 0 and s1.returncode == 0, s0.stderr + s1.stderr
    r0, r1 = (list(csv.DictReader(open(tmp_path / x))) for x in ("r0.csv", "r1.csv"))
    base_cols = ["id", "index", "c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ", "energy", "num_clashes"]
    assert list(r0[0]) == base_cols and list(r1[0]) == base_cols + ["consensus", "n_contacts"] and len(r0) == len(r1) == 12
    assert [{k: r[k] for k in base_cols} for r in r1] == r0
    assert all(int(r["n_contacts"]) >= 0 and (int(r["n_contacts"]) > 0) == (r["consensus"] != "nan") for r in r1)
    assert "consensus pick" in s1.stdout and "consensus pick" not in s0.stdout
    sm = json.load(open(tmp_path / "s.json"))
    assert set(sm["consensus"]["complexes"]) == {"7CEI", "SYN1"} and set(sm["consensus"]["success"]) == {"acceptable", "medium", "high"}
