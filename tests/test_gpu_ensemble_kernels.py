"""The clustering and consensus kernels launch by launch (kernels_cluster.hip: k_pose_dist, k_cluster_leader, k_cluster_count,
k_cluster_pick, k_cluster_dec; kernels_consensus.hip: k_contact_bits, k_contact_count, k_contact_marginals, k_contact_score), driven
through tests/kernels/ensemble_harness.hip on small host arrays with guard bands around every device block, against the float64
definitions (dfmdock_amd/cluster.py, dfmdock_amd/consensus.py) and the numpy restatements of tests/ensemble_harness.py
(tests/test_ensemble_harness_cpu.py shows that the restatements agree with the definitions on these inputs and that the comparisons
used here reject 23 seeded mutants of them).

What is exact and what carries a gate (ensemble_harness.py states each with its derivation):
  RMSD             (D / 2 + 4) 2^-24 rmsd around float64, D = 9 n_res; bit for bit the restated fp32 chain; diagonal 0, bitwise symmetric.
  mask             bit for bit the restatement; equal to float64 outside a border of that relative width around the radius (at most
                   0.5 % of the generic pairs, none of the lattice pairs); symmetric, diagonal set for finite poses, nothing at or
                   beyond B; the pair planted exactly on the radius is a neighbour.
  clustering       on crafted masks, every number exact: n, center, size, cluster_of against cluster.cluster_adjacency, counts, U and
                   state launch by launch against a step-by-step restatement, mlist as a set.
  consensus        every word of k_contact_bits equals consensus.contacts (no border); counts and sums array_equal.
The largest RMSD error / gate per D and the pair counts go to $DFM_ENSEMBLE_PROFILE/ensemble_kernels_gpu.txt when that variable names a
directory (profiles/ensemble_kernels.txt holds the MI355X figures).
"""
import os

import numpy as np
import pytest

import ensemble_harness as eh
from ensemble_harness import u32

pytestmark = pytest.mark.gpu

RATIOS = {}
COUNTS = {}


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    harness = eh.Harness(eh.compile_shim(tmp_path_factory.mktemp("ensemble_harness_gpu")))
    yield harness
    out = os.environ.get("DFM_ENSEMBLE_PROFILE")
    if out:
        with open(os.path.join(out, "ensemble_kernels_gpu.txt"), "w") as f:
            f.write("comparison max_error_over_gate\n" + "".join(f"{k} {v:.4g}\n" for k, v in sorted(RATIOS.items())))
            f.write("".join(f"{k} {v}\n" for k, v in sorted(COUNTS.items())))


# ---- k_pose_dist --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", eh.pose_cases(), ids=repr)
def test_pose_rmsd(h, case):
    got = h.pose_rmsd(case.x, case.res)
    r = eh.check_rmsd(got, case)
    print(case, f"error / gate {r:.3g}")
    RATIOS[f"rmsd D={case.D}"] = max(RATIOS.get(f"rmsd D={case.D}", 0.0), r)


@pytest.mark.parametrize("case", eh.pose_cases(), ids=repr)
def test_pose_mask(h, case):
    words = h.pose_mask(case.x, case.radius, case.res)
    n, b = eh.check_mask(words, case)
    g = "lattice" if case.kind == "lattice" else "generic"
    COUNTS[f"{g} pairs"] = COUNTS.get(f"{g} pairs", 0) + n
    COUNTS[f"{g} border pairs"] = COUNTS.get(f"{g} border pairs", 0) + b
    if case.kind == "planted":
        assert eh.unpack32(words, case.B)[0, case.B - 1], "the pair whose restated value equals the radius is a neighbour"
    if case.kind == "lattice":
        with np.errstate(invalid="ignore"):
            assert np.array_equal(eh.unpack32(words, case.B), case.r64 <= case.radius), "a lattice case has no border"


@pytest.mark.parametrize("case", [c for c in eh.pose_cases() if c.B >= 3], ids=repr)
def test_poisoned_poses_keep_to_themselves(h, case):
    """A pose with a NaN and one with +inf in a compared residue: row and column clear in the mask, diagonal included, and not finite in
    the matrix; every other entry has the bits of the launch without them.  The same poison outside the subset changes nothing."""
    clean_r, clean_m = h.pose_rmsd(case.x, case.res), h.pose_mask(case.x, case.radius, case.res)
    p = eh.poisoned(case, "both", True)
    got_r, got_m = h.pose_rmsd(p.x, p.res), h.pose_mask(p.x, p.radius, p.res)
    eh.check_rmsd(got_r, p)
    eh.check_mask(got_m, p)
    bad = ~p.finite
    assert bad.sum() == 2 and np.isnan(got_r[case.B // 2]).all() and np.isnan(got_r[:, case.B // 2]).all()
    assert not np.isfinite(got_r[bad]).any() and not np.isfinite(got_r[:, bad]).any()
    nb = eh.unpack32(got_m, case.B)
    assert not nb[bad].any() and not nb[:, bad].any()
    keep = np.outer(p.finite, p.finite)
    assert np.array_equal(got_r[keep].view(u32), clean_r[keep].view(u32))
    assert np.array_equal(nb[keep], eh.unpack32(clean_m, case.B)[keep])
    q = eh.poisoned(case, "both", False)
    if q is not None:
        assert h.pose_rmsd(q.x, q.res).tobytes() == clean_r.tobytes() and np.array_equal(h.pose_mask(q.x, q.radius, q.res), clean_m)


# ---- the clustering kernels on crafted masks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", eh.graph_cases(), ids=repr)
def test_leader(h, case):
    for maxc in case.limits():
        eh.check_leader(h.leader(case.mask, case.order, maxc), case, maxc)


@pytest.mark.parametrize("case", eh.graph_cases(), ids=repr)
def test_count_and_size_full(h, case):
    eh.check_count(h.count(case.mask), case)
    for maxc in case.limits():
        eh.check_size_full(h.size_full(case.mask, case.pos, case.order, maxc), case, maxc)


STEP_CASES = [c for c in eh.graph_cases() if c.B in (33, 65, 1025)] + [eh.planted_scan_case()]


@pytest.mark.parametrize("case", STEP_CASES, ids=repr)
def test_steps_one_launch_at_a_time(h, case):
    """count, then up to 12 steps, each compared with the step of the definition on the state before it; then the run is finished on the
    host's restatement and two more launches find the done flag: the first sets it, the second changes nothing."""
    cap = case.B
    st = eh.fresh_state(case.B, cap)
    st.update(h.count(case.mask))

    def launch(st):
        nxt = h.step(case.mask, case.pos, case.order, st, cap)
        eh.check_step(nxt, st, case, cap)
        return nxt

    for _ in range(12):
        if st["state"][1] or st["state"][0] >= cap:
            break
        st = launch(st)
    while not st["state"][1] and st["state"][0] < cap and eh.unpack32(st["U"][None], case.B).any():
        st = eh.restate_step(case.adj, case.pos, case.order, st)
    if st["state"][0] < cap:
        st = launch(launch(st))
        assert st["state"][1] == 1


# ---- the consensus kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", eh.contact_cases(), ids=repr)
def test_contact_bits(h, case):
    bits = h.contact_bits(case.rec, case.lig, case.cutoff)
    eh.check_contact_bits(bits, case.rec, case.lig, case.cutoff)
    got, _ = eh.host_bits(bits, case.L)
    for p, i, j, want in case.planted:
        assert got[p, i, j] == want, (p, i, j)
    COUNTS[f"contacts {case.kind}"] = COUNTS.get(f"contacts {case.kind}", 0) + int(got.sum())


@pytest.mark.parametrize("case", [c for c in eh.contact_cases() if c.kind in ("generic", "origin")], ids=repr)
def test_contact_bits_poisoned(h, case):
    """A NaN coordinate, or +inf in every atom, in one ligand residue of one pose and in one receptor residue: that column or row has no
    contact, and everything else keeps its bits."""
    clean, _ = eh.host_bits(h.contact_bits(case.rec, case.lig, case.cutoff), case.L)
    for how in ("nan", "inf"):
        for where in ("lig", "rec"):
            p = eh.contact_poisoned(case, how, where)
            bits = h.contact_bits(p.rec, p.lig, p.cutoff)
            eh.check_contact_bits(bits, p.rec, p.lig, p.cutoff)
            got, _ = eh.host_bits(bits, case.L)
            hit = np.zeros_like(clean)
            if where == "lig":
                hit[case.n - 1, :, case.L // 2] = True
            else:
                hit[:, case.R // 2, :] = True
            assert not got[hit].any() and np.array_equal(got[~hit], clean[~hit]), (how, where)


@pytest.mark.parametrize("name,cc,mem,pre", eh.count_cases(), ids=[c[0] for c in eh.count_cases()])
def test_contact_count_and_score(h, name, cc, mem, pre):
    bits, L = eh.device_bits(cc), cc.shape[2]
    got = h.contact_count(bits, mem, L, **pre)
    eh.check_contact_count(got, bits, mem, L, pre)
    eh.check_contact_score(h.contact_score(bits, got["count"], L), bits, got["count"], L)
    # accumulation over chunks: the second half of the poses on top of the first gives what the whole gives
    k = len(cc) // 2
    if k:
        first = h.contact_count(bits[:k], mem[:k], L, **pre)
        both = h.contact_count(bits[k:], mem[k:], L, **first)
        for key in ("count", "rec_count", "lig_count"):
            assert np.array_equal(both[key], got[key]), key


def test_score_sum_needs_64_bits(h):
    cc, count = eh.big_score_case()
    bits = eh.device_bits(cc)
    got = h.contact_score(bits, count, 192)
    eh.check_contact_score(got, bits, count, 192)
    assert (got["score_sum"] == 2415919104).all() and (got["n_contacts"] == 36864).all()


@pytest.mark.parametrize("case", [c for c in eh.contact_cases() if c.kind == "generic" and c.n == 3 and c.R >= 65 and c.L > 1], ids=repr)
def test_consensus_full(h, case):
    assert case.n == 3
    for mem in (np.ones(3, np.uint8), np.array([1, 0, 1], np.uint8)):
        eh.check_consensus_full(h.consensus_full(case.rec, case.lig, mem, case.cutoff), case.rec, case.lig, mem, case.cutoff)
