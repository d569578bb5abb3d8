"""The kernel harness of the distogram reduction, the restraint step and the refinement start without a GPU (tests/aux_harness.py,
tests/kernels/aux_harness.hip): the shim builds and links against the library's launchers and every refusal leaves the host guards
zero; the kernel's fp32 bin table restated in numpy decides every quarter-angstrom lattice distance as the float64 bounds do; the onehot
construction separates the 64 bins by far more than the bound; the numpy fp32 restatement of k_pair_dist_sum stays under every bound on
the GPU tests' own inputs and each of its nine seeded mutants is rejected by the comparison named for it; the references are the
package's definitions; the restated arg-min and first-crossing rules agree with the definitions on the GPU tests' inputs and their
mutants do not; the extended-precision IGSO(3) table agrees with mpmath; symmetry_ref is symmetry.evaluate, every decision of every
symmetry pose the GPU file launches has a margin above the gate that could flip it, and each of the ten seeded mutants of the restated
symmetry step is rejected by the comparison named for it."""
import math

import mpmath as mp
import numpy as np
import pytest

import aux_harness as ah
import kernel_harness as kh
from aux_harness import DG, RF, RS, SY, Out, U, f32, f64


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return ah.compile_shim(tmp_path_factory.mktemp("aux_harness"))


def test_library_exports_the_launchers():
    out = kh.exported_symbols(ah.LIBDIR + "/libdfmdock_amd.so", True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in ah.LAUNCHERS:
        assert s in syms, s


def test_shim_links(shim):
    out = kh.exported_symbols(shim, False)
    for s in ah.LAUNCHERS:
        assert s in out, s
    own = kh.exported_symbols(shim, True)
    assert "kh_run" in own and "__device_stub__" not in own, "the shim adds no kernel of its own"
    h = ah.Harness(shim)      # also checks the ctypes call record's size, RS_SMALL, RS_MAX_GROUPS and pair_dist_sum_parts
    assert h.guard >= 1024 and h.check


def refused(h, op, bufs, **scalars):
    r = h.run(op, bufs, check=False, **scalars)
    assert r["err"] == ah.HIP_INVALID_VALUE, (op, sorted(scalars))
    for k, v in bufs.items():
        if isinstance(v, Out):
            assert not r[k + "_guard"][0].any() and not r[k + "_guard"][1].any(), f"{op}: the {k} block was touched"
    return True


def test_shim_refuses_before_touching_a_device(shim):
    """Every check of the shim: hipErrorInvalidValue, and the host guards of every output stay zero - nothing was allocated, uploaded,
    launched or copied back (this runs without a GPU)."""
    h = ah.Harness(shim)
    # pair_dist_sum
    c = ah.dist_case(3, 5, 2, seed=1)
    B, R, L = 2, 3, 5
    n_part = ah.parts_of(R, L)
    good = lambda **k: dict(dict(P=c["P"], Q=c["Q"], ca4=c["ca4"], w_d=c["w_d"], ln_w=c["ln_w"], ln_b=c["ln_b"], w3f=c["w3f"],
                                 part=Out(np.float64, B * n_part * 4), res=Out(np.float64, B * 4)), **k)
    sc = dict(B=B, R=R, L=L, contact_bins=7, near_cut=12.0)
    assert h.check_only("pair_dist_sum", good(), **sc) == ah.HIP_SUCCESS
    assert refused(h, "pair_dist_sum", good(part=Out(np.float64, B * n_part * 4 - 1)), **sc)                  # a partial slot short
    assert refused(h, "pair_dist_sum", good(res=Out(np.float64, B * 4 - 1)), **sc)
    assert refused(h, "pair_dist_sum", good(part=np.zeros(B * n_part * 4)), **sc)                            # output not flagged
    assert refused(h, "pair_dist_sum", good(P=c["P"][:, :-1]), **sc)
    assert refused(h, "pair_dist_sum", good(Q=c["Q"][:1]), **sc)
    assert refused(h, "pair_dist_sum", good(ca4=c["ca4"][:, :-1]), **sc)
    assert refused(h, "pair_dist_sum", good(w3f=c["w3f"][:-1]), **sc)
    assert refused(h, "pair_dist_sum", good(ln_b=c["ln_b"][:-1]), **sc)
    for cb in (0, 64, -1):
        assert refused(h, "pair_dist_sum", good(), **dict(sc, contact_bins=cb))
    assert refused(h, "pair_dist_sum", good(), **dict(sc, L=65))                                              # more partials than `part` holds
    assert refused(h, "pair_dist_sum", good(), **dict(sc, B=0))
    assert refused(h, "pair_dist_sum", good(pair_nll=Out(f32, B * R * L - 1)), **sc)
    assert refused(h, "pair_dist_sum", good(pcontact_mean=Out(f32, R * L)), **sc)                             # the mean without pcontact
    assert refused(h, "pair_dist_sum", good(pcontact=Out(f32, B * R * L), pcontact_mean=Out(f32, R * L - 1)), **sc)

    # restraint
    rc = ah.restraint_case(9, 6, R=4, B=2, seed=2, sizes=(1, 17, 3))
    Bc = rc["B"]
    rgood = lambda **k: dict(dict(rec_pos=rc["rec_pos"], gstart=rc["gstart"], pairs=rc["pairs"], upper=rc["upper"], weight=rc["weight"], big=rc["big"],
                                  lig=rc["lig"], out=Out(f32, Bc * 8)), **k)
    rs = dict(B=Bc, R=4, L=6, G=9, n_big=len(rc["big"]), n_pairs=len(rc["pairs"]), apply=0, prep_next=0, **rc["params"])
    assert h.check_only("restraint", rgood(), **rs) == ah.HIP_SUCCESS
    bad_pairs = rc["pairs"].copy()
    bad_pairs[5, 0] = 4                                                                                     # receptor index R
    assert refused(h, "restraint", rgood(pairs=bad_pairs), **rs)
    bad_pairs = rc["pairs"].copy()
    bad_pairs[7, 1] = -1
    assert refused(h, "restraint", rgood(pairs=bad_pairs), **rs)
    gs = rc["gstart"].copy()
    gs[3] = gs[2]                                                                                           # an empty group
    assert refused(h, "restraint", rgood(gstart=gs), **rs)
    gs = rc["gstart"].copy()
    gs[-1] += 1                                                                                             # does not end at P
    assert refused(h, "restraint", rgood(gstart=gs), **rs)
    gs = rc["gstart"].copy()
    gs[0] = 1
    assert refused(h, "restraint", rgood(gstart=gs), **rs)
    assert refused(h, "restraint", rgood(big=rc["big"][:-1]), **dict(rs, n_big=len(rc["big"]) - 1))           # a large group not listed
    small = np.array([g for g in range(9) if g not in rc["big"]][:len(rc["big"])], np.int32)
    assert refused(h, "restraint", rgood(big=small), **rs)                                                  # a small group listed
    assert refused(h, "restraint", rgood(big=np.repeat(rc["big"][:1], len(rc["big"]))), **rs)                # one listed twice
    assert refused(h, "restraint", rgood(), **dict(rs, G=ah.RS_MAX_GROUPS + 1))
    assert refused(h, "restraint", rgood(upper=rc["upper"][:-1]), **rs)
    assert refused(h, "restraint", rgood(lig=rc["lig"][:1]), **rs)
    assert refused(h, "restraint", rgood(out=Out(f32, Bc * 8 - 1)), **rs)
    assert refused(h, "restraint", rgood(), **dict(rs, apply=1))                                             # apply without in / out pose and updates
    t = np.array([0.5, 0.25], f32)
    assert h.check_only("restraint", rgood(t_dev=t), step=1, n_t=2, **rs) == ah.HIP_SUCCESS
    assert refused(h, "restraint", rgood(t_dev=t), step=2, n_t=2, **rs)                                      # step outside t_dev
    assert refused(h, "restraint", rgood(t_dev=t, ctl=np.array([0, 1, 2], np.uint32)), step=0, n_t=2, **rs)  # ctl[0] - 1 wraps
    assert refused(h, "restraint", rgood(t_dev=t, ctl=np.array([3, 1, 2], np.uint32)), step=0, n_t=2, **rs)
    assert refused(h, "restraint", rgood(ctl=np.array([1, 1, 2], np.uint32)), **rs)                          # a control word without times
    assert refused(h, "restraint", rgood(), **dict(rs, prep_next=1))                                         # prep_next without its outputs
    N = 10
    assert refused(h, "restraint", rgood(prep_pos=Out(f32, Bc * N * 4), prep_ca4=Out(f32, Bc * N * 4), prep_cb4=Out(f32, Bc * N * 4 - 1)),
                   **dict(rs, prep_next=1))

    # igso3_cdf, start_pose
    assert refused(h, "igso3_cdf", dict(cdf=Out(np.float64, ah.IGSO3_N - 1)), sigma=0.5)
    assert refused(h, "igso3_cdf", dict(cdf=np.zeros(ah.IGSO3_N)), sigma=0.5)
    start = ah.start_pose_inputs(4, 3)
    cdf = np.linspace(0, 1, ah.IGSO3_N)
    sgood = lambda **k: dict(dict(start=start, cdf=cdf, lig=Out(f32, 3 * 36), tr_upd=Out(f32, 9), rot_upd=Out(f32, 9)), **k)
    ss = dict(B=3, L=4, start_bstride=36, perturb=1, sigma_r3=1.0)
    assert h.check_only("start_pose", sgood(), **ss) == ah.HIP_SUCCESS
    assert refused(h, "start_pose", sgood(start=start[:2]), **ss)                                            # [B][L][9] wanted
    assert h.check_only("start_pose", sgood(start=start[:1]), **dict(ss, start_bstride=0)) == ah.HIP_SUCCESS
    assert refused(h, "start_pose", sgood(), **dict(ss, start_bstride=35))                                   # trajectories overlap
    assert refused(h, "start_pose", sgood(cdf=cdf[:-1]), **ss)
    assert refused(h, "start_pose", sgood(cdf=None), **ss)
    assert h.check_only("start_pose", sgood(cdf=None), **dict(ss, perturb=0)) == ah.HIP_SUCCESS
    assert refused(h, "start_pose", sgood(lig=Out(f32, 3 * 36 - 1)), **ss)
    assert refused(h, "start_pose", sgood(rot_upd=Out(f32, 8)), **ss)
    assert refused(h, "start_pose", sgood(u_inj=np.zeros(2, f32)), **ss)
    assert refused(h, "start_pose", sgood(axis_inj=np.zeros((3, 2), f32)), **ss)
    assert refused(h, "start_pose", sgood(), **dict(ss, B=0))
    assert refused(h, "start_pose", sgood(), **dict(ss, L=0))


# ---- k_pair_dist_sum: the lattice, the bin table, the onehot construction ------------------------------------------------------------------
def test_bin_table_decides_every_lattice_distance():
    """The kernel's fp32 table (3.25f + step_f k)^2 equals the float64 BOUNDS^2 exactly at k = 0, 31, 62 (10.5625, 729, 2575.5625), differs
    by at most 2.2 x 2^-24 relative elsewhere, and no multiple of 1/16 lies between the two for any k (nor on either, away from those
    three): `d^2 > bound` decides every quarter-angstrom lattice distance as distogram.bin_of does.  The centres are within 3 u 51.5."""
    b2, cen = ah.bound_table_f32()
    ref = DG.BOUNDS ** 2
    exact = np.nonzero(f64(b2) == ref)[0]
    assert exact.tolist() == [0, 31, 62] and ref[[0, 31, 62]].tolist() == [10.5625, 729.0, 2575.5625]
    assert (np.abs(f64(b2) - ref) / ref).max() <= 2.2 * U
    for k in range(63):
        lo, hi = min(float(b2[k]), ref[k]), max(float(b2[k]), ref[k])
        assert math.floor(hi * 16) < math.ceil(lo * 16) or k in (0, 31, 62), k      # no sixteenth in [lo, hi]
    assert np.abs(f64(cen) - DG.CENTRES).max() <= 3 * U * 51.5
    # and end to end on the lattice: all d^2 = n / 16 up to 64^2 x 3
    n = np.arange(0, 16 * 3 * 128 * 128 + 1, dtype=np.float64) / 16.0
    got = (n.astype(f32)[:, None] > b2).sum(-1)
    assert (got == DG.bin_of(np.sqrt(n))).all()


def test_planted_pairs_and_the_unreachable_neighbours():
    """The planted vectors lie on the lattice with the exact d^2 they are named for; 729 - 1/16 and 144 - 1/16 are no sum of three squares
    of quarters (11663 and 2303 are 8 m + 7), so the neighbour below is two sixteenths away there."""
    assert ah.lattice_vector(11663) is None and ah.lattice_vector(2303) is None and 11663 % 8 == 7 and 2303 % 8 == 7
    assert ah.neighbours16(169) == (168, 170) and ah.neighbours16(11664) == (11662, 11665) and ah.neighbours16(41209) == (41208, 41210)
    assert ah.neighbours16(2304) == (2302, 2305)
    offs = dict(ah.planted_offsets())
    d2 = {k: float((v * v).sum()) for k, v in offs.items()}
    assert d2["on 3.25"] == 3.25 ** 2 and d2["on 27"] == 729.0 and d2["on 50.75"] == 50.75 ** 2 and d2["on near 12 a"] == d2["on near 12 b"] == 144.0
    assert d2["below 2304/16"] == 2302 / 16 and d2["above 2304/16"] == 2305 / 16 and d2["below 11664/16"] == 11662 / 16
    for v in offs.values():
        assert (v * 4 == np.round(v * 4)).all()
    for R, L, B in ah.DIST_SHAPES:
        ca = ah.dist_case(R, L, B, seed=1)["ca4"]
        assert np.abs(ca).max() <= 64 and (ca * 4 == np.round(ca * 4)).all()
        if L >= len(offs):
            D2 = ((f64(ca[0, 0, :3]) - f64(ca[0, R:R + len(offs), :3])) ** 2).sum(-1)
            assert D2.tolist() == list(d2.values())
            bins = DG.bin_of(np.sqrt(D2))
            assert {0, 1, 31, 32, 62, 63} <= set(bins.tolist())
            near = np.sqrt(D2) < ah.NEAR_CUT
            assert not near[3] and not near[4] and near[list(offs).index("below 2304/16")]


def test_onehot_separates_the_bins():
    """The onehot regime: the float64 logits of every pair are the same 64 values, all different, and neighbouring -log p differ by
    more than 100 times the bound of pair_nll - pair_nll names the bin."""
    c = ah.dist_cases()["onehot_33_65_1"]
    z = ah.dist_logits64(c)[0]
    assert np.abs(z - z[0, 0, 0]).max() < 1e-12
    ref = ah.dist_ref(c)
    sep = np.diff(np.sort(ah.onehot_nll(c))).min()
    assert sep > 100 * ref["b_pair_nll"].max()
    b, dist = ah.bin_from_nll(c, ref["pair_nll"])
    assert (b == ref["bin"]).all() and dist.max() < 1e-12
    assert len(set(ref["bin"].reshape(-1).tolist())) >= 60      # nearly every bin occurs


def test_w3f_is_the_comment_of_PairDArgs():
    """w3f[((ob 64 + c4) 32 + m) 4 + e] = W3[ob 32 + m][c4 4 + e] / SILU_S, one fp32 product with fl32(1 / SILU_S)."""
    rng = np.random.default_rng(0)
    W3 = rng.standard_normal((64, ah.H)).astype(f32)
    w = ah.pack_w3f(W3)
    inv = f32(1.0) / ah.SILU_S
    for ob, c4, m, e in ((0, 0, 0, 0), (1, 63, 31, 3), (0, 17, 5, 2), (1, 2, 30, 1)):
        assert w[((ob * 64 + c4) * 32 + m) * 4 + e] == W3[ob * 32 + m, c4 * 4 + e] * inv
    assert w.shape == (64 * ah.H,) and w.dtype == f32


# ---- k_pair_dist_sum: the bound has power -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dist_refs():
    cases = ah.dist_cases()
    return cases, {k: ah.dist_ref(c) for k, c in cases.items()}


def test_restatement_stays_under_every_bound(dist_refs):
    """The numpy fp32 restatement of the three kernels on EVERY case of the GPU tests: every discrete output exact, every continuous one
    under its bound, er < 0.1; and the contact_bins sweep on the small case."""
    cases, refs = dist_refs
    worst = {}
    for name, c in cases.items():
        ref = refs[name]
        assert float(ref["er"].max()) < 0.1, name
        cmp = ah.dist_compare(c, ah.dist_fp32(c), ref)
        assert cmp["n_near"] == 0 and cmp["nonfinite"] == 0 and cmp.get("bin", 0) == 0, (name, cmp)
        for k in ("pair_nll", "pcontact", "edist", "pcontact_mean", "nll", "nll_near", "exp_contacts"):
            assert cmp[k] <= 1.0, (name, k, cmp[k])
            worst[k] = max(worst.get(k, 0.0), cmp[k])
    print("restatement: largest |error| / bound", worst)
    c = cases["natural_32_5_3"]
    for cb in (1, 4, 5, 32, 33, 63):
        cmp = ah.dist_compare(c, ah.dist_fp32(c, contact_bins=cb), ah.dist_ref(c, contact_bins=cb))
        assert cmp["pcontact"] <= 1.0 and cmp["exp_contacts"] <= 1.0


# where each mutant is looked for: a case on which the named comparison must reject it
MUTANT_CASES = {"hh_logits_swapped": "onehot_33_65_1", "contact_bins_without_4hh": "natural_33_65_1", "moments_of_next_row": "natural_33_65_1",
                "count_ge": "onehot_33_65_1", "near_le": "onehot_33_65_1", "partial_in_neighbour_slot": "natural_33_129_3",
                "variance_without_2dot": "natural_33_65_1", "centres_half_step": "natural_33_65_1", "mean_over_B_minus_1": "natural_33_129_3"}


@pytest.mark.parametrize("mutant", sorted(ah.DIST_MUTANTS))
def test_every_mutant_is_rejected(dist_refs, mutant):
    """Each seeded mutant of the restatement is rejected by the comparison named in DIST_MUTANTS - a discrete one by a mismatch count,
    a continuous one by at least 4 x its bound."""
    cases, refs = dist_refs
    name, key = MUTANT_CASES[mutant], ah.DIST_MUTANTS[mutant]
    cmp = ah.dist_compare(cases[name], ah.dist_fp32(cases[name], mutant=mutant), refs[name])
    print(mutant, key, cmp[key])
    if key in ("bin", "n_near"):
        assert cmp[key] >= 1
    else:
        assert cmp[key] >= 4.0
    if mutant == "contact_bins_without_4hh":      # every contact_bins that is no multiple of 8 shows it
        c = cases["natural_32_5_3"]
        for cb in (1, 4, 5, 33, 63):
            assert ah.dist_compare(c, ah.dist_fp32(c, contact_bins=cb, mutant=mutant), ah.dist_ref(c, contact_bins=cb))["pcontact"] >= 4.0
    if mutant == "count_ge":      # exactly the pairs planted ON a bound move
        c = cases[name]
        b = ah.bin_from_nll(c, ah.dist_fp32(c, mutant=mutant)["pair_nll"])[0]
        moved = np.argwhere(b != refs[name]["bin"])
        assert set(refs[name]["bin"][tuple(moved.T)].tolist()) <= {0, 31, 62} and len(moved) >= 3


def test_references_are_the_definitions(dist_refs):
    """dist_ref's maps and pose sums are distogram.pair_maps / pose_scores / pcontact_mean of logits that are
    W3 SiLU(LayerNorm(P_r + Q_l + w_d D)) written out here once more."""
    cases, refs = dist_refs
    c, ref = cases["natural_32_5_3"], refs["natural_32_5_3"]
    R = c["R"]
    ca = f64(c["ca4"])[..., :3]
    D = np.sqrt(((ca[:, :R, None] - ca[:, None, R:]) ** 2).sum(-1))
    z = f64(c["P"])[:, :R, None] + f64(c["Q"])[:, None, R:] + f64(c["w_d"]) * D[..., None]
    mu = z.mean(-1, keepdims=True)
    y = (z - mu) / np.sqrt(((z - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * f64(c["ln_w"]) + f64(c["ln_b"])
    logits = (y / (1 + np.exp(-y))) @ f64(c["W3"]).T
    for b in range(c["B"]):
        s = DG.pose_scores(logits[b], D[b], 7, ah.NEAR_CUT)
        for k in ("pair_nll", "pcontact", "edist"):
            np.testing.assert_allclose(ref[k][b], s[k], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ref["res"][b], [s["nll"], s["nll_near"], s["n_near"], s["exp_contacts"]], rtol=1e-12)
    np.testing.assert_allclose(ref["pcontact_mean"], DG.pcontact_mean(ref["pcontact"]), rtol=0, atol=0)


# ---- k_restraint ---------------------------------------------------------------------------------------------------------------------
def all_restraint_cases():
    out = dict(ah.restraint_cases())
    out.update({"tie " + k: v for k, v in ah.tie_cases().items()})
    out.update({"nan " + k: v for k, v in ah.nan_cases().items()})
    out["ulp"] = ah.ulp_cases()[0]
    out["satisfied"] = ah.satisfied_case()
    out["batch"] = ah.restraint_case(70, 86, B=5, seed=9)
    return out


def test_restraint_cases_cover_the_paths():
    """The evaluation cases: every G and L of the issue, both centroids, groups of every size with `big` listing exactly those above 16;
    every clip decision is further from its limit than the bound of the norm, and clipped and unclipped steps of both kinds occur."""
    cases = ah.restraint_cases()
    assert {len(c["upper"]) for c in cases.values()} == {1, 255, 256, 257, 4096}
    assert {c["L"] for c in cases.values()} == {1, 85, 86, 300} and {c["all_atoms"] for c in cases.values()} == {0, 1}
    sizes = set()
    cl = []
    for c in cases.values():
        n = np.diff(c["gstart"])
        sizes |= set(n.tolist())
        assert c["big"].tolist() == np.nonzero(n > ah.RS_SMALL)[0].tolist()
        for b in range(c["B"]):
            ref = ah.restraint_ref(c, b)
            assert ref["decided"].all(), (ref["norm"], ref["limit"], ref["b_norm"])
            assert 0 < ref["n_satisfied"] < len(c["upper"]) or len(c["upper"]) == 1
            cl.append(ref["clipped"])
    assert set(ah.GROUP_SIZES) <= sizes
    cl = np.array(cl)
    assert cl.any(0).all() and (~cl).any(0).all()


def test_argmin_restatement_is_the_definition():
    """The kernel's two arg-min paths restated (serial loop; lane-strided loops + lexicographic butterfly, NaN first) give np.argmin's pair
    in every group of every case of the GPU tests - ties and NaN included."""
    for name, c in all_restraint_cases().items():
        if len(c["upper"]) > 300:
            continue
        for b in range(c["B"]):
            ref = ah.restraint_ref(c, b)
            d2, arg = ah.argmin_restated(c, b)
            np.testing.assert_array_equal(arg, ref["arg"], name)
            with np.errstate(invalid="ignore"):
                np.testing.assert_array_equal(np.sqrt(d2), ref["d"], name)


def test_argmin_mutants_are_rejected():
    """nan_dropped (the comparisons `d2 < best` alone) loses the NaN of every case but the one where it is a group's first pair - the
    NaN tests of the GPU file see a finite energy; last_tie and lane_order pick the other tied pair, whose step is far outside the bound."""
    lost = {}
    for name, c in ah.nan_cases().items():
        ref = ah.restraint_ref(c, 0)
        d2, arg = ah.argmin_restated(c, 0, "nan_dropped")
        lost[name] = bool(np.isnan(ref["d"][0]) and not np.isnan(d2[0]))
    assert lost == dict(small_first=False, small_later=True, big_first=False, big_later_lane=True, big_later_stride=True, big_last=True), lost
    ties = ah.tie_cases()
    for name, mutants in (("serial", ("last_tie",)), ("in_lane", ("last_tie",)), ("across", ("lane_order", "tie_high")), ("first_last", ("tie_high",))):
        c = ties[name]
        assert ah.restraint_ref(c, 0)["arg"][0] == c["tied"][0]
        for m in mutants:
            assert ah.argmin_restated(c, 0, m)[1][0] == c["tied"][1], (name, m)
    for name, c in ties.items():      # what the other pair would do to the step
        ref = ah.restraint_ref(c, 0)
        g = c["groups"][0]
        other = dict(c, groups=[RS.RestraintGroup((g.pairs[c["tied"][1]],), g.upper, g.weight)])
        other.update(ah.pack_groups(other["groups"], c["R"], c["L"]))
        assert (np.abs(ah.restraint_ref(other, 0)["step"] - ref["step"]) > 1e6 * ref["b_step"]).any(), name


def test_restraint_bound_is_a_few_roundings():
    """The bound of energy and step is one fp32 rounding plus float64 terms: below 1.01 u of the value on every finite case."""
    for name, c in all_restraint_cases().items():
        if name.startswith("nan"):
            continue
        ref = ah.restraint_ref(c, 0)
        assert ref["b_energy"] <= 1.01 * U * abs(ref["energy"]) + 1e-44, name
        assert (ref["b_step"] <= 1.01 * U * np.abs(ref["step"]) + 1e-13 * np.abs(ref["step"]).max() + 1e-44).all(), name


# ---- k_igso3_cdf ---------------------------------------------------------------------------------------------------------------------
def test_igso3_reference_and_gate():
    """The extended-precision table: equal to refine.igso3_cdf (float64, libm) within the gate; rows of its pdf equal to mpmath at 200
    bits to 2^-60 relative of the row's sum of |terms|; the gate is far below 1e-10 for every sigma of the GPU tests."""
    sig = ah.igso3_sigmas()
    ds = RF.discrete_sigma()
    assert sig[0] == ds.min() and sig[11] == ds.max() and sum(s in ds for s in sig) == 12 and len(sig) == 15
    gates = []
    for s in sig:
        ref, gate = ah.igso3_ref(s)
        gates.append(float(gate.max()))
        assert gate.max() < 2.5e-11 and (gate > 0).all()
    print("largest gate per sigma:", [f"{g:.2g}" for g in gates])
    for s in (sig[0], sig[5], sig[11]):
        ref, gate = ah.igso3_ref(s)
        assert (np.abs(RF.igso3_cdf(s) - ref) <= gate).all()
        coef, arg, terms, lo = ah.igso3_terms(s)
        rows = (0, 1, 137, 500, 998, 999)
        mp_pdf = ah.igso3_mp_rows(s, rows)
        e = terms.sum(1)
        om = np.asarray(RF.OMEGA, np.longdouble)
        one_m_cos = 2 * np.sin(om / 2) ** 2
        pdf = e * one_m_cos / ah.PI_LD
        for k, want in zip(rows, mp_pdf):
            hi = float(pdf[k])
            with mp.workprec(200):
                err = float(abs(mp.mpf(hi) + mp.mpf(float(pdf[k] - np.longdouble(hi))) - want))      # (the longdouble value, exactly)
            scale = float(np.abs(terms[k]).sum() * one_m_cos[k]) / np.pi
            assert err <= 2.0 ** -58 * scale, (s, k, err / scale)


def test_igso3_small_sigma_tail_is_noise():
    """At the smallest sigma of the grid the float64 definition's table is not monotone from k ~ 275 on: the tail the GPU
    test asks to be returned as summed."""
    cdf = RF.igso3_cdf(ah.igso3_sigmas()[0])
    assert (np.diff(cdf[275:]) < 0).any() and abs(1 - cdf[999]) < 1e-9


# ---- k_start_pose --------------------------------------------------------------------------------------------------------------------
def test_hand_tables_exercise_every_branch():
    """The hand-written tables: the expected index of every row is the first-crossing rule's; together the rows reach k = 0 (u below
    cdf[0], u = 0), no crossing (u = 1, all entries below), u equal to an entry, a flat stretch, a dip and a non-monotone tail; every u is an
    fp32 number; refine.inverse_cdf gives the angle of that index; the mutants `last crossing` and `>` pick another index on some row,
    and then the angle moves by at least a tenth of a table step - 10^4 times the gate of the GPU test."""
    tables = ah.hand_tables()
    dw = np.pi / ah.IGSO3_N
    seen = set()
    moved = {"last": 0, "gt": 0}
    for name, (cdf, rows) in tables.items():
        assert cdf.shape == (ah.IGSO3_N,)
        for u, k in rows:
            assert float(f32(u)) == u and ah.first_crossing(cdf, u) == k, (name, u, k)
            ang = ah.angle_of(cdf, u, k)
            assert abs(ang - float(RF.inverse_cdf(np.array([u]), cdf)[0])) <= 4 * ah.E64 * np.pi
            seen.add("none" if k is None else ("zero" if k == 0 else ("equal" if cdf[k] == u else "inside")))
            for m in moved:      # (`>` at a u equal to a single entry moves the index and not the angle: the interpolation is continuous)
                am = ah.angle_of(cdf, u, ah.first_crossing(cdf, u, m))
                if am != ang:
                    moved[m] += 1
                    assert abs(am - ang) >= 0.1 * dw, (name, u, m)
    assert seen == {"none", "zero", "equal", "inside"} and min(moved.values()) >= 1, (seen, moved)
    assert (np.diff(tables["increasing"][0]) > 0).all() and (np.diff(tables["flat"][0]) == 0).any()
    assert (np.diff(tables["dip"][0]) < 0).any() and (np.diff(tables["tail"][0][650:]) < 0).any()


def test_start_reference_is_the_definition():
    """start_ref's rotation, translation and pose are refine.forward_marginal's and refine.noise_pose's (the float32 definition) within
    the fp32 bound; the native draws restate the Philox stream of k_init_pose with stream id 4."""
    cdf = RF.igso3_cdf(RF.sigma_index(0.3)[1])
    rng = np.random.default_rng(1)
    start = ah.start_pose_inputs(40, 1)[0]
    u, axis, z = float(f32(0.37)), rng.standard_normal(3).astype(f32), rng.standard_normal(3).astype(f32)
    sig = float(RF.r3_sigma(0.3))
    for fam in (0, 1):
        rot, tr, pose, drot, dtr, dpose = ah.start_ref(start, cdf, u, axis, z, sig, fam)
        r2, t2 = RF.forward_marginal(0.3, [u], axis[None], z[None], cdf=cdf)
        np.testing.assert_allclose(rot, r2[0], rtol=1e-14)
        np.testing.assert_allclose(tr, t2[0], rtol=1e-14)
        want = RF.noise_pose(start, rot.astype(f32), tr.astype(f32), fam).reshape(-1)
        assert np.abs(pose - want).max() <= dpose
    u0, ax0, z0, dz = ah.start_draws64(2, 77)
    assert 0 < u0 < 1 and float(f32(u0)) == u0 and np.isfinite(ax0).all() and (dz < 1e-5).all()
    u1 = ah.start_draws64(3, 77)[0]
    assert u1 != u0


# ---- k_symmetry: the reference is the definition, the shim's checks, the margins of every decision, the mutants ------------------------
def all_sym_cases():
    """(name, case) of every launch of the GPU file's symmetry tests."""
    out = [(f"eval L {L} a {aa}", ah.sym_case(L, n, aa)) for L, n in ((1, 2), (21, 3), (22, 4), (85, 5), (86, 7), (300, 24)) for aa in (0, 1)]
    out += [(f"apply L {L}", ah.sym_case(L, 3, aa)) for L, aa in ((1, 0), (21, 1), (22, 0), (85, 1), (86, 0), (300, 1))]
    out += [(f"midpoints n {n}", ah.sym_midpoint_case(n)[0]) for n in sorted(ah.SYM_MIDPOINTS)]
    out.append(("batch", ah.sym_case(85, 5, 1)))
    return out


def test_symmetry_ref_is_the_definition():
    """symmetry_ref returns symmetry.evaluate's own values (on the fp32 coordinates and fp32 parameters); the restatement without a mutant
    agrees with it to float64 rounding on every pose, move included."""
    c = ah.sym_case(22, 4, 0)
    p = SY.SymmetryParams(**c["params"])
    for v in c["params"].values():
        assert float(f32(v)) == v
    for name, c in all_sym_cases():
        for b in range(c["B"]):
            ref = ah.symmetry_ref(c, b)
            with np.errstate(all="ignore"):
                ev = SY.evaluate(c["rec_pos"].reshape(-1, 3, 3), c["lig"][b].reshape(-1, 3, 3), c["n"], SY.SymmetryParams(**c["params"]),
                                 "all_atoms" if c["all_atoms"] else "ca")
            for k in ("m", "theta", "screw", "fit_rmsd", "sym_rmsd"):
                assert ref[k] == ev[k] or (np.isnan(ref[k]) and np.isnan(ev[k])), (name, b, k)
            assert np.array_equal(ref["step"], ev["step"], equal_nan=True) and np.array_equal(ref["axis_point"], ev["axis_point"], equal_nan=True)
            if not np.isfinite(c["lig"][b]).all():
                continue
            rot0, tr0 = np.array([0.3, -0.2, 0.1]), np.array([1.0, -2.0, 0.5])
            rs = ah.symmetry_restated(c, b, rot0=rot0, tr0=tr0)
            assert rs["order_m"] == ref["m"] and np.abs(rs["step"] - ref["step"]).max() <= 1e-12, (name, b)
            pose, tu, ru, *_ = ah.apply_ref(c, b, ref["step"], rot0, tr0)
            assert np.abs(rs["pose"] - pose).max() <= 1e-9 and np.abs(rs["rot_update"] - ru).max() <= 1e-12 and np.abs(rs["tr_update"] - tu).max() <= 1e-12
    last = ah.symmetry_ref(ah.sym_case(86, 3, 0), 2, last=True)
    assert np.linalg.norm(last["step"][:3]) > 10.0 and np.linalg.norm(last["step"][3:]) > 0.3      # the snapped step is not clipped


def test_symmetry_decisions_have_margins():
    """Every decision of every pose the GPU file launches is decided: the gap between the best and the second-best generator exceeds 1e-9
    rad (the theta gate is 1e-11), both clip margins exceed the bound of the step they decide (gain x the gate of screw / theta:
    1e-8 A, 1e-11 rad), and |v| is either below 1e-12 or above 1e-6 (NO_AXIS is 1e-9).  No pose is excused; the only planted boundaries
    are the exactly symmetric pose (delta = 0: a step of zero is far from the clip) and the midpoints, 1e-3 rad off."""
    n_poses = 0
    for name, c in all_sym_cases():
        p = c["params"]
        for b in range(c["B"]):
            if not np.isfinite(c["lig"][b]).all():
                continue
            ref = ah.symmetry_ref(c, b)
            assert ref["vn"] < 1e-12 or ref["vn"] > 1e-6, (name, b, ref["vn"])
            assert (ref["m"] == 0) == (ref["vn"] < 1e-12)
            assert ref["m_gap"] > 1e-9, (name, b, ref["m_gap"])
            assert ref["clip_margin"][0] > 1e3 * p["gain_tr"] * 1e-8 and ref["clip_margin"][1] > 1e3 * p["gain_rot"] * 1e-11, (name, b, ref["clip_margin"])
            n_poses += 1
    assert n_poses > 150
    for n in ah.SYM_MIDPOINTS:
        c, want = ah.sym_midpoint_case(n)
        got = [ah.symmetry_ref(c, b) for b in range(c["B"])]
        assert [g["m"] for g in got] == list(want)
        assert all(5e-4 < g["m_gap"] < 4e-3 for g in got[:-2]), [g["m_gap"] for g in got]      # 2e-3 but for the fp32 rounding of the coordinates
    for L in (22, 86):      # the zero-step poses
        import symmetry_fixtures as SF
        y = ah.sym_chain(L, seed=3)
        c = ah.sym_case_of(y, np.stack([SF.exact_translation(y), y.copy()]), 3, 0)
        assert not np.array_equal(c["lig"][0], c["lig"][1])
        for b in (0, 1):
            ref = ah.symmetry_ref(c, b)
            assert ref["vn"] < 1e-12 and ref["m"] == 0 and ref["theta"] == 0.0 and not ref["step"].any() and np.isnan(ref["screw"])


SYM_MUTANT_INPUT = {"larger_m": ("midpoints n 24", None), "no_gcd": ("midpoints n 8", None), "no_w_flip": ("batch", None),
                    "clip_under_snap": ("apply L 86", "last"), "gains_swapped": ("apply L 86", None), "centre_all_atoms": ("apply L 86", None),
                    "screw_sign": ("apply L 86", None), "compose_order": ("apply L 86", None), "last_off_by_one": ("apply L 86", "last"),
                    "last_from_num_steps": ("apply L 86", "ctl")}


@pytest.mark.parametrize("mutant", sorted(ah.SYM_MUTANTS))
def test_symmetry_mutants_are_rejected(mutant):
    """Each seeded mutant of the restatement fails the comparison named for it in SYM_MUTANTS, with the GPU file's own gate and on its
    own inputs: order_m exact; the step beyond 2 fp32 ulp; the pose and rot_update beyond apply_ref's bounds."""
    name, mode = SYM_MUTANT_INPUT[mutant]
    c = dict(all_sym_cases())[name]
    rot0, tr0 = np.array([0.3, -0.2, 0.1]), np.array([1.0, -2.0, 0.5])
    # test_symmetry_last_step's arguments: idx 3 of 4 steps; with the control words the by-value num_steps says the opposite
    kw = {None: {}, "last": dict(idx=3, num_steps=4), "ctl": dict(idx=3, num_steps=5, ctl=(4, 0, 0, 4))}[mode]
    rejected = 0
    for b in range(c["B"]):
        if not np.isfinite(c["lig"][b]).all():
            continue
        ref = ah.symmetry_ref(c, b, last=mode is not None)
        good, bad = ah.symmetry_restated(c, b, rot0=rot0, tr0=tr0, **kw), ah.symmetry_restated(c, b, mutant, rot0=rot0, tr0=tr0, **kw)
        pose, tu, ru, dpose, dtu, dru = ah.apply_ref(c, b, ref["step"], rot0, tr0)
        ulp = lambda s: np.repeat([np.spacing(f32(np.abs(s[:3]).max())), np.spacing(f32(np.abs(s[3:]).max()))], 3).astype(np.float64)

        def verdict(r):
            return {"order_m": r["order_m"] != ref["m"], "step": bool((np.abs(r["step"] - ref["step"]) > 2 * ulp(ref["step"])).any()),
                    "pose": bool((np.abs(r["pose"] - pose) > dpose).any()), "rot_update": bool((np.abs(r["rot_update"] - ru) > dru).any())}
        assert not any(verdict(good).values()), (mutant, b, verdict(good))
        rejected += verdict(bad)[ah.SYM_MUTANTS[mutant]]
    assert rejected >= 1, mutant


def test_shim_checks_of_the_symmetry_launch(shim):
    """One malformed record per condition, refused before anything is uploaded."""
    h = ah.Harness(shim)
    c = ah.sym_case(22, 3, 0)
    B, L = c["B"], 22
    good = lambda **k: dict(dict(rec_pos=c["rec_pos"], lig=Out(f32, init=c["lig"]), sym_out=Out(np.float64, B * ah.SYM_OUT), step_out=Out(f32, B * 6)), **k)
    sc = dict(B=B, R=L, L=L, all_atoms=0, n=3, apply=0, prep_next=0, snap_last=1, **{k: v for k, v in c["params"].items() if k != "snap_last"})
    assert h.check_only("symmetry", good(), **sc) == ah.HIP_SUCCESS
    assert h.check_only("symmetry", good(lig=c["lig"]), **sc) == ah.HIP_SUCCESS
    for change in (dict(R=21), dict(R=23), dict(R=0, L=0), dict(n=1), dict(n=25), dict(n=0), dict(B=0), dict(apply=2), dict(snap_last=2), dict(apply=1), dict(prep_next=1)):
        assert refused(h, "symmetry", good(), **dict(sc, **change)), change
    for bufs in (good(rec_pos=c["rec_pos"][:-1]), good(lig=Out(f32, init=c["lig"][:-1])), good(lig=Out(f32, B * L * 9)), good(sym_out=Out(np.float64, B * ah.SYM_OUT - 1)),
                 good(step_out=Out(f32, B * 6 - 1)), good(step_out=np.zeros(B * 6, f32)), good(tr_upd=Out(f32, init=np.zeros(B * 3, f32))),
                 good(ctl=np.array([1, 0, 0, 4], np.uint32))):
        assert refused(h, "symmetry", bufs, **sc)
    t = np.array([0.5, 0.25], f32)
    four = lambda a: np.array([a, 0, 0, 2], np.uint32)
    assert h.check_only("symmetry", good(t_dev=t), step=1, n_t=2, **sc) == ah.HIP_SUCCESS
    assert h.check_only("symmetry", good(t_dev=t, ctl=four(2)), step=9, n_t=2, **sc) == ah.HIP_SUCCESS
    assert refused(h, "symmetry", good(t_dev=t), step=2, n_t=2, **sc)                                         # step outside t_dev
    assert refused(h, "symmetry", good(t_dev=t, ctl=four(0)), step=0, n_t=2, **sc)                            # ctl[0] - 1 wraps
    assert refused(h, "symmetry", good(t_dev=t, ctl=four(3)), step=0, n_t=2, **sc)
    assert refused(h, "symmetry", good(t_dev=t, ctl=four(1)[:3]), step=0, n_t=2, **sc)                        # 12 bytes: k_restraint's block, not this kernel's
    assert h.check_only("restraint", dict(rec_pos=c["rec_pos"]), B=1) == ah.HIP_INVALID_VALUE
    ap = good(tr_upd=Out(f32, init=np.zeros(B * 3, f32)), rot_upd=Out(f32, init=np.zeros(B * 3, f32)))
    assert h.check_only("symmetry", ap, **dict(sc, apply=1)) == ah.HIP_SUCCESS
    assert refused(h, "symmetry", dict(ap, lig=c["lig"]), **dict(sc, apply=1))                                # apply needs the pose in / out
    N = 2 * L
    prep = dict(prep_pos=Out(f32, B * N * 4), prep_ca4=Out(f32, B * N * 4), prep_cb4=Out(f32, B * N * 4))
    assert h.check_only("symmetry", good(**prep), **dict(sc, prep_next=1)) == ah.HIP_SUCCESS
    assert refused(h, "symmetry", good(**dict(prep, prep_ca4=Out(f32, B * N * 4 - 1))), **dict(sc, prep_next=1))
    assert refused(h, "symmetry", good(**prep), **sc)                                                         # prep outputs without prep_next


def test_every_declared_launcher_is_called_by_a_shim():
    """Every launch_* that dfm_internal.h declares is called in the source of some shim under tests/kernels/: no launcher is reached
    through whole public calls only."""
    import glob
    import os
    import re
    names = set(re.findall(r"\b(launch_\w+)\s*\(", open(os.path.join(ah.LIBDIR, "csrc", "dfm_internal.h")).read()))
    src = "".join(open(f).read() for f in glob.glob(os.path.join(ah.ROOT, "tests", "kernels", "*_harness.hip")))
    assert len(names) >= 58 and {"launch_symmetry", "launch_density", "launch_density_pose"} <= names
    assert not sorted(n for n in names if not re.search(r"\b" + n + r"\s*\(", src))
