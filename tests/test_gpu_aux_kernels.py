"""The distogram reduction (k_pair_dist_sum + k_dist_finish + k_dist_mean), the restraint step (k_restraint), the symmetry step
(k_symmetry) and the refinement start (k_igso3_cdf, k_start_pose), launch by launch between guard bands against float64 computed from the same inputs, through the host shim of
tests/aux_harness.py.  Every comparison is with the float64 definition, never with another kernel or a second run.  u = 2^-24, e = 2^-53.

k_pair_dist_sum.
  Discrete outputs are exact and no pair is excused.  CA atoms sit on the quarter-angstrom lattice (|coordinate| <= 64): dx, d^2 and, at
  perfect squares, D are exact in fp32 and equal to float64; the kernel's fp32 bound table (3.25f + step_f k)^2 equals the float64
  BOUNDS^2 at k = 0, 31, 62 and has no multiple of 1/16 between itself and the float64 value elsewhere (tests/test_aux_harness_cpu.py scans
  the 63 bounds).  In the `onehot` regime every pair has the same 64 logits, all different, so pair_nll names the bin the kernel used:
  EVERY pair's bin must equal distogram.bin_of.  Planted: pairs exactly on 3.25, 27 and 50.75 A and on the near cutoff 12 A ((12, 0, 0)
  and (8, 8, 4): not near), their lattice neighbours on either side, D = 0, D > 50.75.  The neighbour below 27^2 and below 12^2 is TWO
  sixteenths away: 729 - 1/16 and 144 - 1/16 are 11663 / 16 and 2303 / 16, both of the form 8 m + 7, which no sum of three squares reaches.
  n_near is exact; a near cutoff of 0 empties the set: nll_near NaN, n_near 0, nll finite.
  Continuous outputs (aux_harness.dist_ref).  eps_z: heads_harness.pair_head_m_ref up to the projection (the same arithmetic), whose
  130 u becomes 256 u: 128 steps of v_mfma_f32_32x32x2 per accumulator, at most two roundings of the partial sum each; the packed
  operand's two roundings and the product's are the 3 u |a| term.  With E = max_o eps_z:
    softmax    |d log p_o| <= 2 E: the log-sum-exp and the logit move by at most E each
    ev_o       exp2((z_o - zm) log2 e): the difference, the constant and the product round the argument x three times (3 ln 2 |x| u
               relative on ev), exp2 within 1 ulp, a flushed denormal 2^-126:  dev_o = (3 ln 2 |x_o| + 1) u ev_o + 2^-126
    es         32 in-lane additions and the partner lane's: des = sum_o dev_o + 33 u es
    pair_nll   2 E + des / es + 4 u |log es| (logf within 2 ulp) + u |zm - z_t| + 2 u |nll|
    pcontact   p (expm1(2 E) + des / es + 2 u) + (sum_{o < bins} dev_o + 33 u sum_{o < bins} ev_o) / es       (one division)
    edist      the same with the weights centre_o, whose fp32 table is 3 u 51.5 off (the step, the product, the sum), and 34 roundings
               of the fma chain
    pose sums  the pairs' bounds added, plus n e sum |terms| with n = 16 (a lane's pairs) + 6 (butterfly) + n_part + 1
    pcontact_mean   the mean of the pairs' bounds + one fp32 rounding; and bitwise fl32(distogram.pcontact_mean(the launch's own pcontact))
  The bound is linear in er (the relative bound of rstd), checked to stay below 0.1.  Power: tests/test_aux_harness_cpu.py - an fp32
  restatement stays under every bound on every input used here, nine seeded mutants are each rejected by a named comparison.
k_restraint (aux_harness.restraint_ref).  d^2, d, v = d - u are the definition's own float64 operations in its own order
  (-ffp-contract=off), so n_satisfied, the arg-min and v are exact; energy and the six step components:
  (ceil(G / 256) + 12) e sum |terms| (the lane's fold, 6 butterfly additions, 3 wave additions, 3 roundings inside a term) + the centroid's
  summation order on the torque + 6 e for k and the clip + ONE fp32 rounding.  The clip decision is exact wherever | |k F| - max | exceeds
  the bound of the norm - on every case here (CPU file).  Arg-min ties: one group per launch whose tied pairs pull in different
  directions.  NaN: restraints.evaluate (np.argmin) is the specification - a NaN distance wins the arg-min wherever it stands.
k_symmetry (aux_harness.symmetry_ref = symmetry.evaluate on the kernel's fp32 coordinates and parameters).  No new tolerance: the
  diagnostics carry symmetry_fixtures.check_eval's gates (theta 1e-11 rad, axis 1e-10, the lengths 1e-8 A, the fp32 step 2 ulp of the step
  formed from the device's own float64 outputs), order_m is exact, the move carries apply_ref's bounds as k_restraint's does, the last step
  the sampler tests' closure gates (1e-5 rad, 1e-3 A), and everything else - prep_next against launch_prep_pose, gating, the control words
  against the by-value arguments, batch invariance, the zero step, non-finite poses - is bitwise.  The CPU file asserts that every decision
  of every pose used here (the choice of m, both clips, |v| against NO_AXIS) has a margin above the gate that could flip it.
k_igso3_cdf (aux_harness.igso3_ref): refine.igso3_cdf's formula in numpy.longdouble from the same float64 inputs; the gate counts the
  kernel's roundings term by term (c e sum |terms| with the argument's e |omega (l + 1/2)|; 1000 sequential additions; the 22-addition
  scan).  Its largest entry is 1.5e-13 at sigma = 1.5 and 1.9e-11 at sigma = 0.1 (the argument's rounding, up to 3141 x 2^-53 per term, in
  the worst case over 1000 terms and the scan): 5 to 700 times below the 1e-10 of tests/test_gpu_refine.py, which now applies it too.
k_start_pose: hand-written tables exercise every branch of the first-crossing rule; with the axis (0, 0, 1) injected rot_z is the angle,
  one fp32 rounding of a float64 a few roundings from refine.inverse_cdf: a wrong index is off by at least a tenth of a table step, five
  orders above the gate.  tr = fl32(sigma z).  The pose: the update bound of tests/test_gpu_head_kernels.py.

The largest measured |error| / bound of every test goes to $DFM_AUX_PROFILE/aux_kernels_gpu.txt when that variable names a directory
(profiles/aux_kernels.txt holds the MI355X figures).
"""
import os

import numpy as np
import pytest

import aux_harness as ah
import heads_harness as hh
import symmetry_fixtures as SF
from aux_harness import SY
from aux_harness import Out, U, bits, f32, f64

pytestmark = pytest.mark.gpu

RATIOS = {}
ALL_MAPS = ("pair_nll", "pcontact", "edist", "pcontact_mean")


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    harness = ah.Harness(ah.compile_shim(tmp_path_factory.mktemp("aux_harness_gpu")))
    yield harness
    out = os.environ.get("DFM_AUX_PROFILE")
    if out:
        with open(os.path.join(out, "aux_kernels_gpu.txt"), "w") as f:
            f.write("test max_error_over_bound\n" + "".join(f"{k} {v:.4g}\n" for k, v in sorted(RATIOS.items())))


@pytest.fixture(scope="module")
def heads(tmp_path_factory):
    return hh.Harness(hh.compile_shim(tmp_path_factory.mktemp("heads_harness_aux")))


@pytest.fixture(scope="module")
def cases():
    return ah.dist_cases()


@pytest.fixture(scope="module")
def refs(cases):
    """The float64 reference of each case at the default contact_bins / near cutoff, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ah.dist_ref(cases[name])
        return cache[name]
    return get


def record(key, worst):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(worst))


def within(name, got, ref, bound, key):
    """Every element within its bound (NaN fails); records the largest |error| / bound."""
    got, ref = f64(got), f64(ref)
    ratio = np.abs(got - ref) / np.broadcast_to(bound, ref.shape)
    worst = float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if ratio.size else 0.0
    record(key, worst)
    print(f"{name}: max |err| / bound = {worst:.3g}")
    assert worst <= 1.0, f"{name}: worst |err| / bound = {worst:.3g} at {np.argwhere(~(ratio <= 1.0))[:3].tolist()}"


def check_dist(name, c, got, ref, maps=ALL_MAPS, key=None):
    """One launch against dist_ref: every discrete output exact, every continuous one within its bound, nothing non-finite lost."""
    assert float(ref["er"][np.isfinite(ref["pair_nll"])].max()) < 0.1
    cmp = ah.dist_compare(c, got, ref, maps)
    print(name, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in cmp.items()})
    assert cmp["n_near"] == 0, f"{name}: n_near {got['res'][:, 2]} != {ref['res'][:, 2]}"
    assert cmp["nonfinite"] == 0, f"{name}: {cmp['nonfinite']} outputs are finite where the definition is not"
    assert cmp.get("bin", 0) == 0, f"{name}: {cmp.get('bin')} pairs in another bin than distogram.bin_of"
    for k in maps + ("nll", "nll_near", "exp_contacts"):
        record(f"{key or name} {k}", cmp[k])
        assert cmp[k] <= 1.0, f"{name}: {k} worst |err| / bound = {cmp[k]:.3g}"
    assert not ah.is_sentinel(got["part"].view(np.uint32)).any(), f"{name}: a partial slot was not written"
    if "pcontact_mean" in maps:
        own = ah.DG.pcontact_mean(got["pcontact"]).astype(f32)
        same = (bits(got["pcontact_mean"]) == bits(own)) | (np.isnan(got["pcontact_mean"]) & np.isnan(own))
        assert same.all(), f"{name}: pcontact_mean is not the rounded float64 mean of pcontact"


# ---- k_pair_dist_sum -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,L,B", ah.DIST_SHAPES)
def test_dist_sum_bins_exact(h, cases, refs, R, L, B):
    """The onehot regime: EVERY pair's bin equals distogram.bin_of - the pairs on 3.25 / 27 / 50.75 A, their lattice neighbours, D = 0 and
    the last bin included - n_near is exact with pairs exactly on the near cutoff, and the maps are within their bounds."""
    name = f"onehot_{R}_{L}_{B}"
    c, ref = cases[name], refs(name)
    got = h.dist_sum(c)
    b, dist = ah.bin_from_nll(c, got["pair_nll"])
    sep = np.diff(np.sort(ah.onehot_nll(c))).min()
    assert (dist < sep / 4).all(), "a pair_nll is none of the 64 known values"
    check_dist(f"k_pair_dist_sum {name}", c, got, ref, key="k_pair_dist_sum onehot")
    np.testing.assert_array_equal(b, ref["bin"])
    if L >= len(ah.planted_offsets()):
        planted = ref["bin"][0, 0, :len(ah.planted_offsets())]
        assert {0, 1, 31, 32, 62, 63} <= set(planted.tolist()), planted      # both sides of the three exact bounds


@pytest.mark.parametrize("R,L,B", ah.DIST_SHAPES)
def test_dist_sum_sizes(h, cases, refs, R, L, B):
    """Natural-scale activations at every shape: maps, pose sums and pcontact_mean against float64; the poisoned rows (ligand rows of P,
    receptor rows of Q) are never read; trajectory B - 1 alone has the bits it has in the batch."""
    name = f"natural_{R}_{L}_{B}"
    c, ref = cases[name], refs(name)
    got = h.dist_sum(c)
    check_dist(f"k_pair_dist_sum {name}", c, got, ref, key="k_pair_dist_sum sizes")
    if B > 1:
        one = h.dist_sum(c, sl=slice(B - 1, B))
        for k in ("pair_nll", "pcontact", "edist", "res"):
            assert (bits(one[k][0]) == bits(got[k][B - 1])).all(), f"{k}: a trajectory's bits depend on the batch"


@pytest.mark.parametrize("name", ["kappa_50", "kappa_2000", "spread", "wd0"])
def test_dist_sum_regimes(h, cases, refs, name):
    """Rows with a large common mean (the moment variance cancels kappa-fold), logits spread over several hundred (most exp2 underflow),
    w_d = 0."""
    c, ref = cases[name], refs(name)
    if name == "spread":
        z = ah.dist_logits64(c)[0]
        assert np.median(z.max(-1) - z.min(-1)) > 200.0
    check_dist(f"k_pair_dist_sum {name}", c, h.dist_sum(c), ref)


def test_dist_sum_contact_bins_sweep(h, cases):
    """contact_bins = 1 .. 63 on one small case of each kind; {1, 4, 5, 32, 33, 63} on the tail shapes."""
    for name in ("onehot_32_5_3", "natural_32_5_3"):
        c = cases[name]
        for cb in range(1, 64):
            got = h.dist_sum(c, maps=("pcontact",), contact_bins=cb)
            ref = ah.dist_ref(c, contact_bins=cb)
            within(f"pcontact {name} contact_bins {cb}", got["pcontact"], ref["pcontact"], ref["b_pcontact"], "k_pair_dist_sum contact_bins sweep")
            within(f"exp_contacts {name} contact_bins {cb}", got["res"][:, 3], ref["res"][:, 3], ref["b_res"][:, 3], "k_pair_dist_sum contact_bins sweep")
    for R, L, B in ah.DIST_TAIL_SHAPES:
        c = cases[f"onehot_{R}_{L}_{B}"]
        for cb in ah.TAIL_CONTACT_BINS:
            got = h.dist_sum(c, maps=("pcontact",), contact_bins=cb)
            ref = ah.dist_ref(c, contact_bins=cb)
            within(f"pcontact tail {R}x{L} contact_bins {cb}", got["pcontact"], ref["pcontact"], ref["b_pcontact"], "k_pair_dist_sum contact_bins tails")


def test_dist_sum_optional_maps(h, cases, refs):
    """Each optional map asked for alone, and none at all: the map has the bits it has in the full launch, the slots left out stay
    untouched, and the pose sums are bitwise the same either way."""
    name = "natural_33_129_3"
    c = cases[name]
    full = h.dist_sum(c)
    for maps in ((), ("pair_nll",), ("pcontact",), ("edist",), ("pcontact", "pcontact_mean")):
        got = h.dist_sum(c, maps=maps)
        assert (bits(got["res"]) == bits(full["res"])).all() and (bits(got["part"]) == bits(full["part"])).all(), maps
        for m in maps:
            assert (bits(got[m]) == bits(full[m])).all(), m


def test_dist_sum_near_cut(h, cases):
    """near_cut = 0 empties the set: nll_near is NaN, n_near 0, nll finite.  near_cut = 12 with pairs exactly on it: covered by every
    other test (n_near exact); here also one ulp above 12, which must take exactly the pairs on 12 in."""
    c = cases["onehot_33_65_1"]
    got = h.dist_sum(c, maps=(), near_cut=0.0)
    assert np.isnan(got["res"][:, 1]).all() and (got["res"][:, 2] == 0).all() and np.isfinite(got["res"][:, 0]).all()
    up = float(np.nextafter(f32(12.0), f32(13.0)))
    ref12, ref_up = ah.dist_ref(c), ah.dist_ref(c, near_cut=up)
    got_up = h.dist_sum(c, maps=(), near_cut=up)
    on = int((ref12["D"] == 12.0).sum())
    assert on >= 2 and (ref_up["res"][:, 2].sum() - ref12["res"][:, 2].sum()) == on
    np.testing.assert_array_equal(got_up["res"][:, 2], ref_up["res"][:, 2])


NONFINITE = [(v, where) for v in (np.nan, np.inf) for where in ("P", "Q", "ca_rec", "ca_lig")]


@pytest.mark.parametrize("value,where", NONFINITE)
def test_dist_sum_nonfinite(h, value, where):
    """A NaN, or a +inf, in one P row, one Q row or one CA coordinate of trajectory 1 of 3: every map entry and pose sum the float64
    definition makes non-finite is non-finite, everything it leaves finite stays within its bound, and trajectories 0 and 2 keep their
    bits."""
    c = ah.dist_case(33, 65, 3, seed=7)
    clean = h.dist_sum(c)
    r0, l0 = 32, 40      # the tail tile's only receptor residue; a ligand residue of the first chunk
    if where == "P":
        c["P"][1, r0, 17] = value
    elif where == "Q":
        c["Q"][1, 33 + l0, 200] = value
    elif where == "ca_rec":
        c["ca4"][1, r0, 1] = value
    else:
        c["ca4"][1, 33 + l0, 2] = value
    ref = ah.dist_ref(c)
    hit = ~np.isfinite(ref["pair_nll"])
    assert hit[1].any() and not hit[0].any() and not hit[2].any() and not hit.all()
    got = h.dist_sum(c)
    check_dist(f"k_pair_dist_sum {value} in {where}", c, got, ref, key="k_pair_dist_sum non-finite input")
    for b in (0, 2):
        for k in ("pair_nll", "pcontact", "edist", "res"):
            assert (bits(got[k][b]) == bits(clean[k][b])).all(), f"{k}: trajectory {b} changed"


# ---- k_restraint ---------------------------------------------------------------------------------------------------------------------
def check_eval(name, c, out, key, sl=None):
    """The evaluation outputs of every trajectory against restraints.evaluate."""
    for n, b in enumerate(range(c["B"]) if sl is None else sl):
        ref = ah.restraint_ref(c, b)
        assert ref["decided"].all(), f"{name}: the clip decision of trajectory {b} is within the bound of the norm"
        assert out[n, 1] == ref["n_satisfied"], f"{name}: n_satisfied {out[n, 1]} != {ref['n_satisfied']}"
        within(f"{name} energy [{b}]", out[n, 0], ref["energy"], ref["b_energy"], key + " energy")
        within(f"{name} step [{b}]", out[n, 2:], ref["step"], ref["b_step"], key + " step")


@pytest.fixture(scope="module")
def rcases():
    return ah.restraint_cases()


@pytest.mark.parametrize("G,L,all_atoms", ah.RESTRAINT_SHAPES)
def test_restraint_eval(h, rcases, G, L, all_atoms):
    """Evaluation mode against restraints.evaluate: n_satisfied exact, energy and step within a few float64 roundings of the sums plus
    one fp32 rounding; the pose is an input and nothing else is written.  Group sizes 1, 16, 17, 63, 64, 65, 200."""
    c = rcases[f"G{G}_L{L}_a{all_atoms}"]
    r = h.restraint(c)
    check_eval(f"k_restraint G {G} L {L} all_atoms {all_atoms}", c, r["out"], "k_restraint eval")
    clipped = [ah.restraint_ref(c, b)["clipped"] for b in range(c["B"])]
    print("clipped:", clipped)


@pytest.mark.parametrize("name", ["serial", "in_lane", "across", "first_last"])
def test_restraint_ties(h, name):
    """Exact ties at the minimum: the first pair in list order wins - in the serial loop, inside one lane, across lanes (the lower pair
    index, not the lower lane) and between the first and the last pair of a 200-pair group."""
    c = ah.tie_cases()[name]
    ref = ah.restraint_ref(c, 0)
    assert ref["arg"][0] == c["tied"][0]
    r = h.restraint(c)
    check_eval(f"k_restraint tie {name}", c, r["out"], "k_restraint ties")
    # the other tied pair would give a step far outside the bound
    other = dict(c, groups=[ah.RS.RestraintGroup((c["groups"][0].pairs[c["tied"][1]],), c["groups"][0].upper, c["groups"][0].weight)])
    other.update(ah.pack_groups(other["groups"], c["R"], c["L"]))
    alt = ah.restraint_ref(other, 0)
    assert (np.abs(alt["step"] - ref["step"]) > 1e6 * ref["b_step"]).any()


def test_restraint_ulp_of_upper(h):
    """d exactly `upper` and one fp32 ulp below: satisfied; one ulp above: violated by 2^-21 A; d = 0; weight 0."""
    c, names = ah.ulp_cases()
    ref = ah.restraint_ref(c, 0)
    assert ref["n_satisfied"] == 3 and 0 < ref["energy"] < 10.0
    r = h.restraint(c)
    check_eval("k_restraint ulp", c, r["out"], "k_restraint ulp of upper")
    for k, nm in enumerate(names):      # one group per launch: each decision on its own
        one = dict(c, groups=[c["groups"][k]])
        one.update(ah.pack_groups(one["groups"], c["R"], c["L"]))
        o = h.restraint(one)["out"]
        e = ah.restraint_ref(one, 0)
        assert o[0, 1] == e["n_satisfied"], nm
        within(f"k_restraint {nm}", o[0, 0], e["energy"], e["b_energy"], "k_restraint ulp of upper")


def run_apply(h, c, rot0, tr0, **kw):
    r = h.restraint(c, apply=1, rot0=rot0, tr0=tr0, **kw)
    B = r["lig"].size // (c["L"] * 9)
    return r, r["lig"].reshape(B, -1), r["tr_upd"].reshape(B, 3), r["rot_upd"].reshape(B, 3)


@pytest.mark.parametrize("G,L,all_atoms", [(1, 1, 0), (255, 85, 1), (256, 86, 0), (257, 300, 1)])
def test_restraint_apply_and_prep(h, heads, rcases, G, L, all_atoms):
    """Apply mode: the moved pose, tr_update and the composed rot_update (which starts non-zero) against float64 with the heads tests'
    update bound; `out` as in evaluation mode; prep_next writes the bits launch_prep_pose writes for the moved pose."""
    c = rcases[f"G{G}_L{L}_a{all_atoms}"]
    B, R = c["B"], c["R"]
    N = R + L
    rng = np.random.default_rng(G)
    rot0 = np.array([[0.3, -0.2, 0.5], [0.0, 0.0, 0.0]], f32)[:B]
    tr0 = (rng.standard_normal((B, 3)) * 3).astype(f32)
    r, lig, tu, ru = run_apply(h, c, rot0, tr0, prep=True)
    check_eval(f"k_restraint apply G {G}", c, r["out"], "k_restraint eval")
    moved = False
    for b in range(B):
        ref = ah.restraint_ref(c, b)
        pose, tur, rur, dpose, dtu, dru = ah.apply_ref(c, b, ref["step"], rot0[b], tr0[b])
        moved = moved or bool(np.any(ref["step"] != 0))
        within(f"k_restraint pose [{b}]", lig[b], pose, dpose, "k_restraint apply pose")
        within(f"k_restraint tr_update [{b}]", tu[b], tur, dtu, "k_restraint apply tr_update")
        within(f"k_restraint rot_update [{b}]", ru[b], rur, dru, "k_restraint apply rot_update")
    assert moved
    pp = heads.run("prep_pose", dict(rec_pos=c["rec_pos"], lig=lig, prep_pos=Out(f32, B * N * 4), prep_ca4=Out(f32, B * N * 4),
                                     prep_cb4=Out(f32, B * N * 4)), B=B, R=R, L=L, all_atoms=all_atoms)
    assert pp["err"] == hh.HIP_SUCCESS
    for k in ("prep_pos", "prep_ca4", "prep_cb4"):
        assert not ah.is_sentinel(r[k]).any() and (bits(r[k]) == bits(pp[k])).all(), k


def test_restraint_all_satisfied(h):
    """Every group satisfied: energy 0, a zero step, `moves` false - the pose and the updates keep their bits under apply."""
    c = ah.satisfied_case()
    rot0, tr0 = np.full((c["B"], 3), 0.25, f32), np.full((c["B"], 3), -1.5, f32)
    r, lig, tu, ru = run_apply(h, c, rot0, tr0)
    assert (r["out"][:, 0] == 0).all() and (r["out"][:, 1] == len(c["groups"])).all() and (r["out"][:, 2:] == 0).all()
    assert (bits(lig) == bits(c["lig"].reshape(c["B"], -1))).all() and (bits(tu) == bits(tr0)).all() and (bits(ru) == bits(rot0)).all()


@pytest.mark.parametrize("via", ["step", "ctl"])
def test_restraint_gating(h, heads, rcases, via):
    """t_dev with `step`, and with the control word (index ctl[0] - 1; the by-value step then points at a NaN time): times above, equal
    to and below t_start.  Gated off: pose, updates and `out` keep their bits - and prep_next still prepares the (unmoved) pose."""
    c = dict(rcases["G256_L86_a0"])
    c["params"] = dict(c["params"], t_start=float(f32(0.4)))
    B, R, L = c["B"], c["R"], c["L"]
    N = R + L
    t = np.array([np.nan, np.nextafter(f32(0.4), f32(1)), f32(0.4), f32(0.1), np.nan], f32)
    rot0, tr0 = np.full((B, 3), 0.125, f32), np.full((B, 3), 2.0, f32)
    free, lig_free, tu_free, ru_free = run_apply(h, c, rot0, tr0, prep=True)
    pp = heads.run("prep_pose", dict(rec_pos=c["rec_pos"], lig=c["lig"], prep_pos=Out(f32, B * N * 4), prep_ca4=Out(f32, B * N * 4),
                                     prep_cb4=Out(f32, B * N * 4)), B=B, R=R, L=L, all_atoms=0)
    for idx, runs in ((1, False), (2, True), (3, True)):
        kw = dict(t_dev=t, step=idx) if via == "step" else dict(t_dev=t, step=0, ctl=np.array([idx + 1, 7, 9], np.uint32))
        r, lig, tu, ru = run_apply(h, c, rot0, tr0, prep=True, **kw)
        if runs:
            for a, b_ in ((lig, lig_free), (tu, tu_free), (ru, ru_free), (r["out"], free["out"]), (r["prep_ca4"], free["prep_ca4"])):
                assert (bits(a) == bits(b_)).all(), (via, idx)
        else:
            assert (bits(lig) == bits(c["lig"].reshape(B, -1))).all() and (bits(tu) == bits(tr0)).all() and (bits(ru) == bits(rot0)).all()
            assert ah.is_sentinel(r["out"]).all(), "a gated-off launch wrote `out`"
            for k in ("prep_pos", "prep_ca4", "prep_cb4"):
                assert (bits(r[k]) == bits(pp[k])).all(), k


def test_restraint_batch_invariance(h):
    """Trajectory b of B = 5 has the bits of the same pose alone: pose, updates, out."""
    c = ah.restraint_case(70, 86, B=5, seed=9)
    rot0, tr0 = np.zeros((5, 3), f32), np.zeros((5, 3), f32)
    r, lig, tu, ru = run_apply(h, c, rot0, tr0)
    for b in (0, 3, 4):
        r1, lig1, tu1, ru1 = run_apply(h, c, rot0[b:b + 1], tr0[b:b + 1], sl=slice(b, b + 1))
        for a, b_ in ((lig1[0], lig[b]), (tu1[0], tu[b]), (ru1[0], ru[b]), (r1["out"][0], r["out"][b])):
            assert (bits(a) == bits(b_)).all(), b


@pytest.mark.parametrize("name", ["small_first", "small_later", "big_first", "big_later_lane", "big_later_stride", "big_last"])
def test_restraint_nan_wins_the_argmin(h, name):
    """A NaN ligand CA as the first pair of its group, and as a later one (a later position of the serial loop; a later lane and a
    later stride of the same lane in a wave's group): restraints.evaluate's np.argmin keeps it, so the energy and the step are NaN and
    the group is not satisfied.  The finite trajectory next to it is unaffected."""
    c = ah.nan_cases()[name]
    ref = ah.restraint_ref(c, 0)
    assert np.isnan(ref["energy"]) and np.isnan(ref["step"]).all() and np.isnan(ref["d"][0])
    r = h.restraint(c)
    assert np.isnan(r["out"][0, 0]), f"{name}: the NaN pair lost the arg-min: energy {r['out'][0, 0]}"
    assert np.isnan(r["out"][0, 2:]).all() and r["out"][0, 1] == ref["n_satisfied"]
    check_eval(f"k_restraint {name} (finite trajectory)", c, r["out"][1:], "k_restraint eval", sl=[1])


# ---- k_igso3_cdf ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(ah.igso3_sigmas())))
def test_igso3_cdf(h, n):
    """The table against refine.igso3_cdf's formula in extended precision under the derived gate; the 24 threads past the table write
    nothing."""
    sigma = ah.igso3_sigmas()[n]
    cdf = h.igso3(sigma)
    assert ah.is_sentinel(cdf[ah.IGSO3_N:].view(np.uint32)).all(), "an entry past the table was written"
    ref, gate = ah.igso3_ref(sigma)
    assert gate.max() < 2.5e-11
    within(f"k_igso3_cdf sigma {sigma:.6g} (largest gate {gate.max():.3g})", cdf[:ah.IGSO3_N], ref, gate, "k_igso3_cdf")
    within(f"k_igso3_cdf sigma {sigma:.6g} cdf[999]", cdf[999], ref[999], gate[999], "k_igso3_cdf last entry")


def test_igso3_cdf_tail_not_smoothed(h):
    """At the smallest sigma the pdf is rounding noise from k ~ 275 on: the table's tail is returned as summed - within the gate of the
    reference and NOT its own running maximum (no clamping, no monotone repair)."""
    sigma = ah.igso3_sigmas()[0]
    cdf = h.igso3(sigma)[:ah.IGSO3_N]
    ref, gate = ah.igso3_ref(sigma)
    within("k_igso3_cdf tail", cdf[300:], ref[300:], gate[300:], "k_igso3_cdf")
    assert abs(1.0 - cdf[999]) < 1e-9
    assert (np.diff(cdf[300:]) < 0).any(), "the tail is monotone: smoothed?"


# ---- k_start_pose --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["increasing", "flat", "dip", "tail", "all_below", "first_above"])
def test_start_pose_first_crossing(h, table):
    """Hand-written tables, evaluation mode, the axis (0, 0, 1) injected: rot_update = (0, 0, fl32(angle)) with the angle of the FIRST
    crossing - u below cdf[0], above every entry, equal to an entry, 0 and 1, on a flat stretch, across a dip and a non-monotone tail -
    and tr_update = fl32(sigma z)."""
    cdf, rows = ah.hand_tables()[table]
    B = len(rows)
    u = np.array([r[0] for r in rows], f32)
    axis = np.tile(f32([0, 0, 1]), (B, 1))
    z = np.random.default_rng(3).standard_normal((B, 3)).astype(f32)
    sigma = 1.7320508
    start = ah.start_pose_inputs(5, 1)[0]
    r = h.start(start, cdf, B, 5, 0, u=u, axis=axis, tr=z, sigma_r3=sigma, pose=False)
    for b, (ub, k) in enumerate(rows):
        assert ah.first_crossing(cdf, ub) == k
        ang = float(ah.RF.inverse_cdf(np.array([ub]), cdf)[0])
        assert (r["rot_upd"][b, :2] == 0).all()
        within(f"k_start_pose {table} u {ub:.6g}", r["rot_upd"][b, 2], ang, ang * (U + 8 * ah.E64), "k_start_pose angle")
    assert (bits(r["tr_upd"]) == bits((sigma * f64(z)).astype(f32))).all(), "tr_update is not fl32(sigma z)"


@pytest.mark.parametrize("L,B,all_atoms,strided", [(1, 1, 0, 0), (86, 5, 1, 1), (300, 5, 0, 0), (86, 1, 0, 1), (300, 5, 1, 1)])
def test_start_pose_modes(h, L, B, all_atoms, strided):
    """A real table: the pose, rot_update and tr_update with injected draws against float64; the evaluation mode returns the same
    updates and writes nothing else; perturb = 0 copies the pose bit for bit with zero updates; start_bstride 0 and L * 9."""
    cdf = ah.igso3_ref(ah.igso3_sigmas()[5])[0]
    rng = np.random.default_rng([L, B])
    start = ah.start_pose_inputs(L, B if strided else 1, seed=1)
    u, axis, z = rng.uniform(0.01, 0.99, B).astype(f32), rng.standard_normal((B, 3)).astype(f32), rng.standard_normal((B, 3)).astype(f32)
    sigma = 2.5
    args = dict(B=B, L=L, bstride=L * 9 if strided else 0, all_atoms=all_atoms, sigma_r3=sigma)
    r = h.start(start, cdf, u=u, axis=axis, tr=z, **args)
    for b in range(B):
        rot, tr, pose, drot, dtr, dpose = ah.start_ref(start[b if strided else 0], cdf, float(u[b]), axis[b], z[b], sigma, all_atoms)
        within(f"k_start_pose rot [{b}]", r["rot_upd"][b], rot, drot, "k_start_pose rot_update")
        within(f"k_start_pose tr [{b}]", r["tr_upd"][b], tr, dtr, "k_start_pose tr_update")
        within(f"k_start_pose pose [{b}]", r["lig"][b], pose, dpose, "k_start_pose pose")
    ev = h.start(start, cdf, u=u, axis=axis, tr=z, pose=False, **args)
    assert (bits(ev["rot_upd"]) == bits(r["rot_upd"])).all() and (bits(ev["tr_upd"]) == bits(r["tr_upd"])).all()
    cp = h.start(start, None, perturb=0, **args)
    src = np.broadcast_to(start.reshape(-1, L * 9), (B, L * 9)) if not strided else start.reshape(B, L * 9)
    assert (bits(cp["lig"]) == bits(np.ascontiguousarray(src))).all(), "perturb = 0 is not a copy"
    assert (bits(cp["rot_upd"]) == 0).all() and (bits(cp["tr_upd"]) == 0).all(), "perturb = 0: the updates are not +0"


def test_start_pose_native_draws(h):
    """No injection: the draws are Philox stream RNG_START of (trajectory, seed) - u exactly, the normals within the bound of the
    device's logf / cosf - and an injected zero axis gives NaN updates for that trajectory only."""
    cdf = ah.igso3_ref(ah.igso3_sigmas()[5])[0]
    B, L, seed, sigma = 5, 86, 0x1234567890, 3.0
    start = ah.start_pose_inputs(L, 1, seed=2)
    r = h.start(start, cdf, B, L, 0, sigma_r3=sigma, seed=seed)
    for b in range(B):
        u, axis, z, dz = ah.start_draws64(b, seed)
        rot, tr, pose, drot, dtr, dpose = ah.start_ref(start[0], cdf, u, axis, z, sigma, 0, daxis=dz[:3], dz=dz[3:])
        within(f"k_start_pose native rot [{b}]", r["rot_upd"][b], rot, drot, "k_start_pose native draws")
        within(f"k_start_pose native tr [{b}]", r["tr_upd"][b], tr, dtr, "k_start_pose native draws")
        within(f"k_start_pose native pose [{b}]", r["lig"][b], pose, dpose, "k_start_pose native draws")
    other = h.start(start, cdf, B, L, 0, sigma_r3=sigma, seed=seed + 1)
    assert (bits(other["rot_upd"]) != bits(r["rot_upd"])).any()
    axis = np.random.default_rng(5).standard_normal((B, 3)).astype(f32)
    axis[2] = 0
    zr = h.start(start, cdf, B, L, 0, sigma_r3=sigma, seed=seed, axis=axis)
    assert np.isnan(zr["rot_upd"][2]).all() and np.isnan(zr["lig"][2]).all()
    keep = [0, 1, 3, 4]
    assert np.isfinite(zr["rot_upd"][keep]).all() and np.isfinite(zr["lig"][keep]).all() and np.isfinite(zr["tr_upd"]).all()


# ---- k_symmetry ----------------------------------------------------------------------------------------------------------------------
SYM_GATES = dict(theta=1e-11, axis=1e-10, screw=1e-8, axis_point=1e-8, fit_rmsd=1e-8, sym_rmsd=1e-8)      # symmetry_fixtures.check_eval's own
SYM_ORDER_OF = {1: 2, 21: 3, 22: 4, 85: 5, 86: 7, 300: 24}


def sym_check_eval(name, c, ev, key="k_symmetry eval", sl=None):
    """symmetry_fixtures.check_eval, unchanged gates, on the evaluation outputs of a launch; records worst / gate of each."""
    lig = c["lig"] if sl is None else c["lig"][sl]
    worst, clipped = SF.check_eval(ev, c["rec_pos"].reshape(-1, 3, 3), lig.reshape(len(lig), -1, 3, 3), c["n"], ah.sym_p32(c),
                                   "all_atoms" if c["all_atoms"] else "ca")
    print(name, {k: f"{v:.3g}" for k, v in worst.items()})
    for k, gate in SYM_GATES.items():
        record(f"{key} {k}", worst[k] / gate)
    record(f"{key} step (gate 2 ulp)", worst["step_ulp"] / 2.0)
    return clipped


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def prep_of(heads, c, lig):
    B, L = len(lig), c["L"]
    N = 2 * L
    pp = heads.run("prep_pose", dict(rec_pos=c["rec_pos"], lig=np.ascontiguousarray(lig, f32), prep_pos=Out(f32, B * N * 4), prep_ca4=Out(f32, B * N * 4),
                                     prep_cb4=Out(f32, B * N * 4)), B=B, R=L, L=L, all_atoms=c["all_atoms"])
    assert pp["err"] == hh.HIP_SUCCESS
    return pp


def start_updates(B, seed):
    rng = np.random.default_rng([41, seed])
    return (rng.standard_normal((B, 3)) * 0.3).astype(f32), (rng.standard_normal((B, 3)) * 3).astype(f32)


@pytest.mark.parametrize("all_atoms", [0, 1])
@pytest.mark.parametrize("L", ah.SYM_SIZES)
def test_symmetry_eval(h, L, all_atoms):
    """Evaluation mode against symmetry.evaluate on the special poses of symmetry_fixtures.poses, at 3, 63, 66, 255, 258 and 900 atoms:
    order_m exact, the diagnostics within check_eval's gates, the fp32 step within 2 ulp of the step formed from the device's own float64
    outputs; the pose is an input and keeps its bits; step_out alone, out alone and both together give the same bits."""
    c = ah.sym_case(L, SYM_ORDER_OF[L], all_atoms)
    r = h.symmetry(c)
    assert same_bits(r["lig"], c["lig"].reshape(c["B"], -1)), "the evaluation mode wrote the pose"
    clipped = sym_check_eval(f"k_symmetry eval L {L} all_atoms {all_atoms}", c, r["ev"])
    assert clipped[2][0] and not clipped[3].any() and r["ev"]["order_m"][4] == 0 and r["ev"]["order_m"][5] == 0
    only_out, only_step = h.symmetry(c, step_out=False), h.symmetry(c, out=False)
    assert same_bits(only_out["sym_out"], r["sym_out"]) and same_bits(only_step["step_out"], r["step_out"])
    assert not ah.is_sentinel(r["step_out"]).any() and not ah.is_sentinel(r["sym_out"][:, :11].view(np.uint32)).any()


@pytest.mark.parametrize("n", sorted(ah.SYM_MIDPOINTS))
def test_symmetry_nearest_generator(h, n):
    """Poses 1e-3 rad either side of the midpoint between neighbouring generators (n = 5: m 1|2, 8: 1|3, 12: 1|5, 24: 1|5, 5|7, 7|11), one
    below the first generator and one above the last: order_m is exactly the expected m, and everything else is within the gates."""
    c, want = ah.sym_midpoint_case(n)
    r = h.symmetry(c)
    assert r["ev"]["order_m"].tolist() == list(want)
    sym_check_eval(f"k_symmetry midpoints n {n}", c, r["ev"], key="k_symmetry midpoints")


@pytest.mark.parametrize("L,all_atoms", [(1, 0), (21, 1), (22, 0), (85, 1), (86, 0), (300, 1)])
def test_symmetry_apply_and_prep(h, heads, L, all_atoms):
    """Apply mode from a non-zero rot_update / tr_update: the moved pose, tr_update and the composed rot_update against apply_ref of the
    DEFINITION's step within apply_ref's bounds (the restraint and heads tests' update bound); `out` as in evaluation mode; the NaN pose
    gets a NaN pose and NaN updates, the pose without an axis keeps its bits; prep_next writes the bits launch_prep_pose writes for the
    moved pose and leaves no sentinel."""
    c = ah.sym_case(L, 3, all_atoms)
    B = c["B"]
    rot0, tr0 = start_updates(B, L)
    r = h.symmetry(c, apply=1, prep=True, rot0=rot0, tr0=tr0)
    sym_check_eval(f"k_symmetry apply L {L}", c, r["ev"])
    moved = 0
    for b in range(B):
        ref = ah.symmetry_ref(c, b)
        if b == 5:
            assert np.isnan(r["lig"][b]).all() and np.isnan(r["tr_upd"][b]).all() and np.isnan(r["rot_upd"][b]).all()
            continue
        pose, tur, rur, dpose, dtu, dru = ah.apply_ref(c, b, ref["step"], rot0[b], tr0[b])
        moved += bool(np.any(ref["step"] != 0))
        within(f"k_symmetry pose [{b}]", r["lig"][b], pose, dpose, "k_symmetry apply pose")
        within(f"k_symmetry tr_update [{b}]", r["tr_upd"][b], tur, dtu, "k_symmetry apply tr_update")
        within(f"k_symmetry rot_update [{b}]", r["rot_upd"][b], rur, dru, "k_symmetry apply rot_update")
    assert moved >= 5
    assert same_bits(r["lig"][4], c["lig"][4].reshape(-1)) and same_bits(r["tr_upd"][4], tr0[4]) and same_bits(r["rot_upd"][4], rot0[4])
    pp = prep_of(heads, c, r["lig"])
    for k in ("prep_pos", "prep_ca4", "prep_cb4"):
        assert not ah.is_sentinel(r[k]).any(), k
        assert ((bits(r[k]) == bits(pp[k])) | (np.isnan(r[k]) & np.isnan(pp[k]))).all(), k
        fin = np.isfinite(pp[k])
        assert fin.mean() > 0.8 and (bits(r[k])[fin] == bits(pp[k])[fin]).all(), k


@pytest.mark.parametrize("L,all_atoms", [(22, 0), (86, 1)])
def test_symmetry_zero_step(h, L, all_atoms):
    """A translation that fp32 holds exactly, and a pose bitwise equal to the receptor: no axis.  m = 0, theta = 0, a zero step, NaN where
    the definition says NaN; under apply the pose and both updates keep their bits."""
    y = ah.sym_chain(L, seed=3)
    c = ah.sym_case_of(y, np.stack([SF.exact_translation(y), y.copy()]), 3, all_atoms)
    assert not same_bits(c["lig"][0], c["lig"][1])
    rot0, tr0 = start_updates(2, 7)
    r = h.symmetry(c, apply=1, rot0=rot0, tr0=tr0)
    sym_check_eval(f"k_symmetry zero step L {L}", c, r["ev"], key="k_symmetry zero step")
    ev = r["ev"]
    assert (ev["order_m"] == 0).all() and (ev["theta"] == 0).all() and (bits(r["step_out"]) == 0).all()
    assert np.isnan(ev["screw"]).all() and np.isnan(ev["axis"]).all() and np.isnan(ev["axis_point"]).all() and np.isnan(ev["sym_rmsd"]).all()
    assert (ev["fit_rmsd"] <= 1e-12).all()
    assert same_bits(r["lig"], c["lig"].reshape(2, -1)) and same_bits(r["tr_upd"], tr0) and same_bits(r["rot_upd"], rot0)


@pytest.mark.parametrize("via", ["step", "ctl"])
def test_symmetry_gating(h, heads, via):
    """t_dev with the by-value `step`, and with the control words (index ctl[0] - 1; the by-value step then points at a NaN time): times
    just above, equal to and below t_start.  Gated off: the pose, the updates, `out` and `step_out` keep their bits or sentinels and prep_*
    equals launch_prep_pose of the UNMOVED pose.  Gated on: bitwise the launch without t_dev."""
    c = dict(ah.sym_case(86, 3, 0))
    c["params"] = dict(c["params"], t_start=float(f32(0.4)))
    B = c["B"]
    t = np.array([np.nan, np.nextafter(f32(0.4), f32(1)), f32(0.4), f32(0.1), np.nan], f32)
    rot0, tr0 = start_updates(B, 11)
    free = h.symmetry(c, apply=1, prep=True, rot0=rot0, tr0=tr0)
    assert not same_bits(free["lig"], c["lig"].reshape(B, -1))
    pp = prep_of(heads, c, c["lig"])
    keys = ("lig", "tr_upd", "rot_upd", "sym_out", "step_out", "prep_pos", "prep_ca4", "prep_cb4")
    for idx, runs in ((1, False), (2, True), (3, True)):
        kw = dict(t_dev=t, step=idx, num_steps=99) if via == "step" else dict(t_dev=t, step=4 * (idx % 2), num_steps=idx + 1,
                                                                              ctl=np.array([idx + 1, 7, 9, 99], np.uint32))
        r = h.symmetry(c, apply=1, prep=True, rot0=rot0, tr0=tr0, **kw)
        if runs:
            for k in keys:
                assert same_bits(r[k], free[k]), (via, idx, k)
        else:
            assert same_bits(r["lig"], c["lig"].reshape(B, -1)) and same_bits(r["tr_upd"], tr0) and same_bits(r["rot_upd"], rot0)
            assert ah.is_sentinel(r["step_out"]).all() and ah.is_sentinel(r["sym_out"].view(np.uint32)).all(), "a gated-off launch wrote its outputs"
            for k in ("prep_pos", "prep_ca4", "prep_cb4"):
                assert ((bits(r[k]) == bits(pp[k])) | (np.isnan(r[k]) & np.isnan(pp[k]))).all(), k


@pytest.mark.parametrize("via", ["step", "ctl"])
def test_symmetry_last_step(h, via):
    """snap_last = 1 at idx + 1 == num_steps: step_out is the unclipped full projection (within 2 ulp of device_step with gains 1 and no
    clip) on a case whose ordinary step clips, and the moved pose, evaluated by the float64 definition, has |theta - theta*| <= 1e-5 and
    closure <= 1e-3 A (the sampler tests' gates).  One step earlier, and with snap_last = 0, the step follows the gains: bitwise the launch
    without t_dev.  With the control words, the by-value num_steps contradicts ctl[3] in both directions."""
    c = ah.sym_case(86, 3, 0)
    B, n = c["B"], c["n"]
    y = c["rec_pos"].reshape(-1, 3, 3)
    t = np.full(6, 0.5, f32)
    idx, S = 3, 4
    rot0, tr0 = start_updates(B, 13)

    def run(snap, last):
        cc = dict(c, params=dict(c["params"], snap_last=snap))
        if via == "step":
            kw = dict(t_dev=t, step=idx, num_steps=S if last else S + 1)
        else:      # the by-value arguments say the opposite of the control words
            kw = dict(t_dev=t, step=(0 if last else S - 1), num_steps=(S + 1 if last else S), ctl=np.array([idx + 1, 0, 0, S if last else S + 1], np.uint32))
        return h.symmetry(cc, apply=1, rot0=rot0, tr0=tr0, **kw)
    plain = h.symmetry(c, apply=1, rot0=rot0, tr0=tr0)
    assert ah.symmetry_ref(c, 2)["clipped"].all(), "the case must clip without snap"
    for snap, last in ((1, False), (0, True), (0, False)):
        r = run(snap, last)
        for k in ("lig", "tr_upd", "rot_upd", "sym_out", "step_out"):
            assert same_bits(r[k], plain[k]), (via, snap, last, k)
    r = run(1, True)
    assert same_bits(r["sym_out"], plain["sym_out"])
    full = SY.SymmetryParams(gain_rot=1.0, gain_tr=1.0, max_rot=1e30, max_tr=1e30, snap_last=1)
    worst = 0.0
    for b in range(B):
        if b == 5:
            assert np.isnan(r["step_out"][b]).all()
            continue
        want = SF.device_step(r["ev"], b, n, full)
        for hh_ in (0, 1):
            w3 = want[hh_ * 3:hh_ * 3 + 3]
            ulp = SF.ulp32(np.abs(w3).max()) if np.abs(w3).max() > 0 else 2.0 ** -149
            dev = float(np.abs(f64(r["step_out"][b, hh_ * 3:hh_ * 3 + 3]) - w3).max())
            worst = max(worst, dev / ulp)
            assert dev <= 2 * ulp, (b, hh_, dev, ulp)
        if b == 4:
            continue
        closure, dtheta, screw = SF.closure(y, r["lig"][b].reshape(-1, 3, 3), n)
        print(f"k_symmetry last step [{b}]: closure {closure:.3g} A, |theta - theta*| {dtheta:.3g}, screw {screw:.3g}")
        record("k_symmetry last step closure (gate 1e-3 A)", closure / 1e-3)
        record("k_symmetry last step theta (gate 1e-5 rad)", dtheta / 1e-5)
        assert dtheta <= 1e-5 and closure <= 1e-3, (b, dtheta, closure)
    record("k_symmetry last step step_out (gate 2 ulp)", worst / 2.0)
    assert np.linalg.norm(r["step_out"][2, :3]) > c["params"]["max_tr"] and np.linalg.norm(r["step_out"][2, 3:]) > c["params"]["max_rot"]


def test_symmetry_batch_invariance(h, heads):
    """Trajectory b of B = 5 has the bits of the same pose alone: pose, updates, out, step_out, prep_*."""
    c = ah.sym_case(85, 5, 1)
    rot0, tr0 = start_updates(5, 17)
    r = h.symmetry(c, apply=1, prep=True, rot0=rot0, tr0=tr0, sl=slice(0, 5))
    N = 2 * c["L"]
    for b in (0, 2, 3, 4):
        one = h.symmetry(c, apply=1, prep=True, rot0=rot0[b:b + 1], tr0=tr0[b:b + 1], sl=slice(b, b + 1))
        for k in ("lig", "tr_upd", "rot_upd", "sym_out", "step_out"):
            assert same_bits(one[k][0], r[k][b]), (b, k)
        for k in ("prep_pos", "prep_ca4", "prep_cb4"):
            assert same_bits(one[k], r[k].reshape(5, N * 4)[b]), (b, k)


@pytest.mark.parametrize("where,value", [("lig", np.nan), ("lig", np.inf), ("rec", np.nan), ("rec", -np.inf)])
def test_symmetry_nonfinite(h, where, value):
    """A non-finite coordinate in one ligand pose: that trajectory gets NaN diagnostics, m = 0 and a NaN step and, under apply, a NaN pose
    and NaN updates, while its finite neighbours are bitwise what they are without it.  In the receptor: every trajectory."""
    base = ah.sym_case(22, 3, 0)
    lig = base["lig"][[0, 2, 3, 6, 7]].copy()
    rec = base["rec_pos"].copy()
    rot0, tr0 = start_updates(5, 19)
    clean = h.symmetry(ah.sym_case_of(rec.reshape(-1, 3, 3), lig, 3, 0), apply=1, rot0=rot0, tr0=tr0)
    if where == "lig":
        lig[2, 13, 4] = value
        hit = [2]
    else:
        rec[7, 2] = value
        hit = [0, 1, 2, 3, 4]
    r = h.symmetry(ah.sym_case_of(rec.reshape(-1, 3, 3), lig, 3, 0), apply=1, rot0=rot0, tr0=tr0)
    for b in range(5):
        if b in hit:
            assert np.isnan(r["sym_out"][b, :10]).all() and r["sym_out"][b, 10] == 0 and np.isnan(r["step_out"][b]).all(), b
            assert np.isnan(r["lig"][b]).all() and np.isnan(r["tr_upd"][b]).all() and np.isnan(r["rot_upd"][b]).all(), b
        else:
            for k in ("lig", "tr_upd", "rot_upd", "sym_out", "step_out"):
                assert same_bits(r[k][b], clean[k][b]), (b, k)
    ev = ah.symmetry_ref(ah.sym_case_of(rec.reshape(-1, 3, 3), lig, 3, 0), hit[0])
    assert ev["m"] == 0 and np.isnan(ev["step"]).all() and np.isnan(ev["theta"])
