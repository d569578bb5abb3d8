"""The kernel harness of the docking-metrics kernels without a GPU (tests/metrics_harness.py, tests/kernels/metrics_harness.hip): the
shim builds and links against the library's launchers; the float64 definition is itself accurate to a quarter of every gate on every
GPU case's inputs (against its extended-precision evaluation); a numpy restatement of the kernels passes every comparison the GPU
tests use and each of its ten seeded mutants is rejected by them on the GPU tests' own inputs; the generators keep the pairs within
1e-3 A of a cutoff under the cap, and the lattice cases hold the planted pairs they claim."""

import numpy as np
import pytest

import metrics_harness as mh
import kernel_harness as kh


def all_cases():
    return mh.harness_cases() + mh.api_cases() + mh.lattice_cases() + (mh.poison_case(),)


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return mh.compile_shim(tmp_path_factory.mktemp("metrics_harness"))


def test_library_exports_the_launchers():
    out = kh.exported_symbols(mh.LIBDIR + "/libdfmdock_amd.so", True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in mh.LAUNCHERS:
        assert s in syms, s


def test_shim_links(shim):
    out = kh.exported_symbols(shim, False)
    for s in mh.LAUNCHERS:
        assert s in out, s
    kernels = kh.exported_symbols(shim, True)
    assert "kh_run" in kernels and "__device_stub__" not in kernels, "the shim adds no kernel of its own"
    h = mh.Harness(shim)      # also checks that the ctypes call record has the shim's size
    assert h.guard >= 1024


def test_shim_refuses_short_buffers(shim):
    """A buffer too small for the launch it feeds, or a contact that names no residue, is hipErrorInvalidValue before anything is
    allocated or launched (this runs without a GPU)."""
    h = mh.Harness(shim)
    c = mh.harness_cases()[4]
    k = mh.consts(c)
    bufs = dict(h._bufs(c), sums=mh.Out(np.float64, c.P * c.chains * 24), xf=mh.Out(np.float64, c.P * 36), rmsd=mh.Out(np.float64, c.P * 3),
                recovered=mh.Out(np.int32, c.P))
    for short in (dict(lig_model=c.lig[:-1]), dict(rec_model=c.rec[:-1]), dict(xf=mh.Out(np.float64, c.P * 36 - 1)), dict(flig=c.flig[:-1]),
                  dict(contacts=c.contacts[:-1]), dict(contacts=np.where(np.arange(c.contacts.size).reshape(-1, 2) == 4, c.R, c.contacts).astype(np.int32)),
                  dict(sums=mh.Out(np.float64, c.P * 24))):
        r = h.run("full", dict(bufs, **short), check=False, **h._scalars(c, k))
        assert r["err"] == mh.HIP_INVALID_VALUE, list(short)
    r = h.run("native_pairs", dict(rec_nat=c.nat_rec, lig_nat=c.nat_lig, pairs=mh.Out(np.uint8, c.R * c.L - 1)), check=False, R=c.R, L=c.L,
              iface_cutoff=10.0, contact_cutoff=5.5)
    assert r["err"] == mh.HIP_INVALID_VALUE


# ---- the cases hold what the issue lists -------------------------------------------------------------------------------------------------
def test_cases_cover_the_shapes():
    cs = mh.harness_cases()
    assert {(c.R, c.L) for c in cs} >= set(mh.SHAPES)
    for shape in mh.SHAPES:
        assert {c.chains for c in cs if (c.R, c.L) == shape} == {1, 2}, shape
    assert {c.P for c in cs} >= {1, 3, 4, 5, 67}
    assert {len(c.contacts) for c in cs} >= {0, 1, 63, 64, 65, 200}
    assert all((c.contacts[0] == (c.R - 1, c.L - 1)).all() for c in cs if len(c.contacts))
    kinds = {(int(c.frec.sum()), int(c.flig.sum())) for c in cs}
    assert (0, 0) in kinds and (1, 1) in kinds and any(c.frec.all() and c.flig.all() and c.R > 1 for c in cs)
    assert any(c.frec.sum() == 1 and c.frec[-1] and c.flig.sum() == 1 and c.flig[-1] and c.R > 64 and c.L > 64 for c in cs), "the lane tail alone"
    assert {k for c in cs for k in c.kinds} == set(mh.POSE_KINDS)
    assert any(np.abs(c.nat_rec).max() > 8000 for c in cs) and any(np.abs(c.nat_rec).max() < 1000 for c in cs)
    assert all(c.P <= 4096 and c.R <= 300 and c.L <= 300 for c in all_cases())
    api = mh.api_cases()
    assert {(c.R, c.L, c.chains) for c in api} == {(R, L, ch) for R, L in mh.SHAPES for ch in (1, 2)}
    assert any(not c.frec.any() for c in api) and any(c.frec.all() and c.flig.all() and c.R > 1 for c in api)
    assert any(c.frec.sum() == 1 and c.flig.sum() == 1 and c.R > 1 and c.L > 1 for c in api)
    planar = [c for c in cs if "planar" in c.name]
    collinear = [c for c in cs if "collinear" in c.name]
    assert len(planar) == 2 and all(np.ptp(c.nat_rec[..., 2]) == 0 for c in planar)
    for c in collinear:
        x = c.nat_rec.reshape(-1, 3).astype(np.float64)
        assert np.linalg.svd(x - x.mean(0), compute_uv=False)[1] < 1e-4
        assert not mh.definition(c)[1].any(), "a collinear receptor has no unique fit: l_rmsd is not compared"
    assert all(mh.definition(c)[1][np.isfinite(mh.definition(c)[0][:, 0])].all() for c in cs if c not in collinear), "every other fit is unique"


def test_lattice_cases_hold_their_planted_pairs():
    assert [c.R * c.L for c in mh.lattice_cases()] == [1, 255, 256, 257, 65 * 63]
    for c in mh.lattice_cases():
        for x in (c.nat_rec, c.nat_lig):
            off = x.astype(np.float64) * 4
            # multiples of 0.25 A, but for the x of the planted atoms one ulp inside (two residues of three atoms)
            assert (np.abs(off - np.round(off)) < 1e-4).all() and (off != np.round(off)).sum() <= 6
        want, d = mh.pairs_ref(c.nat_rec, c.nat_lig, *mh.LATTICE_CUTOFFS)
        assert (c.R - 1, c.L - 1) == c.planted[0][:2]
        for i, j, flags in c.planted:
            assert want[i, j] == flags, (c, i, j)
        on = [d[i, j] for i, j, _ in c.planted]
        assert 5.0 in on and (c.R * c.L == 1 or (13.0 in on and any(4.99999 < x < 5.0 for x in on) and any(12.99999 < x < 13.0 for x in on)))
        le, _ = mh.pairs_ref(c.nat_rec, c.nat_lig, *mh.LATTICE_CUTOFFS, mutant="le")
        assert (le != want).any()
        sure, _, _ = mh.recovered_ref(c)
        # the native pose finds its contacts, the planted contacts once more (they are listed twice) and no pair ON the cutoff
        assert sure[0] == len(c.native_contacts) + sum(1 for _, _, f in c.planted if f & 2), c
        assert (c.contacts[:, 0].max() == c.R - 1) and (c.contacts[:, 1].max() == c.L - 1)


# ---- item 3: the definition's own error ---------------------------------------------------------------------------------------------------
def test_definition_is_accurate_to_a_quarter_of_the_gate():
    """|float64 definition - extended precision| / gate over every compared RMSD of every GPU case: below 0.25.  The worst ratio is
    printed per group of cases."""
    worst = {}
    for c in all_cases() + (mh.poisoned(mh.poison_case(), "nan"), mh.poisoned(mh.poison_case(), "inf")):
        ref, unique = mh.definition(c)
        ext = mh.definition_extended(c)
        fin = np.isfinite(ref[:, 0])
        group = "9000 A" if np.abs(c.nat_rec).max() > 8000 else "elsewhere"
        for col in range(3):
            sel = fin & unique if col == 2 else fin
            sel = sel & np.isfinite(ref[:, col])
            assert (np.isfinite(ext[:, col]) == np.isfinite(ref[:, col])).all()
            r = mh.ratio_of(np.abs(ref[sel, col] - ext[sel, col]), mh.rmsd_gate(ext[sel, col]))
            worst[group] = max(worst.get(group, 0.0), r)
            assert r < 0.25, (c, col, r)
    print("definition error / gate:", {k: f"{v:.3g}" for k, v in worst.items()})


# ---- item 5: the comparisons have power ----------------------------------------------------------------------------------------------------
def solve_launch(mutant=None):
    sums, kinds = mh.solve_inputs()
    return mh.restate_solve(sums, 2, None, mh.SOLVE_CONSTS, mutant), sums, kinds


def test_restatement_passes_every_comparison():
    """The unmutated restatement on every case, the crafted k_metrics_solve launch included; the worst ratios are printed."""
    worst = {}
    for c in all_cases():
        ratios, _ = mh.check_full(mh.restate(c), c)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    xf, sums, kinds = solve_launch()
    for k, v in mh.check_solve(xf, sums, 2, None, mh.SOLVE_CONSTS, "crafted").items():
        worst["crafted " + k] = v
    print("restatement, error / gate:", {k: f"{v:.3g}" for k, v in worst.items()})
    lanes = np.array([k == "nan" for k in kinds])
    assert np.isnan(xf[lanes]).all((1, 2)).sum() == 0 and np.isnan(xf[lanes]).any((1, 2)).all() and np.isfinite(xf[~lanes]).all()
    for c in mh.lattice_cases():
        mh.check_pairs(mh.pairs_ref(c.nat_rec, c.nat_lig, *mh.LATTICE_CUTOFFS)[0], c.nat_rec, c.nat_lig, *mh.LATTICE_CUTOFFS, exact=True)


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", mh.MUTANTS)
def test_mutants_are_rejected(mutant):
    """Each seeded mutant of the restatement fails a comparison of the GPU tests on the GPU tests' own inputs - and on the inputs chosen
    for it: the 9000 A cases for the dropped shift, the crafted launch for the short Jacobi and the missing reflection fix, the lattice
    cases for <= at the cutoff, a moving receptor for rec_moves."""
    cs = mh.harness_cases()
    by = {c.name: c for c in cs + mh.lattice_cases()}
    hits = [c.name for c in cs + mh.lattice_cases() if rejected(lambda: mh.check_full(mh.restate(c, mutant), c))]
    print(mutant, "rejected on", hits)
    assert hits, mutant
    must = {"f32_accumulator": ["63x64 given", "130x300 implied"],
            "shift_dropped": [c.name for c in cs if np.abs(c.nat_rec).max() > 8000],
            "mean_over_n": [c.name for c in cs if c.P >= 3],
            "lane_tail_lost": [c.name for c in cs if (c.R % 64 and c.chains == 2) or c.L % 64],
            "lig_flags_ignored": [c.name for c in cs if not c.flig.all()],
            "all_atom_fit_for_l": [c.name for c in cs if c.P >= 3 and "collinear" not in c.name],
            "le_at_cutoff": [c.name for c in mh.lattice_cases()],
            "rec_moves_ignored": [c.name for c in cs if c.chains == 2 and set(c.kinds) != {"native"}],
            # the whole model mirrored (a mirrored ligand next to the unmoved receptor is still best fitted by a proper rotation)
            "no_reflection_fix": [c.name for c in cs if "mirror" in c.kinds and c.chains == 2 and c.R + c.L > 2]}.get(mutant, [])
    for name in must:
        assert name in hits, (mutant, name, by[name].kinds)
    if mutant in ("two_sweeps", "no_reflection_fix", "mean_over_n"):
        xf, sums, _ = solve_launch(mutant)
        assert rejected(lambda: mh.check_solve(xf, sums, 2, None, mh.SOLVE_CONSTS, "crafted")), mutant
    if mutant == "le_at_cutoff":
        for c in mh.lattice_cases():
            bad = mh.pairs_ref(c.nat_rec, c.nat_lig, *mh.LATTICE_CUTOFFS, mutant="le")[0]
            assert rejected(lambda: mh.check_pairs(bad, c.nat_rec, c.nat_lig, *mh.LATTICE_CUTOFFS, exact=True)), c


# ---- the border caps ------------------------------------------------------------------------------------------------------------------------
def test_border_pairs_stay_under_the_cap():
    """At most 0.5 % of the decisions of the generic k_native_pairs cases, and of the contact evaluations of the generic pose cases, lie
    within 1e-3 A of their cutoff; a lattice case has none by construction (its decisions are exact)."""
    n = b = 0
    for rec, lig in mh.generic_pair_cases():
        want, _ = mh.pairs_ref(rec, lig, 10.0, 5.5)
        e, k = mh.check_pairs(want, rec, lig, 10.0, 5.5, exact=False)
        n, b = n + e, b + k
    print(f"k_native_pairs: {b} borderline of {n} decisions")
    assert n > 50000 and b <= mh.BORDER_CAP * n
    n = b = 0
    for c in mh.harness_cases() + mh.api_cases() + (mh.poison_case(),):
        _, border, e = mh.recovered_ref(c)
        n, b = n + e, b + int(border.sum())
    print(f"recovered contacts: {b} borderline of {n} evaluations")
    assert n > 10000 and b <= mh.BORDER_CAP * n
