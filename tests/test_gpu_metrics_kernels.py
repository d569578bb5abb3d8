"""The docking-metrics kernels launch by launch (kernels_metrics.hip: k_native_pairs, k_metrics_reduce, k_metrics_solve,
k_metrics_resid), driven through tests/kernels/metrics_harness.hip on small host arrays with guard bands around every device block,
against the float64 references of tests/metrics_harness.py (written from dfmdock_amd/metrics.py; tests/test_metrics_harness_cpu.py
shows that the definition is accurate to a quarter of every gate on these inputs and that the comparisons used here reject ten seeded
mutants of a numpy restatement of the kernels), and the same cases through the public call engine.Native.metrics.

What is exact and what carries a gate (metrics_harness.py states each with its derivation):
  exact            the pair flags and the recovered contacts on lattice coordinates, pairs planted exactly on a cutoff and one fp32 ulp
                   inside it included; the interface residues and contacts dfm_native_create reports for them; what a NaN pose or an
                   infinite coordinate leaves of its three neighbours in a workgroup (bitwise what they are without it).
  border rule      on generic coordinates a decision within 1e-3 A of its cutoff may go either way (at most 0.5 % of the decisions).
  sums             (n_atoms + 8) 2^-53 sum |terms| around the exactly rounded sum.
  fits             |R R^T - I|, |det R - 1| <= 1e-13, tr(R M) within 1e-12 s1 of the optimum, t to 1e-13 (|T| + |S|) / n; a fit whose M
                   holds a NaN is NaN throughout, and only that fit.
  RMSDs            1e-9 A + 1e-9 rmsd against the SVD definition; l_rmsd where the receptor's fit is unique.
The largest error / gate of every toleranced comparison goes to $DFM_METRICS_PROFILE/metrics_kernels_gpu.txt when that variable names a
directory (profiles/metrics_kernels.txt holds the MI355X figures).
"""
import os

import numpy as np
import pytest

import metrics_harness as mh

pytestmark = pytest.mark.gpu

RATIOS = {}
COUNTS = {"recovered evaluations": 0, "recovered borderline": 0}


def note(prefix, ratios):
    for k, v in ratios.items():
        RATIOS[f"{prefix} {k}"] = max(RATIOS.get(f"{prefix} {k}", 0.0), float(v))
    print(prefix, {k: f"{v:.3g}" for k, v in ratios.items()})


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    harness = mh.Harness(mh.compile_shim(tmp_path_factory.mktemp("metrics_harness_gpu")))
    yield harness
    out = os.environ.get("DFM_METRICS_PROFILE")
    if out:
        with open(os.path.join(out, "metrics_kernels_gpu.txt"), "w") as f:
            f.write("comparison max_error_over_gate\n" + "".join(f"{k} {v:.4g}\n" for k, v in sorted(RATIOS.items())))
            f.write("".join(f"{k} {v}\n" for k, v in sorted(COUNTS.items())))


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def count(evals):
    COUNTS["recovered evaluations"] += evals[0]
    COUNTS["recovered borderline"] += evals[1]


# ---- k_native_pairs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mh.lattice_cases(), ids=repr)
def test_native_pairs_lattice(h, case):
    """Exact, the pairs ON a cutoff (no contact) and one fp32 ulp inside (a contact) included; R L = 1, 255, 256, 257, 65 x 63."""
    flags = h.native_pairs(case.nat_rec, case.nat_lig, *mh.LATTICE_CUTOFFS)
    mh.check_pairs(flags, case.nat_rec, case.nat_lig, *mh.LATTICE_CUTOFFS, exact=True)
    for i, j, want in case.planted:
        assert flags[i, j] == want, (i, j)


def test_native_pairs_generic(h):
    n = b = 0
    for rec, lig in mh.generic_pair_cases():
        e, k = mh.check_pairs(h.native_pairs(rec, lig, 10.0, 5.5), rec, lig, 10.0, 5.5, exact=False)
        n, b = n + e, b + k
    COUNTS["k_native_pairs decisions"], COUNTS["k_native_pairs borderline"] = n, b
    assert b <= mh.BORDER_CAP * n


# ---- reduce, finish, full ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mh.harness_cases() + mh.lattice_cases(), ids=repr)
def test_full(h, case):
    """reduce + finish in one go against every reference; `reduce` alone and `finish` on its sums give the same bits."""
    out = h.full(case)
    ratios, evals = mh.check_full(out, case)
    note("lattice" if case.lattice else "full", ratios)
    count(evals)
    sums = h.reduce(case)
    assert sums.tobytes() == out["sums"].tobytes()
    fin = h.finish(case, sums, out["rec_const"])
    for k in ("xf", "rmsd", "recovered"):
        assert fin[k].tobytes() == out[k].tobytes(), k
    if case.chains == 1:      # the implied receptor's constants are its sums as its own model
        k = mh.consts(case)
        ref, bound = mh.sums_exact(case.nat_rec[None], case.nat_rec, case.frec, k["o"])
        note("rec_const", {"sums": mh.ratio_of(np.abs(out["rec_const"] - ref[0]), bound[0])})
        assert mh.ratio_of(np.abs(out["rec_const"] - ref[0]), bound[0]) <= 1.0


def test_mirrored_model_does_not_fit(h):
    """A mirrored model is no rigid image of the native: c_rmsd stays large (and equals the definition's, which test_full holds it to)."""
    seen = 0
    for case in mh.harness_cases():
        if case.chains == 2 and "mirror" in case.kinds and case.R + case.L >= 100:
            rmsd = h.full(case)["rmsd"]
            for p, kind in enumerate(case.kinds):
                if kind == "mirror":
                    seen += 1
                    assert rmsd[p, 0] > 1.0 and rmsd[p, 0] == pytest.approx(mh.definition(case)[0][p, 0], abs=1e-9, rel=1e-9)
    assert seen >= 2


def test_solve_on_crafted_sums(h):
    """k_metrics_solve alone: 4096 lanes in one launch, three crafted matrices per lane (metrics_harness.solve_inputs)."""
    sums, kinds = mh.solve_inputs()
    P = len(kinds)
    case = mh.solve_dummy_case(P)
    out = h.finish(case, sums, k=mh.SOLVE_CONSTS)
    note("crafted", mh.check_solve(out["xf"], sums, 2, None, mh.SOLVE_CONSTS, "crafted"))
    lanes = np.array([k == "nan" for k in kinds])
    bad = np.isnan(out["xf"]).any(2)
    assert not bad[~lanes].any(), "a NaN left its lane"
    assert bad[lanes].any(1).all() and not bad[lanes].all(1).any(), "a NaN lane has the fits that read the NaN, and only those, NaN"
    assert np.isnan(out["xf"][bad]).all(), "a fit with a NaN is NaN throughout"
    # per kind: the largest optimality gap
    for kind in mh.SOLVE_KINDS:
        sel = np.array([k == kind for k in kinds])
        if kind != "nan":
            r = mh.check_solve(out["xf"][sel], sums[sel], 2, None, mh.SOLVE_CONSTS, kind)
            RATIOS[f"crafted optimality {kind}"] = r["optimality"]
    # exact half-turns about the axes come back as the half-turn itself, to the last bit but for the sign of a zero
    for axis, kind in enumerate(("halfturn_x", "halfturn_y", "halfturn_z")):
        sel = np.array([k == kind for k in kinds])
        d = -np.ones(3)
        d[axis] = 1.0
        for fit in (1, 2):
            np.testing.assert_array_equal(out["xf"][sel][:, fit, :9], np.broadcast_to(np.diag(d).reshape(9), (sel.sum(), 9)))


def test_solve_without_residues(h):
    """n == 0: all 12 entries of that fit are NaN - the interface fit without an interface residue, every fit without any residue."""
    sums, _ = mh.solve_inputs()
    sums = np.ascontiguousarray(sums[:5])
    case = mh.solve_dummy_case(5)
    k = dict(mh.SOLVE_CONSTS, n_rec_iface=0, n_lig_iface=0)
    out = h.finish(case, sums, k=k)
    assert np.isnan(out["xf"][:, 1]).all() and np.isfinite(out["xf"][:, [0, 2]]).all()
    mh.check_solve(out["xf"], sums, 2, None, k, "no interface")
    assert np.isnan(out["rmsd"][:, 1]).all()
    out = h.finish(case, sums, k=dict(k, n_rec=0, n_lig=0))
    assert np.isnan(out["xf"]).all()
    out = h.finish(case, sums, k=dict(k, n_lig=0))      # the ligand uncounted: the all-atom and the receptor fit divide by n_rec
    assert np.isnan(out["xf"][:, 1]).all() and np.isfinite(out["xf"][:, [0, 2]]).all()


def test_poisoned_pose_keeps_to_itself(h):
    """One NaN pose, then one +inf coordinate, at pose 2 of a workgroup of four: nothing of it is finite, and its three neighbours are
    bitwise what they are without it - sums, fits, RMSDs and recovered contacts."""
    clean_case = mh.poison_case()
    clean = h.full(clean_case)
    ratios, evals = mh.check_full(clean, clean_case)
    note("full", ratios)
    count(evals)
    keep = np.arange(4) != 2
    for how in ("nan", "inf"):
        case = mh.poisoned(clean_case, how)
        out = h.full(case)
        for k in ("sums", "xf", "rmsd", "recovered"):
            assert out[k][keep].tobytes() == clean[k][keep].tobytes(), (how, k)
        assert not np.isfinite(out["rmsd"][2]).any(), how
        assert not np.isfinite(out["xf"][2, :2]).any(), how
        assert np.isfinite(out["xf"][2, 2]).all(), "the receptor of the poisoned pose is finite, and so is its fit"
        mh.check_full(out, case)
        if how == "nan":
            assert out["recovered"][2] == 0


# ---- the public call ------------------------------------------------------------------------------------------------------------------------
def through_the_call(model, case, iface_cutoff, contact_cutoff, contacts):
    with model.native(case.nat_rec, case.nat_lig, iface_cutoff=iface_cutoff, contact_cutoff=contact_cutoff) as nat:
        info = nat.info()
        got = nat.metrics(case.lig, case.rec)
    np.testing.assert_array_equal(info["iface_rec"], np.where(case.frec)[0])
    np.testing.assert_array_equal(info["iface_lig"], np.where(case.flig)[0])
    np.testing.assert_array_equal(info["contacts"], contacts)
    fnat = np.array([round(int(n) / (len(contacts) + 1e-6), 6) for n in got["n_recovered"]])
    np.testing.assert_array_equal(got["fnat"], fnat)
    return np.stack([got["c_rmsd"], got["i_rmsd"], got["l_rmsd"]], 1), got["n_recovered"]


@pytest.mark.parametrize("case", mh.api_cases(), ids=repr)
def test_public_call(model, case):
    """engine.Native.metrics at the tight gate: every chain length, the receptor implied and given, no / every / one / the usual
    interface; the interface residues and contacts it derives equal the float64 decisions."""
    rmsd, found = through_the_call(model, case, case.iface_cutoff, 5.5, case.contacts)
    note("public call", {"rmsd": mh.check_rmsd(rmsd, case)})
    count(mh.check_recovered(found, case))


@pytest.mark.parametrize("case", mh.lattice_cases(), ids=repr)
def test_public_call_lattice(model, case):
    """The lattice natives through dfm_native_create: interface residues, contacts and recovered contacts exactly."""
    own = mh.Case(case.name, case.nat_rec, case.nat_lig, case.lig, None, case.frec, case.flig, case.native_contacts, case.kinds,
                  cutoff=mh.LATTICE_CUTOFFS[1], lattice=True)
    rmsd, found = through_the_call(model, own, *mh.LATTICE_CUTOFFS, case.native_contacts)
    note("public call", {"rmsd": mh.check_rmsd(rmsd, own)})
    sure, _, _ = mh.recovered_ref(own)
    np.testing.assert_array_equal(found, sure)
