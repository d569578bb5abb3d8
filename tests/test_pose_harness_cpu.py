"""The kernel harness of the rigid-pose kernels without a GPU (tests/pose_harness.py, tests/kernels/pose_harness.hip): the shim builds,
links against the library's launchers and refuses every bad index on the CPU side of its call record; the numpy frame equals
dfm_poseprep.h: build_pose_frame (tests/pose_frame_main.cpp, built as tests/test_pose_prep_cpu.py builds it) on every case that uses a
host-shaped frame; the brute-force restatement agrees with the package's definition under the existing border rule; the inputs hold
what the GPU tests rely on (no sqrt-based decision of a generic case within 1e-9 A of its threshold, the planted pairs, ties that are
exact in float64, the rows of 0 .. 129 atoms); the restatement WITH the walk equals the brute force bit for bit, and each of its seeded
mutants is rejected by the comparison functions the GPU tests use, on the GPU tests' own cases; the mpmath reference and the numpy
restatement of pose_transform agree to the figure the device's gate is built on."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_harness as ph
import kernel_harness as kh

ROOT = ph.ROOT
BORDER, BORDER_CAP = 1e-3, 0.005      # the border rule of the API tests: a decision this close to its cutoff, for at most this share


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return ph.Harness(ph.compile_shim(tmp_path_factory.mktemp("pose_harness")))


def test_shim_links_and_adds_no_kernel(shim):
    und = kh.exported_symbols(shim.path, False)
    for name in ("launch_sterics_pose", "launch_surface_pose", "launch_iface_pose", "launch_rescon_pose", "launch_hbond_pose",
                 "launch_pairpot_pose", "launch_stericsERK", "launch_resconERK", "launch_rescon_finish", "launch_hbond_finish"):
        assert name in und, name
    defined = kh.exported_symbols(shim.path, True)
    assert "kh_run" in defined and "__device_stub__" not in defined, "the shim adds no kernel of its own"
    assert shim.guard >= 1024


def _sterics_call(h, case, **change):
    fr, P = case.fr, len(case.T)
    bufs, sc = h._frame(fr)
    bufs.update(T=case.T, n_clash=ph.Out(np.int32, P), n_contact=ph.Out(np.int32, P), min_bits=ph.Out(np.uint64, P),
                lig_clash=ph.Out(np.int32, P * fr.Al), lig_contact=ph.Out(np.int32, P * fr.Al), exits=ph.Out(np.uint64, 2))
    sc = dict(sc, n=P)
    for k, v in change.items():
        (sc if k in sc else bufs)[k] = v
    return bufs, sc


def test_shim_refuses_every_bad_index(shim):
    """Everything a kernel would follow as an index, wrong in turn: hipErrorInvalidValue from the check that kh_run makes before it touches
    the device (ph_check is that check alone; this runs without a GPU)."""
    c = ph.generic_case(0)
    fr, P = c.fr, len(c.T)
    bufs, sc = _sterics_call(shim, c)
    assert shim.check_only("sterics", bufs, **sc) == ph.HIP_SUCCESS
    cs = fr.cell_start
    dup = fr.lig_index.copy()
    dup[3] = dup[4]
    big = fr.lig_index.copy()
    big[0] = fr.Al
    bad = [dict(rec=fr.rec4[:-1]), dict(lig=fr.lig4[:-1]), dict(sphere=fr.sphere[:-1]), dict(cell_start=cs[:-1]), dict(T=c.T[:-1]),
           dict(cell_start=np.concatenate([[1], cs[1:]]).astype(np.int32)), dict(cell_start=np.concatenate([cs[:-1], [fr.Ar + 1]]).astype(np.int32)),
           dict(cell_start=np.concatenate([cs[:1], cs[2:3], cs[1:2], cs[3:]]).astype(np.int32) if cs[1] != cs[2] else cs[:-1]),
           dict(lig_index=dup), dict(lig_index=big), dict(lig_index=fr.lig_index[:-1]), dict(n_clash=ph.Out(np.int32, P - 1)),
           dict(min_bits=ph.Out(np.uint64, P - 1)), dict(lig_contact=ph.Out(np.int32, P * fr.Al - 1)), dict(exits=ph.Out(np.uint64, 1)),
           dict(nx=fr.dims[0] + 1), dict(nz=0), dict(edge=0.0), dict(edge=np.nan), dict(Ar=fr.Ar + 1), dict(Al=fr.Al + 1), dict(Al=0),
           dict(n_contact=np.zeros(P, np.int32)), dict(lo=[np.inf, 0, 0])]
    for change in bad:
        b, s = _sterics_call(shim, c, **change)
        assert shim.check_only("sterics", b, **s) == ph.HIP_INVALID_VALUE, list(change)
    # the pose kernels, the residue bits, the finish kernels
    rot, tr = ph.pose_inputs(5)
    ok = dict(rot=rot, tr=tr, T=ph.Out(np.float64, 60), tot=ph.Out(np.int64, 20))
    assert shim.check_only("pose_iface", ok, n=5) == ph.HIP_SUCCESS
    for change in (dict(rot=rot[:-1]), dict(T=ph.Out(np.float64, 59)), dict(tot=ph.Out(np.int64, 19)), dict(T=np.zeros(60))):
        assert shim.check_only("pose_iface", dict(ok, **change), n=5) == ph.HIP_INVALID_VALUE, list(change)
    assert shim.check_only("pose_iface", ok, n=0) == ph.HIP_INVALID_VALUE and shim.check_only("pose_surface", ok, n=5) == ph.HIP_INVALID_VALUE
    rc = ph.rescon_case()
    bufs, sc = shim._frame(rc.fr)
    del bufs["lig_index"]
    bufs.update(T=rc.T, bits=ph.Out(np.uint32, len(rc.T) * rc.Lr * 128))
    sc = dict(sc, n=len(rc.T), Rr=rc.Rr, Lr=rc.Lr, W=128)
    assert shim.check_only("rescon", bufs, **sc) == ph.HIP_SUCCESS
    for change in (dict(Rr=4095), dict(Lr=65), dict(W=127), dict(Lr=71)):      # a residue bit at or above Rr / Lr, a row too short, bits too short
        assert shim.check_only("rescon", bufs, **dict(sc, **change)) == ph.HIP_INVALID_VALUE, list(change)
    bits, rcl, lcl = ph.finish_inputs(33, 65)
    fin = dict(bits=bits, class_mask=ph.class_masks(33, rcl), lig_class=lcl, tot=ph.Out(np.int32, 27), rec_degree=ph.Out(np.int32, 99))
    assert shim.check_only("rescon_finish", fin, n=3, Rr=33, Lr=65, W=2) == ph.HIP_SUCCESS
    for change in (dict(W=1), dict(Rr=65), dict(Lr=66), dict(n=4)):
        assert shim.check_only("rescon_finish", fin, **dict(dict(n=3, Rr=33, Lr=65, W=2), **change)) == ph.HIP_INVALID_VALUE, list(change)
    assert shim.check_only("rescon_finish", dict(fin, lig_class=np.where(np.arange(65) == 7, 3, lcl).astype(np.int32)), n=3, Rr=33, Lr=65, W=2) == ph.HIP_INVALID_VALUE
    hb = dict(bits=np.zeros(130, np.uint32), tot=ph.Out(np.int32, 10))
    assert shim.check_only("hbond_finish", hb, n=2, Lc=5, Wc=13) == ph.HIP_SUCCESS
    assert shim.check_only("hbond_finish", hb, n=2, Lc=5, Wc=14) == ph.HIP_INVALID_VALUE
    assert shim.check_only("hbond_finish", hb, n=3, Lc=5, Wc=13) == ph.HIP_INVALID_VALUE


# ---- 1. the numpy frame equals dfm_poseprep.h ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_frame")
    exe = str(d / "pose_frame")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "pose_frame_main.cpp"), "-o", exe])

    def run(fr):
        path = str(d / "atoms.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iif", fr.Ar, fr.Al, fr.reach))
            for a in (fr.center32, fr.rec_atoms, fr.lig_atoms):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        r = subprocess.run([exe, path, "cutoff"], capture_output=True, text=True)
        assert r.stderr == "" and r.returncode == 0, r.stderr      # a sanitizer report
        return {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    return run


def test_numpy_frame_equals_the_host_preparation(frame_exe):
    """Grid, starts, order, ligand index, spheres, threshold and slack, to the printed digits (17 for a double, 9 for a float: both give
    the number back)."""
    seen = set()
    others = [(n, c.fr) for n, c, _ in ph.iface_cases() + ph.pairpot_cases()] + [(n, hb.fr) for n, hb, _, _, _ in ph.hbond_cases()]
    for c, fr in [(c, c.fr) for c in ph.host_shaped_cases()] + others + [("api", ph.Frame(*ph.generic_atoms(0)[:3], 3.0, 5.0))]:
        if id(fr) in seen:
            continue
        seen.add(id(fr))
        out = frame_exe(fr)
        d = lambda k: np.array([float(v) for v in out[k]], np.float64)
        g = lambda k: np.array([float(v) for v in out[k]], np.float32)
        i = lambda k: np.array([int(v) for v in out[k]], np.int64)
        assert np.array_equal(d("lo"), fr.lo) and np.array_equal(d("hi"), fr.hi) and np.array_equal(d("center"), fr.center), c
        assert tuple(i("dims")) == fr.dims + (fr.max_cell,), c
        assert np.array_equal(d("edge_grow"), [fr.edge, fr.grow]) and np.array_equal(g("thr_reject2"), np.float32([fr.thr, fr.reject2])), c
        assert np.array_equal(i("cell_start"), fr.cell_start) and np.array_equal(i("order"), fr.order), c
        assert np.array_equal(d("lig_lo"), fr.lig_lo) and np.array_equal(i("lig_index"), fr.lig_index), c
        assert np.array_equal(g("sphere"), fr.sphere.reshape(-1)) and out["finite"] == ["1"], c
    assert len(seen) >= 24 and {float(fr.reach) for _, fr in others} >= {4.0, 5.0, 5.5, 8.0}
    far = ph.far_cases()
    assert far[0].fr.slack == np.float32(1e-3) and far[1].fr.slack > np.float32(4e-3), "pose_slack is above its floor at 20000 A only"


# ---- 2. the restatement agrees with the package's definition ---------------------------------------------------------------------------------
def test_restatement_agrees_with_the_definition():
    """sterics.sterics poses the ligand with `@ R.T`, which does not round like the kernel: a pair within 1e-3 A of a cutoff may fall either
    way, for at most 0.5 % of the decisions."""
    from dfmdock_amd import sterics as ST
    for seed in (0, 1):
        c = ph.generic_case(seed)
        rec, lig, cen, rot, tr = ph.generic_atoms(seed)
        want = ST.sterics(rec, lig, cen, rot, tr, ph.GENERIC["clash"], ph.GENERIC["contact"], per_atom=True)
        d = c.ref["d"]
        border = np.stack([(np.abs(d - cut) < BORDER).sum((1, 2)) for cut in (c.fr.clash, c.fr.contact)])
        assert border.sum() <= BORDER_CAP * 2 * d.size
        for k, b in (("n_clash", border[0]), ("n_contact", border[1])):
            assert (np.abs(want[k].astype(np.int64) - c.ref[k]) <= b).all(), (seed, k)
        assert want["n_contact"].sum() > 1000, "the poses touch"
        np.testing.assert_allclose(want["min_dist"], c.ref["min_dist"], rtol=0, atol=1e-9)
        if not border.any():
            for k in ("lig_clash", "lig_contact"):
                np.testing.assert_array_equal(want[k], c.ref[k])


def test_rescon_restatements_agree_with_the_definition():
    """affinity.residue_contacts on the rot / tr, residues and classes of the residue-contact case against rescon_bits_ref (the bitmap) and
    rescon_finish_ref (ic, n_pairs, n_rec_res, n_lig_res, both degree arrays).  The border rule: the definition's bitmap lies between the
    restatement's at cutoff - 1e-3 A and at cutoff + 1e-3 A, and equals the restatement's - with every total and degree - for each pose in
    which those two are the same bitmap.  The finish restatement on the DEFINITION's own bitmap must give the definition's totals and
    degrees for every pose: no distance is involved there."""
    import copy
    from dfmdock_amd import affinity as AF
    rc = ph.rescon_case()
    rec, lig, cen, rot, tr = ph.generic_atoms(0)
    rcl, lcl = np.random.default_rng(1).integers(0, 3, rc.Rr).astype(np.uint8), np.random.default_rng(2).integers(0, 3, rc.Lr).astype(np.uint8)
    want = AF.residue_contacts(rec, rc.rec_res, rcl, lig, rc.lig_res, lcl, cen, rot, tr, ph.GENERIC["contact"], per_residue=True, bits=True)

    def bits_at(cut):
        f = copy.copy(rc.fr)
        f.contact = cut
        return ph.rescon_bits_ref(f, rc.T, rc.rec_res, rc.lig_res, rc.Rr, rc.Lr)
    bits, sure, loose = bits_at(rc.fr.contact), bits_at(rc.fr.contact - BORDER), bits_at(rc.fr.contact + BORDER)
    got = want["contact_bits"]
    assert got.shape == bits.shape and ((sure & ~got) == 0).all() and ((got & ~loose) == 0).all()
    settled = (sure == loose).all((1, 2))
    assert settled.sum() >= 3 and ph.popcount(bits[settled]).sum() > 100, "poses without a borderline residue pair, and they touch"
    assert np.array_equal(got[settled], bits[settled])

    def same(fin, sel):
        t = fin["tot"]
        return all(np.array_equal(np.asarray(a)[sel], np.asarray(b)[sel]) for a, b in (
            (t[:, :6], want["ic"]), (t[:, 6], want["n_pairs"]), (t[:, 7], want["n_rec_res"]), (t[:, 8], want["n_lig_res"]),
            (fin["rec_degree"], want["rec_degree"]), (fin["lig_degree"], want["lig_degree"])))
    assert same(ph.rescon_finish_ref(got, rc.Rr, rcl, lcl.astype(np.int32)), slice(None)), "the finish restatement on the definition's bitmap"
    assert same(ph.rescon_finish_ref(bits, rc.Rr, rcl, lcl.astype(np.int32)), settled), "bitmap and finish restatements together"
    assert want["ic"].sum(0).min() > 0 and {0, 31, 32, 4095} <= set(np.where(want["rec_degree"].sum(0) > 0)[0].tolist())


# ---- 3. the input conditions -----------------------------------------------------------------------------------------------------------------
def test_no_generic_decision_lies_on_its_threshold():
    """Bitwise comparison of a sqrt-based decision needs the device's sqrt only to be within an ulp or so: on every generic case no
    distance is within 1e-9 A of a cutoff (the seeds were picked for it).  The tie and knife-edge cases are exact by construction."""
    for c in (ph.generic_case(0), ph.generic_case(1)) + ph.grid_variants() + ph.size_cases() + ph.row_cases() + ph.far_cases() + (ph.rescon_case(),):
        d = c.ref["d"]
        for cut in (c.fr.clash, c.fr.contact):
            assert not (np.abs(d - cut) < 1e-9).any(), (c, cut)


def test_cases_hold_what_they_claim():
    g = ph.generic_case(0)
    assert (g.fr.Ar, g.fr.Al, len(g.T)) == (300, 130, 6) and len(g.fr.sphere) == 3
    status, _ = g.front
    assert (status[:-1] == 0).all(1).any(), "a pose with three walked blocks: the atomic minimum has three contenders"
    assert (status[-1] == 1).all() and (status[4] == 2).any(), "the far pose leaves at the sphere test, a block of pose 4 at the box test"
    assert all((c.front[0] == 0).any() and c.ref["n_contact"].sum() > 0 for c in ph.size_cases()), "every size case walks and touches"
    walked_min = [np.where((g.ref["d"][0, 64 * b:64 * b + 64] < g.fr.contact), g.ref["d"][0, 64 * b:64 * b + 64], np.inf).min() for b in range(3)]
    assert np.isfinite(walked_min).all()
    assert sorted(c.fr.Al for c in ph.size_cases()) == [1, 63, 64, 65, 129] and {len(c.T) for c in ph.size_cases()} == {1, 2, 8}
    assert all(c.fr.Ar == 1 for c in ph.size_cases())
    for c in ph.row_cases():
        rows = ph.sterics_walk(c.fr, c.T)["rows"]
        assert c.row is None or c.row in rows, (c, rows)
        assert c.ref["n_contact"].sum() > 0
    assert ph.row_cases()[-1].fr.max_cell >= 200
    for c in ph.grid_variants():
        assert c.fr.dims != g.fr.dims or not np.array_equal(c.fr.lig_index, g.fr.lig_index) or not np.array_equal(c.fr.sphere, g.fr.sphere), c
    assert ph.grid_variants()[3].fr.dims == (1, 1, 1)
    # far from the origin: at least 100 pairs in the last 1e-2 A below the contact cutoff
    for c in ph.far_cases():
        assert ph.last_hundredth(c) >= 100, (c, ph.last_hundredth(c))
    assert len(ph.knife_cases()) == 2
    for c in ph.knife_cases():
        assert (c.ref["d"] == c.fr.contact).any() or (c.ref["d"] == np.nextafter(c.fr.contact, 0)).any()
    nf = ph.nonfinite_T_case()
    assert len(nf.T) == 26 and (~np.isfinite(nf.T)).sum() == 24 and ph.finite_poses(nf.T).sum() == 2
    assert nf.ref["n_contact"][0] > 0 and (nf.ref["n_contact"][1:25] == 0).all() and nf.ref["n_contact"][25] == nf.ref["n_contact"][0]


def test_tie_cases_are_exact_in_float64():
    """Every coordinate a multiple of 0.25 A, every pose a lattice map: the squared distance of every pair is an integer multiple of 1/16
    that float64 holds exactly, so d is the correctly rounded sqrt of the true squared distance and `d < cutoff` is the true decision."""
    base, up, same = ph.tie_cases()
    fr = base.fr
    X, Y, Z = ph.posed(fr, base.T)
    for v in (X, Y, Z):
        assert (v * 4 == np.round(v * 4)).all()
    r = ph.f64(fr.rec4)
    n2 = sum((np.round(4 * (v[..., None] - r[:, k])).astype(np.int64)) ** 2 for k, v in enumerate((X, Y, Z)))
    assert np.array_equal(base.ref["d"], np.sqrt(n2 / 16.0))      # n2 / 16 is exact: the restatement's sum of squares lost nothing
    assert np.array_equal(base.ref["d"] < 5.0, n2 < 400) and np.array_equal(base.ref["d"] < 3.0, n2 < 144)
    on5, on3, on0 = int((n2[0] == 400).sum()), int((n2[0] == 144).sum()), int((n2[0] == 0).sum())
    assert on5 >= 3 and on3 >= 1 and on0 >= 1, (on5, on3, on0)
    assert up.ref["n_contact"][0] - base.ref["n_contact"][0] == on5, "the pairs AT 5 A are contacts one fp32 ulp of cutoff above it only"
    assert same.ref["n_clash"].tolist() == same.ref["n_contact"].tolist() == base.ref["n_contact"].tolist()


# ---- 4. the walk restated, and its mutants -----------------------------------------------------------------------------------------------------
def as_device(w):
    """A restated launch in the form Harness.sterics returns."""
    return dict(w, min_bits=w["min_dist"].view(np.uint64))


def test_walk_restatement_equals_the_brute_force():
    """The kernel's way - early exits, cell ranges, rows in batches of 64, the fp32 reject - finds exactly the pairs of all P x Al x Ar: in
    numpy, on every case the GPU tests use, the far ones and the non-host grids included."""
    for c in ph.walk_cases():
        n, _ = ph.check_sterics(as_device(ph.sterics_walk(c.fr, c.T, base=(7, -3))), c.ref, c.front[0], base=(7, -3))
        assert n == 2 * len(c.T) * c.fr.Al * c.fr.Ar
    g = ph.generic_case(0)
    for v in ph.grid_variants():
        for k in ("n_clash", "n_contact", "min_dist", "lig_clash", "lig_contact"):
            assert v.ref[k].tobytes() == g.ref[k].tobytes(), (v, k)


# mutant -> the comparison of check_sterics that must catch it (its first assertion to fail)
CAUGHT_BY = {"f32_pose": "min_dist", "min_of_last_block": "min_dist"}      # every other one: n_contact, the first count compared

# mutant -> the case of the GPU tests that rejects it
REJECTED_BY = {"f32_pose": lambda: ph.generic_case(0), "fma": lambda: ph.knife_cases()[0], "le": lambda: ph.tie_cases()[0],
               "reject_bare": lambda: ph.far_cases()[0], "reject_factor_only": lambda: ph.far_cases()[1],
               "first_64_of_a_row": lambda: ph.row_cases()[4], "last_cell_dropped": lambda: ph.generic_case(0),
               "lanes_past_Al": lambda: ph.generic_case(0), "T_transposed": lambda: ph.generic_case(1),
               "sphere_no_grow": lambda: ph.row_cases()[0], "min_of_last_block": lambda: ph.generic_case(0)}


@pytest.mark.parametrize("mutant", ph.MUTANTS)
def test_walk_mutants_are_rejected(mutant):
    """Each seeded mutant of the restated kernel fails check_sterics on a case of the GPU tests (and the unmutated restatement passes it:
    test_walk_restatement_equals_the_brute_force)."""
    c = REJECTED_BY[mutant]()
    with pytest.raises(AssertionError) as caught:
        ph.check_sterics(as_device(ph.sterics_walk(c.fr, c.T, mutant)), c.ref, c.front[0])
    by = CAUGHT_BY.get(mutant, "n_contact")
    assert by in str(caught.value), f"{mutant} was to be caught by {by}: {caught.value}"
    print(f"{mutant}: rejected on '{c}' by the comparison of {by}")


def test_an_fp32_pose_flips_a_count_on_the_knife_edge():
    """On the generic case the fp32 pose is caught by min_dist.  The count decisions have power against it too: with the contact cutoff one
    double above a pair's own distance, rounding the posed atom to fp32 moves that pair across it and n_contact changes."""
    flipped = [c for c in ph.knife_cases() if not np.array_equal(ph.sterics_walk(c.fr, c.T, "f32_pose")["n_contact"], c.ref["n_contact"])]
    assert flipped, "no knife-edge case changes a count under an fp32 pose"
    print("f32_pose: n_contact changes on", flipped)


def test_fused_product_is_caught_from_both_sides():
    for c in ph.knife_cases():
        with pytest.raises(AssertionError):
            ph.check_sterics(as_device(ph.sterics_walk(c.fr, c.T, "fma")), c.ref, c.front[0])


def test_factor_alone_passes_at_3000_and_fails_at_20000():
    """The slack above its floor is what the 20000 A case tests: the factor alone still finds every pair at 3000 A."""
    near, far = ph.far_cases()
    ph.check_sterics(as_device(ph.sterics_walk(near.fr, near.T, "reject_factor_only")), near.ref, per_atom=False)
    with pytest.raises(AssertionError):
        ph.check_sterics(as_device(ph.sterics_walk(far.fr, far.T, "reject_factor_only")), far.ref, per_atom=False)


def test_finish_mutants_are_rejected():
    rc = ph.rescon_case()
    good = ph.rescon_bits_ref(rc.fr, rc.T, rc.rec_res, rc.lig_res, rc.Rr, rc.Lr)
    assert ph.popcount(good).sum() > 50
    assert good.tobytes() != ph.rescon_bits_ref(rc.fr, rc.T, rc.rec_res, rc.lig_res, rc.Rr, rc.Lr, "last_kept").tobytes(), \
        "last_kept: rejected on 'rescon Rr 4096'"
    bits, rcl, lcl = ph.finish_inputs(4096, 65)
    with pytest.raises(AssertionError):
        ph.check_finish(ph.rescon_finish_ref(bits, 4096, rcl, lcl, "words_64_up_dropped"), ph.rescon_finish_ref(bits, 4096, rcl, lcl))
    ph.check_finish(ph.rescon_finish_ref(bits, 4096, rcl, lcl), ph.rescon_finish_ref(bits, 4096, rcl, lcl))
    words = np.random.default_rng(2).integers(0, 1 << 32, (2, 65), dtype=np.uint64).astype(np.uint32)
    base = np.arange(10).reshape(2, 5)
    assert not np.array_equal(ph.hbond_finish_ref(words, base, "tail_dropped"), ph.hbond_finish_ref(words, base))


# ---- 5. pose_transform ---------------------------------------------------------------------------------------------------------------------------
def test_pose_restatement_agrees_with_mpmath_to_the_measured_figure():
    cpu, gate = ph.pose_gate()
    print(f"pose_transform: numpy restatement against mpmath {cpu:.3g}, the device's gate {gate:.3g}")
    assert 0.0 < cpu <= 8 * 2.0 ** -53, "a few roundings of entries of size 1"
    assert gate == 8.0 * cpu
    rots = ph.pose_rotations()
    assert len(rots) == 49 and (rots[0] == 0).all()
    T = ph.pose_T(rots, np.zeros_like(rots))
    assert (T[0, :9] == np.eye(3).reshape(-1)).all()
    ang = np.sqrt((ph.f64(rots) ** 2).sum(1))
    assert (ang < 1e-6).sum() >= 9 and ((ang > 1e-6) & (ang < 1.2e-6)).sum() >= 4, "both sides of the small-angle branch"
    # a proper rotation to rounding, whatever the angle
    R = T[:, :9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-15
    rot, tr = ph.nonfinite_poses()
    assert not ph.finite_poses(ph.pose_T(rot, tr)).any(), "every non-finite input gives a T that walk_front rejects"


# ---- interface energy and pair potential ---------------------------------------------------------------------------------------------------------
def test_iface_restatement_agrees_with_the_definition():
    """ifenergy.interface_energy poses with `@ R.T`: r2 moves by a few ulp, so a pair within 1e-3 A of the cutoff may fall either way
    and a term may round to the neighbouring quantum."""
    from dfmdock_amd import ifenergy as IE
    rec, lig, cen, rot, tr = ph.generic_atoms(0)
    name, c, par = ph.iface_cases()[0]
    want = IE.interface_energy(rec, par.rec_par, lig, par.lig_par, cen, rot, tr, *par.args, per_atom=True)
    ref = ph.iface_ref(c.fr, c.T, par)
    with np.errstate(invalid="ignore"):
        border = (np.abs(np.sqrt(ref["r2"]) - float(par.cutoff)) < BORDER).sum((1, 2))
    assert border.sum() <= BORDER_CAP * ref["r2"].size and ref["tot"][:, 3].sum() > 10000
    assert (np.abs(want["n_pairs"] - ref["tot"][:, 3]) <= border).all()
    for k, col in (("rep_q", 0), ("att_q", 1), ("elec_q", 2)):
        slack = ref["tot"][:, 3] + border * (1 << 20)      # a quantum per pair, a kcal/mol per border pair
        assert (np.abs(want[k] - ref["tot"][:, col]) <= slack).all(), k
    assert ref["soft_pairs"] > 0 and ref["clamped_pairs"] > 0, "the soft-core branch and the elec_min_dist clamp are taken"


def test_pairpot_restatement_agrees_with_the_definition():
    from dfmdock_amd import pairpot as PP
    rec, lig, cen, rot, tr = ph.generic_atoms(0)
    for name, c, pot in ph.pairpot_cases()[:6]:
        want = PP.pair_potential(rec, pot.rec_type, lig, pot.lig_type, cen, rot, tr, pot.edges, pot.table, per_atom=True, counts=True)
        ref = ph.pairpot_ref(c.fr, c.T, pot)
        with np.errstate(invalid="ignore"):
            d = np.sqrt(ref["r2"])
            border = sum((np.abs(d - float(e)) < 1e-9).sum() for e in pot.edges)
        assert border == 0, "no pair of the generic case within 1e-9 A of an edge: the definition must agree exactly"
        assert np.array_equal(want["energy_q"], ref["tot"][:, 0]) and np.array_equal(want["n_pairs"], ref["tot"][:, 1]), name
        assert np.array_equal(want["lig_q"], ref["lig_q"]) and np.array_equal(want["counts"], ref["counts"]), name
        assert ref["tot"][:, 1].sum() > 10000 and (ref["r2"] < pot.e2[0]).sum() > 100, "pairs inside, pairs below the first edge"
        assert pot.top == {1: 1, 2: 2, 3: 2, 30: 16, 63: 32, 64: 64}[pot.NB]


def test_iface_and_pairpot_edge_cases_and_mutants():
    cases = dict((n, (c, p)) for n, c, p in ph.iface_cases())
    c5, p5 = cases["ties cutoff 5"]
    c5u, p5u = cases["ties cutoff 5 + 1 ulp"]
    r5, r5u = ph.iface_ref(c5.fr, c5.T, p5), ph.iface_ref(c5u.fr, c5u.T, p5u)
    on = int((r5["r2"][0] == 25.0).sum())
    assert on >= 3 and r5u["tot"][0, 3] - r5["tot"][0, 3] == on and (r5["r2"] == 0.0).any()
    with pytest.raises(AssertionError):      # mutant `<=` at the cutoff: rejected on 'ties cutoff 5'
        ph.check_iface(ph.iface_ref(c5.fr, c5.T, p5, "le"), r5, c5.fr, c5.front[0], per_atom=False)
    cl, pl = cases["limits"]
    with pytest.raises(AssertionError):      # mutant without the elec_min_dist clamp: rejected on 'limits'
        ph.check_iface(ph.iface_ref(cl.fr, cl.T, pl, "no_elec_clamp"), ph.iface_ref(cl.fr, cl.T, pl), cl.fr, cl.front[0], per_atom=False)
    cn, pn = cases["negative sums"]
    rn = ph.iface_ref(cn.fr, cn.T, pn)
    assert (rn["tot"][:-1, 1] < 0).all() and (rn["tot"][:-1, 2] < 0).all()
    pots = dict((n, (c, p)) for n, c, p in ph.pairpot_cases())
    for lo in (0, 3):
        c, pot = pots[f"integer edges {lo} .. 8"]
        ref = ph.pairpot_ref(c.fr, c.T, pot)
        for k in range(lo, 9):      # pairs AT every edge: bin k - lo, and none at the last
            at = ref["r2"] == float(k * k)
            assert at.any(), k
            assert (ref["pair"][at] == (k < 8)).all() and (k == 8 or (ref["k"][at] == k - lo).all())
        with pytest.raises(AssertionError):      # mutant: bin search off by one at an edge, rejected on 'integer edges'
            ph.check_pairpot(ph.pairpot_ref(c.fr, c.T, pot, "bin_off_by_one"), ref, c.fr, c.front[0], per_atom=False)
    c3, pot3 = pots["integer edges 3 .. 8"]
    assert (ph.pairpot_ref(c3.fr, c3.T, pot3)["r2"] < 9.0).any(), "pairs below the first edge"
    c, pot = pots["NB 2 T 256"]
    assert pot.T == 256 and np.abs(pot.table_q).max() == 1 << 30


# ---- hydrogen bonds ------------------------------------------------------------------------------------------------------------------------------
def test_hbond_restatement_agrees_with_the_definition_and_rejects_its_mutant():
    from dfmdock_amd import hbonds as HB
    cases = {c[0]: c for c in ph.hbond_cases()}
    for name in ("c2 0", "Rc 33"):
        _, hb, T, rot, tr = cases[name]
        want = HB.hbonds(hb.rec, hb.lig, hb.fr.center32, rot, tr, 3.5, 90.0, 4.0, per_atom=True)
        ref = ph.hbond_ref(hb, T)
        with np.errstate(invalid="ignore"):
            border = sum((np.abs(np.sqrt(ref["r2"]) - cut) < BORDER).sum((1, 2)) for cut in (3.5, 4.0))
        assert border.sum() <= BORDER_CAP * 2 * ref["r2"].size
        assert (np.abs(want["n_salt_atoms"] - ref["tot"][:, 3]) <= border).all() and (np.abs(want["n_hbond"] - ref["tot"][:, :3].sum(1)) <= border).all()
        # a borderline pair moves one bond or one salt pair: one count of a kind, at most one bridge, one entry of each per-atom array
        assert (np.abs(want["hb_kind"] - ref["tot"][:, :3]).sum(1) <= border).all() and (np.abs(want["n_salt"] - ref["tot"][:, 4]) <= border).all()
        for k in ("rec_hb", "rec_sb", "lig_hb", "lig_sb"):
            assert (np.abs(want[k].astype(np.int64) - ref[k]).sum(1) <= border).all(), (name, k)
        quiet = border == 0      # no pair within 1e-3 A of either cutoff: the definition's every number
        assert quiet.any() or name != "c2 0"
        for k, mine in (("hb_kind", ref["tot"][:, :3]), ("n_salt", ref["tot"][:, 4]), ("n_salt_atoms", ref["tot"][:, 3])) + tuple((k, ref[k]) for k in ("rec_hb", "rec_sb", "lig_hb", "lig_sb")):
            assert np.array_equal(np.asarray(want[k])[quiet], mine[quiet]), (name, k)
        assert ref["tot"][:, :3].sum(0).min() > 0 and ref["tot"][:, 3].sum() > 0 and ref["tot"][:, 4].sum() > 0, "kinds 0, 1, 2, salt pairs, salt bridges"
    assert cases["Rc 0"][1].Rc == 0 and cases["Rc 0"][1].Wc == 0 and cases["Lc 0"][1].Lc == 0 and cases["Rc 33"][1].Rc == 33 and cases["Rc 33"][1].Wc == 2
    assert ph.hbond_ref(cases["Rc 33"][1], cases["Rc 33"][2])["bits"][:, :, 1].any(), "the 33rd charged residue is met"
    _, hb, T, _, _ = cases["c2 0.97"]
    ref = ph.hbond_ref(hb, T)
    assert (ref["bond"] & (ref["uu"] == 0.0)).any(), "a bond through an antecedent coincident with its atom (du = 0, uu = 0)"
    with pytest.raises(AssertionError):      # mutant `du < 0`: rejected on 'c2 0.97'
        ph.check_hbond(ph.hbond_ref(hb, T, "angle_lt"), ref, hb, ph.walk_front(hb.fr, T)[0], per_atom=False)
    roles = {(int(a) & 15, int(b) & 15) for a in hb.lig["role"] for b in hb.rec["role"]}
    assert len(roles) >= 200, "every role combination on both sides"


# ---- buried surface ------------------------------------------------------------------------------------------------------------------------------
def test_surface_restatement_agrees_with_the_definition_and_the_cases_hold_their_claims():
    from dfmdock_amd import surface as SF
    cases = {c[0]: c for c in ph.surface_cases()}
    name, sf, T, rot, tr = cases["host exposure K 128"]
    rec, lig, cen, _, _ = ph.generic_atoms(0)
    assert np.array_equal(ph.sphere_dirs(128), np.asarray(SF.sphere_points(128), np.float32))
    assert np.array_equal(ph.exposure_ref(rec, sf.rec_radius, sf.probe, sf.dirs), SF.exposure(rec, sf.rec_radius, 1.4, 128))
    assert np.array_equal(ph.unpack_bits(sf.lig_exp, 128), SF.exposure(lig, sf.lig_radius, 1.4, 128))
    want = SF.bsa(rec, sf.rec_radius, lig, sf.lig_radius, cen, rot, tr, 1.4, 128, per_atom=True)
    ref = ph.surface_ref(sf, T)
    # `@ R.T` moves a posed atom by 1e-15 A: a point within 1e-9 A of a sphere may fall either way - none does here, or a few
    diff = np.abs(want["lig_buried"].astype(np.int64) - ref["lig_buried"]).sum() + np.abs(want["rec_buried"].astype(np.int64) - ref["rec_buried"]).sum()
    total = int(ref["lig_buried"].sum() + ref["rec_buried"].sum())
    assert total > 5000 and diff <= BORDER_CAP * total, (diff, total)
    status = ph.walk_front(sf.fr, T)[0]
    assert ((ref["rec_bur"] != 0).any(2).sum(1) > 0).any() and (status[:-1] == 0).all(1).any(), "rec_bur is set by three blocks of one pose"
    for K in (64, 128, 192, 256):
        s = cases[f"K {K} sixteen classes"][1]
        assert s.G == K // 64 and len(s.values) == 16 and set(s.rec_class) == set(range(16))
    assert [cases[f"Ar {n}"][1].fr.Ar for n in (1, 255, 256, 257)] == [1, 255, 256, 257]
    for n, s_, T_, _, _ in ph.surface_cases():      # no point within 1e-9 A of the sphere it is tested against: `d < R` is safe bitwise
        assert ph.surface_ref(s_, T_)["nearest"] > 1e-9, n
    _, d, dT, _, _ = cases["dense clump"]
    assert ph.surface_ref(d, dT)["n_close"].max() > 1000, "a block whose queue of 512 drains several times"
    # a mutant: the receptor's radius without its probe (rejected on 'host exposure K 128')
    bad = ph.Surface(rec, sf.rec_radius, lig, sf.lig_radius, cen, 1.4, 128, sf.rec_exp, sf.lig_exp)
    bad.probe = 1.3
    with pytest.raises(AssertionError):
        ph.check_surface(ph.surface_ref(bad, T), ref, sf, status)


def test_shim_refuses_bad_indices_of_the_other_four_walks(shim):
    """Types at or above T, a slab offset that is not type * T * NB, NB = 65, a wrong `top`, e2 without its +inf tail, a charged-residue
    index at or above Rc / Lc, a radius class of 16, G = 5, short parameter arrays: hipErrorInvalidValue on the CPU side of the record."""
    seen = {}

    def record(op, bufs, check=True, **sc):      # the harness's own call records, checked and not run
        seen[op] = (bufs, sc)
        raise LookupError
    run, shim.run = shim.run, record
    try:
        _, c, par = ph.iface_cases()[0]
        _, cp, pot = ph.pairpot_cases()[3]
        _, hb, Th, _, _ = ph.hbond_cases()[0]
        _, sf, Ts, _, _ = ph.surface_cases()[0]
        for call in (lambda: shim.iface(c.fr, c.T, par), lambda: shim.pairpot(cp.fr, cp.T, pot), lambda: shim.hbond(hb, Th), lambda: shim.surface(sf, Ts)):
            with pytest.raises(LookupError):
                call()
    finally:
        shim.run = run

    def check(op, **change):
        bufs, sc = (dict(v) for v in seen[op])
        for k, v in change.items():
            (sc if k in sc else bufs)[k] = v
        return shim.check_only(op, bufs, **sc)
    for op in seen:
        assert check(op) == ph.HIP_SUCCESS, op
    bufs = seen["iface"][0]
    assert check("iface", rec_par=bufs["rec_par"][:-1]) == check("iface", lig_par=bufs["lig_par"][:-1]) == ph.HIP_INVALID_VALUE
    assert check("iface", tot=ph.Out(np.int64, 4 * len(c.T) - 1)) == check("iface", lig_index=c.fr.lig_index[::-1][:-1]) == ph.HIP_INVALID_VALUE
    bufs = seen["pairpot"][0]
    rp = bufs["rec_par"].view(np.int32).copy()
    bad_type, bad_slab = rp.copy(), rp.copy()
    bad_type[5, 0], bad_slab[5, 1] = pot.T, rp[5, 1] + 1
    bad_lt = bufs["lig_type"].copy()
    bad_lt[-1] = pot.T
    e2 = pot.e2.copy()
    e2[100] = 1e30
    for change in (dict(rec_par=bad_type.view(np.float32)), dict(rec_par=bad_slab.view(np.float32)), dict(lig_type=bad_lt), dict(e2=e2), dict(e2=pot.e2[:127]),
                   dict(NB=65), dict(NB=pot.NB + 1), dict(top=pot.top * 2), dict(top=pot.top // 2), dict(NT=pot.T + 1), dict(table_q=pot.table_q.reshape(-1)[:-1]),
                   dict(lo2=0.0), dict(counts=ph.Out(np.int32, len(cp.T) * pot.T * pot.T * pot.NB - 1))):
        assert check("pairpot", **change) == ph.HIP_INVALID_VALUE, list(change)
    bufs = seen["hbond"][0]
    rec = bufs["rec"].view(np.int32).copy()
    charged = np.where(rec[:, 3] & 12)[0][0]
    rec[charged, 3] = (rec[charged, 3] & 255) | (hb.Rc << 8)
    lig = bufs["lig"].view(np.int32).copy()
    lig[np.where(lig[:, 3] & 12)[0][0], 3] |= hb.Lc << 8
    role = bufs["rec"].view(np.int32).copy()
    role[0, 3] |= 64
    for change in (dict(rec=rec.view(np.float32)), dict(lig=lig.view(np.float32)), dict(rec=role.view(np.float32)), dict(Wc=hb.Wc + 1), dict(Rc=hb.Rc + 32),
                   dict(rec_ante=bufs["rec_ante"][:-1]), dict(rec_index=np.zeros(hb.fr.Ar, np.int32)), dict(bits=ph.Out(np.uint32, len(Th) * hb.Lc * hb.Wc - 1))):
        assert check("hbond", **change) == ph.HIP_INVALID_VALUE, list(change)
    bufs = seen["surface"][0]
    cls = bufs["rec_class"].copy()
    cls[3] = 16
    for change in (dict(G=5), dict(G=0), dict(G=sf.G + 1), dict(rec_class=cls), dict(lig_class=np.full(sf.fr.Al, -1, np.int32)), dict(dirs=sf.dirs[:-1]),
                   dict(rec_exp=bufs["rec_exp"][:-1]), dict(rec_bur=ph.Out(np.uint64, len(Ts) * sf.fr.Ar * sf.G - 1)), dict(tot=ph.Out(np.int32, 32 * len(Ts) - 1))):
        assert check("surface", **change) == ph.HIP_INVALID_VALUE, list(change)


# ---- the density fit: density_ref is the definition, the shim's checks, the power of the comparisons, the conditions on the inputs -------------
def test_shim_links_the_density_launchers(shim):
    und = kh.exported_symbols(shim.path, False)
    assert "launch_density_pose" in und and "launch_densityERK" in und


def all_density_launches():
    return [L for shape in ph.DENSITY_SHAPES for C in (1, 2, 3, 4) for L in ph.density_launches(shape, C)]


def test_density_restatement_agrees_with_the_definition():
    """density_ref on T = pose_T(rot, tr) equals dfmdock_amd.density.density on every array, for every launch of test_density_exact and
    for the poses of the non-finite, all-outside and limit cases that come from rot / tr; the channels at or above C are left out."""
    n = 0
    for dc, rot, tr, T, base in all_density_launches():
        ref, want = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, dc["C"]), ph.density_definition(dc, rot, tr)
        C = dc["C"]
        assert np.array_equal(ref["tot"][:, :C], want["sum_q"]) and not ref["tot"][:, C:4].any()
        assert np.array_equal(ref["tot"][:, 4], want["n_inside"]) and np.array_equal(ref["tot"][:, 5], want["n_above"])
        assert np.array_equal(ref["atom_q"], want["atom_q"])
        n += ref["inside"].size
    assert n == 8 * 323 * 8
    # T as exact doubles: the identity and zero rotation vectors are the same pose to the definition
    dc, T = ph.sum_limit_density_case()
    want = ph.density_definition(dc, np.zeros((2, 3), np.float32), T[:, 9:].astype(np.float32))
    ref = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, dc["C"])
    assert np.array_equal(ref["tot"][:, :2], want["sum_q"]) and np.array_equal(ref["atom_q"], want["atom_q"])
    for dc, T in ((ph.ties_density_case()[0], ph.ties_density_case()[2]), (ph.ties_density_case()[1], ph.ties_density_case()[2])):
        want = ph.density_definition(dc, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
        assert np.array_equal(ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, 1)["atom_q"], want["atom_q"])
    # a pose that is not finite: zeros in the definition, nothing added in the restatement
    dc, rot, tr, T, _ = ph.density_launches((3, 5, 4), 2)[11]
    ref = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], ph.nonfinite_density_T(T[0], T[1]), 2)
    assert not ref["tot"][1:37].any() and not ref["atom_q"][1:37].any() and ref["tot"][0, 4] > 0 and ref["tot"][37, 4] > 0


def test_density_inputs_hold_what_they_claim():
    """The conditions the GPU tests rely on, none excused: the planted transforms are exact (the restatement's inside decision equals the
    rational one for all 4 x 119 pairs; every face atom has its two fp32 neighbours on either side of the decision; upper faces are
    outside, lower faces inside, u = -1/2 outside); every generic launch has atoms inside and outside, on both sides of the threshold; the
    limit case's terms are 2^37."""
    dc, T, labels = ph.planted_density_case()
    ref = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, dc["C"])
    exact = ph.density_inside_exact(dc, T)
    assert np.array_equal(ref["inside"], exact)
    assert set(np.unique(T[:, :9]).tolist()) == {-1.0, 0.0, 1.0}
    own = {}
    for a, (p, kind) in enumerate(labels):
        own.setdefault((p, kind), []).append(bool(exact[p, a]))
    for p in range(4):
        assert own[(p, "lower")] == [True] * 3 and own[(p, "upper")] == [False] * 3 and own[(p, "neg_half")] == [False] * 3, p
        for face, inward in (("lower", True), ("upper", False)):
            up, down = own[(p, face + "+")], own[(p, face + "-")]
            assert all(a != b for a, b in zip(up, down)), (p, face)      # one ulp either way decides
        assert sum(own[(p, "node")]) == 4 and len(own[(p, "node")]) == 8      # the nodes on an upper face are outside
    assert not exact[:, -3:].any()      # 1e30, 3e38
    assert exact.sum(1).min() >= 13 and (~exact).sum(1).min() >= 50      # every pose sees the other poses' atoms on both sides too
    for dc, rot, tr, T, base in all_density_launches():
        ref = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, dc["C"])
        if dc["Al"] >= 63:
            assert (ref["inside"].sum(1) > 0).all() and (~ref["inside"]).sum(1).min() > 0
            assert 0 < ref["tot"][:, 5].sum() < ref["tot"][:, 4].sum()
    mz, Tz = ph.minus_zero_density_case()
    with np.errstate(all="ignore"):
        u = (Tz[0, 9] - mz["geo"][0]) / mz["geo"][3]
    assert u == 0.0 and np.signbit(u) and ph.density_ref(mz["grid4"], mz["geo"], mz["lig4"], Tz, 1)["inside"].all()
    assert not ph.density_inside_exact(mz, Tz).any()      # the exact quotient is negative: the IEEE comparison is the definition
    dc, T = ph.limit_density_case()
    assert len(T) == 65535 and dc["Al"] == 1


DENSITY_MUTANT_CASE = {"le_upper": "planted", "trunc": "planted", "fx_f32": "generic 130", "y_before_x": "rounded", "stride_swapped": "generic 130",
                       "half_away": "half", "contracted": "rounded", "channel1_above": "generic 130", "lanes_past_Al": "generic 65", "tot_stored": "generic 130"}


@pytest.mark.parametrize("mutant", sorted(ph.DENSITY_MUTANTS))
def test_density_mutants_are_rejected(mutant):
    """Each seeded mutant of density_ref is rejected by the comparison named for it in DENSITY_MUTANTS, on inputs the GPU file launches."""
    half, rounded, Tt = ph.ties_density_case()
    L = ph.density_launches((3, 5, 4), 2)
    planted = ph.planted_density_case()
    cases = {"planted": (planted[0], planted[1], ph.density_base(4)), "half": (half, Tt, ph.density_base(1)), "rounded": (rounded, Tt, ph.density_base(1)),
             "generic 65": (L[11][0], L[11][3], L[11][4]), "generic 130": (L[14][0], L[14][3], L[14][4])}
    dc, T, base = cases[DENSITY_MUTANT_CASE[mutant]]
    assert (dc["Al"], len(T)) in ((65, 5), (130, 5), (119, 4), (5, 1), (8, 1))
    ref = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, dc["C"], base=base)
    good = ph.density_compare(dict(tot=np.concatenate([ref["tot"], base[len(T):]]), atom_q=ref["atom_q"]), ref, len(T), dc["Al"], base=base)
    assert not any(good.values())
    bad = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, dc["C"], base=base, mutant=mutant)
    cmp = ph.density_compare(dict(tot=np.concatenate([bad["tot"], base[len(T):]]), atom_q=bad["atom_q"]), ref, len(T), dc["Al"], base=base)
    assert cmp[ph.DENSITY_MUTANTS[mutant]] > 0, (mutant, cmp)


def test_density_compare_sees_writes_past_the_launch():
    dc, rot, tr, T, base = ph.density_launches((2, 2, 2), 1)[4]
    ref = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, 1, base=base)
    tot, aq = np.concatenate([ref["tot"], base[len(T):]]), np.concatenate([ref["atom_q"].reshape(-1), np.full(2 * dc["Al"], ph.MARKER)])
    assert ph.density_compare(dict(tot=tot, atom_q=aq), ref, len(T), dc["Al"], base=base)["past"] == 0
    tot[-1, 4] += 1
    aq[len(T) * dc["Al"]] = 0
    assert ph.density_compare(dict(tot=tot, atom_q=aq), ref, len(T), dc["Al"], base=base)["past"] == 2


def _density_call(dc, poses, **change):
    """The record of one density launch on `poses` [P,12], with scalars or buffers replaced by `change`."""
    P = len(poses)
    bufs = dict(grid=dc["grid4"], geo=dc["geo"], lig=dc["lig4"], T=poses, tot=ph.Out(np.int64, P * 6), atom_q=ph.Out(np.int64, P * max(dc["Al"], 1)))
    sc = dict(nx=dc["dims"][0], ny=dc["dims"][1], nz=dc["dims"][2], n=P, Al=dc["Al"], C=dc["C"])
    for k, v in change.items():
        (sc if k in sc else bufs)[k] = v
    return bufs, sc


def test_shim_checks_of_the_density_launch(shim):
    """One malformed record per condition, refused without touching a device; n, nx / ny / nz < 2 and Al < 1 pass the shim (they are the
    launcher's to refuse) as long as the arrays hold max(., 2) nodes per axis, max(Al, 1) atoms and max(n, 0) poses."""
    dc, rot, tr, T, _ = ph.density_launches((3, 5, 4), 2)[5]      # Al = 63, n = 5
    b, s = _density_call(dc, T)
    assert shim.check_only("density", b, **s) == ph.HIP_SUCCESS
    geo = lambda k, v: dict(geo=np.concatenate([dc["geo"][:k], [v], dc["geo"][k + 1:]]))
    bad = [dict(grid=dc["grid4"].reshape(-1)[:-1]), dict(lig=dc["lig4"][:-1]), dict(geo=dc["geo"][:-1]), dict(T=T[:-1]), dict(tot=ph.Out(np.int64, 29)),
           dict(atom_q=ph.Out(np.int64, 5 * 63 - 1)), dict(tot=np.zeros(30, np.int64)), dict(grid=ph.Out(np.float32, init=dc["grid4"])),
           geo(0, np.nan), geo(7, np.inf), geo(9, -np.inf), geo(4, 0.0), geo(3, -1.5), geo(10, 4.0), geo(11, 3.0), geo(12, 3.0), geo(13, np.nan),
           dict(nx=5), dict(ny=4), dict(nz=4), dict(n=6), dict(Al=64), dict(C=0), dict(C=5)]
    for change in bad:
        b, s = _density_call(dc, T, **change)
        assert shim.check_only("density", b, **s) == ph.HIP_INVALID_VALUE, list(change)
        r = shim.run("density", b, check=False, **s)
        assert r["err"] == ph.HIP_INVALID_VALUE and all(not r[k + "_guard"][0].any() for k, v in b.items() if isinstance(v, ph.Out)), list(change)
    small = ph.density_case((2, 2, 2), 2, 3)
    T2 = T[:2]
    for change in (dict(n=0), dict(Al=0), dict(nx=1, geo=np.concatenate([small["geo"][:10], [0.0], small["geo"][11:]])),
                   dict(nz=1, geo=np.concatenate([small["geo"][:12], [0.0], small["geo"][13:]]))):
        b, s = _density_call(small, T2, **change)
        assert shim.check_only("density", b, **s) == ph.HIP_SUCCESS, list(change)
    b, s = _density_call(small, np.tile(T2[:1], (65536, 1)), atom_q=None)
    assert shim.check_only("density", b, **s) == ph.HIP_SUCCESS
    rot, tr = ph.pose_inputs(5)
    ok = dict(rot=rot, tr=tr, T=ph.Out(np.float64, 60), tot=ph.Out(np.int64, 30))
    assert shim.check_only("pose_density", ok, n=5) == ph.HIP_SUCCESS
    for change in (dict(tot=ph.Out(np.int64, 29)), dict(tr=tr[:-1]), dict(T=ph.Out(np.float64, 59))):
        assert shim.check_only("pose_density", dict(ok, **change), n=5) == ph.HIP_INVALID_VALUE, list(change)
