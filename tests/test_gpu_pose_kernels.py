"""The rigid-pose kernels launch by launch - all sixteen launchers of the six families that share dfm_posewalk.h (pose_transform,
walk_front, walk_rows): sterics, buried surface, interface energy, residue contacts, hydrogen bonds, pair potential - driven through
tests/kernels/pose_harness.hip on small host arrays with guard bands around every device block, against the float64 restatements of
tests/pose_harness.py by brute force over all P x Al x Ar pairs (tests/test_pose_harness_cpu.py shows that the numpy frame is the
host's, that the restated walk finds exactly the brute force's pairs and that the comparisons used here reject its seeded mutants),
and the same poses through the public creators and calls; and the density fit's two launchers (k_density_pose with the other six pose
kernels, k_density - a gather from a grid, no walk - alone on T of exact doubles, on a prefilled tot and a marked atom_q, against
pose_harness.density_ref, integer for integer).

What is exact and what carries a gate (pose_harness.py states each):
  exact (bitwise)   every count, per-atom count, bitmap, total, degree and exit counter; the translation entries of T; rot = 0 gives the
                    identity; what a non-finite pose leaves of itself (its initial values) and of its neighbours (what they are
                    without it); a launcher's refusal leaves every block as it was.  No pair near a cutoff is excused: T is fed as
                    the kernel reads it, so the restatement rounds like the kernel.
  rotation of T     8 x the error of the float64 numpy restatement of pose_transform against mpmath on the same inputs.
  min_dist          1 ulp.
The figures go to $DFM_POSE_PROFILE/pose_kernels_gpu.txt when that variable names a directory (profiles/pose_kernels.txt holds the
MI355X figures).
"""
import os
import time

import numpy as np
import pytest

import pose_harness as ph

pytestmark = pytest.mark.gpu

FIG = {"T rotation error, device": 0.0}
COUNTS = {"min_dist not bitwise": 0, "min_dist compared": 0}
EXITS = {}


def tally(name, decisions):
    COUNTS[f"decisions {name}"] = COUNTS.get(f"decisions {name}", 0) + int(decisions)


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    t0 = time.time()      # the module's tests run one after the other: from here to the teardown is the file's wall time, shim build included
    harness = ph.Harness(ph.compile_shim(tmp_path_factory.mktemp("pose_harness_gpu")))
    yield harness
    out = os.environ.get("DFM_POSE_PROFILE")
    if out:
        cpu, gate = ph.pose_gate()
        dev = FIG["T rotation error, device"]
        with open(os.path.join(out, "pose_kernels_gpu.txt"), "w") as f:
            f.write(f"T rotation entries, largest absolute error against mpmath: numpy restatement {cpu:.4g}, device {dev:.4g}, "
                    f"ratio {dev / cpu:.3g}, gate {gate:.4g} (8 x the restatement's)\n")
            f.write("".join(f"{k} {v}\n" for k, v in sorted(COUNTS.items())))
            f.write("exits per case (sphere test, box test, walked):\n" + "".join(f"  {k}: {v}\n" for k, v in EXITS.items()))
            f.write(f"wall time of the file {time.time() - t0:.1f} s\n")


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


# ---- the pose kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65])
def test_pose_kernels(h, n):
    """All seven launch_*_pose on every finite rotation of pose_harness.pose_rotations: translation exact, rotation within the gate, rot = 0
    the identity, the totals zeroed as each header comment promises, nothing past n written, the seven T bitwise the same."""
    rot, tr = ph.pose_inputs(n)
    first = None
    for op in ph.POSE_OPS:
        out = h.pose(op, rot, tr)
        FIG["T rotation error, device"] = max(FIG["T rotation error, device"], ph.check_pose(out, op, rot, tr))
        first = out["T"] if first is None else first
        assert out["T"].tobytes() == first.tobytes(), f"{op}: T differs from launch_sterics_pose's"


def test_pose_kernel_single_rotations(h):
    """n = 1 on each rotation in turn would be 49 launches; one launch of 49 poses is test_pose_kernels' n = 64.  Here, each alone in
    a launch of one: the identity, |rot| = 9.9e-7 (the small-angle branch), the fp32 nearest 1e-6 (just below the threshold of 1e-6 once
    widened: still the branch) and 1.1e-6 (the other side)."""
    rots = ph.pose_rotations()
    for k in (0, 5, 9, 13):
        rot, tr = rots[k:k + 1], np.float32([[1.5, -2.25, 1e4]])
        ph.check_pose(h.pose("pose_rescon", rot, tr), "pose_rescon", rot, tr)


def test_non_finite_pose_inputs(h):
    """NaN, +inf, -inf in each of the six input positions, through pose kernel and main launch with ordinary poses between them: every
    such T is one walk_front rejects - the pose keeps the pose kernel's 0, 0, +inf and the marker on every atom - and the ordinary poses
    are bitwise the reference on the device's own T."""
    g = ph.generic_case(0)
    brot, btr = ph.nonfinite_poses()
    rot, tr = np.concatenate([g.rot[:1], brot, g.rot[1:3]]), np.concatenate([g.tr[:1], btr, g.tr[1:3]])
    for op in ph.POSE_OPS:
        ph.check_pose(h.pose(op, rot, tr), op, rot, tr)
    out = h.sterics(g.fr, rot=rot, tr=tr)
    bad = np.arange(1, 19)
    assert not ph.finite_poses(out["T"][bad]).any()
    assert (out["n_clash"][bad] == 0).all() and (out["n_contact"][bad] == 0).all() and np.isposinf(out["min_dist"][bad]).all()
    assert (out["lig_contact"][bad] == ph.MARKER).all() and (out["lig_clash"][bad] == ph.MARKER).all()
    c = ph.Case("chain", g.fr, out["T"])
    ph.check_sterics(out, c.ref, c.front[0])
    assert c.ref["n_contact"][[0, 19, 20]].min() > 0


# ---- the shared walk, through launch_sterics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ph.walk_cases(), ids=repr)
def test_walk_exact(h, case):
    """Every integer bitwise, min_dist to 1 ulp, the exits, the per-atom outputs written exactly on the atoms of the walked blocks (the
    marker everywhere else), totals prefilled with a base come back as base + count; without per-atom outputs the same totals."""
    base = (1000, -5)
    out = h.sterics(case.fr, case.T, base=base)
    n, loose = ph.check_sterics(out, case.ref, case.front[0], base=base)
    tally("k_sterics", n)
    COUNTS["min_dist not bitwise"] += loose
    COUNTS["min_dist compared"] += len(case.T)
    st = case.front[0]
    EXITS[case.name] = (int((st == 1).sum()), int((st == 2).sum()), int((st == 0).sum()))
    bare = h.sterics(case.fr, case.T, per_atom=False)
    ph.check_sterics(bare, case.ref, case.front[0], per_atom=False)
    assert bare["min_bits"].tobytes() == out["min_bits"].tobytes()


def test_grids_that_are_not_the_hosts_give_the_same_integers(h):
    """edge = reach / 2 and 2.5 reach, a padded box, one cell, the ligand in random order, spheres of twice the radius: every integer
    output and min_dist equal the host-shaped frame's, bitwise."""
    g = ph.generic_case(0)
    want = h.sterics(g.fr, g.T)
    for v in ph.grid_variants():
        got = h.sterics(v.fr, v.T)
        for k in ("n_clash", "n_contact", "min_bits"):
            assert got[k].tobytes() == want[k].tobytes(), (v, k)
        walked = (got["lig_contact"] != ph.MARKER) & (want["lig_contact"] != ph.MARKER)
        for k in ("lig_clash", "lig_contact"):
            assert np.array_equal(got[k][walked], want[k][walked]), (v, k)
            assert (np.where(got[k] == ph.MARKER, 0, got[k]) == np.where(want[k] == ph.MARKER, 0, want[k])).all(), (v, k)


@pytest.mark.parametrize("case", ph.far_cases(), ids=repr)
def test_far_from_the_origin_no_pair_is_missing(h, case):
    """(3000, -2500, 1800) with reach 5 and (20000, -20000, 20000) with reach 3, where pose_slack is above its floor: at least 100 pairs
    in the last 1e-2 A below the contact cutoff, and the fp32 reject drops none of them (test_walk_exact holds every count; this names
    the claim)."""
    assert ph.last_hundredth(case) >= 100
    out = h.sterics(case.fr, case.T)
    np.testing.assert_array_equal(out["n_contact"], case.ref["n_contact"])
    np.testing.assert_array_equal(out["lig_contact"], case.ref["lig_contact"])


def test_non_finite_entries_of_T(h):
    """Each of the 12 entries of a pose's T NaN, then +inf, in one launch of 24 + 2: those poses keep their prefill, the two ordinary
    ones are the reference."""
    c = ph.nonfinite_T_case()
    out = h.sterics(c.fr, c.T, base=(3, 4))
    assert (out["n_clash"][1:25] == 3).all() and (out["n_contact"][1:25] == 4).all() and (out["min_bits"][1:25] == ph.INF_BITS).all()
    assert (out["lig_contact"][1:25] == ph.MARKER).all()
    assert out["n_contact"][0] == out["n_contact"][25] == c.ref["n_contact"][0] + 4 and out["min_bits"][0] == out["min_bits"][25]
    assert (out["exits"] == 0).all()


@pytest.mark.parametrize("n", [0, 65536])
def test_refusals_leave_every_block_alone(h, n):
    c = ph.size_cases()[0]
    T = np.tile(c.T[:1], (max(n, 1), 1))
    out = h.sterics(c.fr, T, base=(11, 12), n=n, check=False)
    assert out["err"] == ph.HIP_INVALID_VALUE
    assert (out["n_clash"] == 11).all() and (out["n_contact"] == 12).all() and (out["min_bits"] == ph.INF_BITS).all()
    assert (out["lig_clash"] == ph.MARKER).all() and (out["lig_contact"] == ph.MARKER).all() and (out["exits"] == 0).all()
    for k in ("n_clash", "n_contact", "min_bits", "lig_clash", "lig_contact", "exits"):
        assert ph.guards_intact(out, k), k


def test_min_dist_over_three_blocks(h):
    """A pose whose three blocks all walk and all hold a contact: the atomic minimum has three contenders."""
    g = ph.generic_case(0)
    out = h.sterics(g.fr, g.T)
    p = int(np.where((g.front[0] == 0).all(1))[0][0])
    assert ph.ulps(out["min_dist"][p], g.ref["min_dist"][p]) <= 1 and np.isfinite(out["min_dist"][p])


# ---- chain and public call -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_chain_and_public_call(h, model, seed):
    """Pose kernel, then main launch, on rot / tr: the results equal the reference evaluated on the device's own T, bitwise; the same rot /
    tr through engine.Model.atoms(...).sterics give the harness's results bitwise - which ties the numpy frame to the shipped host
    preparation on the GPU as well."""
    g = ph.generic_case(seed)
    out = h.sterics(g.fr, rot=g.rot, tr=g.tr)
    c = ph.Case("chain", g.fr, out["T"])
    n, loose = ph.check_sterics(out, c.ref, c.front[0])
    tally("k_sterics chain", n)
    COUNTS["min_dist not bitwise"] += loose
    COUNTS["min_dist compared"] += len(g.T)
    rec, lig, cen, rot, tr = ph.generic_atoms(seed)
    atoms = model.atoms(rec, lig, cen, ph.GENERIC["clash"], ph.GENERIC["contact"])
    try:
        api = atoms.sterics(rot, tr, per_atom=True)
        info = atoms.info()
    finally:
        atoms.close()
    assert info["n_cells"] == int(np.prod(g.fr.dims)) and info["max_cell_atoms"] == g.fr.max_cell
    for k in ("n_clash", "n_contact"):
        assert np.asarray(api[k]).tobytes() == out[k].tobytes(), k
    assert np.asarray(api["min_dist"], np.float64).tobytes() == out["min_dist"].tobytes()
    for k in ("lig_clash", "lig_contact"):      # the public call zeroes what the harness marks
        assert np.array_equal(api[k], np.where(out[k] == ph.MARKER, 0, out[k])), k


# ---- residue contacts: the bitmap, then the finish kernel alone --------------------------------------------------------------------------------
def test_rescon_bitmap_exact(h):
    """Rr = 4096 with atoms of residues 0, 31, 32, 4095; ligand atoms that meet receptor residue 31 through many atoms, consecutive
    ligand atoms of different residues meeting the same one (the `last` skip): the bitmap is the brute force's, bit for bit."""
    c = ph.rescon_case()
    bits = h.rescon(c.fr, c.T, c.Rr, c.Lr)
    want = ph.rescon_bits_ref(c.fr, c.T, c.rec_res, c.lig_res, c.Rr, c.Lr)
    np.testing.assert_array_equal(bits, want)
    tally("k_rescon", c.ref["d"].size)
    seen = np.where(ph.popcount(np.bitwise_or.reduce(want, (0, 1))) > 0)[0]
    assert {0, 1, 127} <= set(seen.tolist()), "words 0, 1 and 127 hold a contact"
    rcl, lcl = np.random.default_rng(1).integers(0, 3, c.Rr).astype(np.uint8), np.random.default_rng(2).integers(0, 3, c.Lr).astype(np.int32)
    ph.check_finish(h.rescon_finish(bits, c.Rr, rcl, lcl), ph.rescon_finish_ref(want, c.Rr, rcl, lcl))


@pytest.mark.parametrize("Rr", ph.FINISH_RR)
def test_rescon_finish_alone(h, Rr):
    """Bitmaps made in numpy (densities 0, 0.5 and all ones), never from poses: W = 1 .. 128 words (one pass, 64 / 65: the pass boundary,
    128: two full passes), Lr = 1 .. 130, random classes, degrees present and absent: all nine totals and both degree arrays against
    popcounts."""
    for Lr in ph.FINISH_LR:
        bits, rcl, lcl = ph.finish_inputs(Rr, Lr)
        ref = ph.rescon_finish_ref(bits, Rr, rcl, lcl)
        ph.check_finish(h.rescon_finish(bits, Rr, rcl, lcl), ref)
        if Lr in (1, 65):
            ph.check_finish(h.rescon_finish(bits, Rr, rcl, lcl, degrees=False), ref, degrees=False)
        tally("k_rescon_finish bits", bits.size * 32)


def test_hbond_finish_alone(h):
    """words = 0, 1, 63, 64, 65, 1000 of random bits: entry 4 is the popcount, entries 0 .. 3 keep their prefill."""
    rng = np.random.default_rng(17)
    for Lc, Wc in ph.HBOND_WORDS:
        bits = rng.integers(0, 1 << 32, (3, Lc * Wc), dtype=np.uint64).astype(np.uint32)
        base = rng.integers(-50, 50, (3, 5)).astype(np.int32)
        got = h.hbond_finish(bits, Lc, Wc, base)
        np.testing.assert_array_equal(got, ph.hbond_finish_ref(bits, base), f"words {Lc * Wc}")


# ---- interface energy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,par", ph.iface_cases(), ids=[c[0] for c in ph.iface_cases()])
def test_iface_exact(h, name, case, par):
    """tot and both per-atom outputs bitwise against the restatement: the soft-core branch, the elec_min_dist clamp, r2 = 0, sqrt_eps = 0,
    charge = 0, the limits 2 / +-4 / soft = 0.5, negative att and elec sums, r2 == cut2 (no pair) and one fp32 ulp of cutoff above it (a
    pair); tot prefilled with a base comes back as base + sum; without per-atom outputs the same totals."""
    ref = ph.iface_ref(case.fr, case.T, par)
    base = np.tile(np.int64([5, -7, 1 << 40, -3]), (len(case.T), 1))
    out = h.iface(case.fr, case.T, par, base=base)
    tally("k_iface", ph.check_iface(out, ref, case.fr, case.front[0], base=base))
    bare = h.iface(case.fr, case.T, par, per_atom=False)
    ph.check_iface(bare, ref, case.fr, case.front[0], per_atom=False)
    if name == "negative sums":
        assert (ref["tot"][:-1, 1] < 0).all() and (ref["tot"][:-1, 2] < 0).all()


# ---- pair potential ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,pot", ph.pairpot_cases(), ids=[c[0] for c in ph.pairpot_cases()])
def test_pairpot_exact(h, name, case, pot):
    """Both instantiations (counts given / null) bitwise against the restatement and agreeing on tot and lig_q: NB = 1 .. 64 (every first
    step of the bin search), edges[0] > 0 with pairs below it, integer edges with pairs AT them (r2 == e2[k] is bin k, the last edge
    excluded), T = 1, 3, 256, entries of +-2^30 quanta, the sum of counts = n_pairs."""
    ref = ph.pairpot_ref(case.fr, case.T, pot)
    base = np.tile(np.int64([-(1 << 50), 9]), (len(case.T), 1))
    full = h.pairpot(case.fr, case.T, pot, base=base)
    tally("k_pairpot", ph.check_pairpot(full, ref, case.fr, case.front[0], base=base))
    lean = h.pairpot(case.fr, case.T, pot, counts=False, base=base)
    ph.check_pairpot(lean, ref, case.fr, case.front[0], base=base, counts=False)
    assert lean["tot"].tobytes() == full["tot"].tobytes() and lean["lig_q"].tobytes() == full["lig_q"].tobytes()
    ph.check_pairpot(h.pairpot(case.fr, case.T, pot, per_atom=False, counts=False), ref, case.fr, case.front[0], per_atom=False, counts=False)


def test_iface_and_pairpot_chain_and_public_call(h, model):
    """The poses of the generic complex through the public creators and calls: rot / tr through the pose kernel give T; the harness on that
    T - the numpy frame, the restated parameters - gives bitwise what engine.Model.interface(...).energy and
    engine.Model.pairpot(...).energy return."""
    rec, lig, cen, rot, tr = ph.generic_atoms(0)
    _, c, par = ph.iface_cases()[0]
    T = h.pose("pose_iface", rot, tr, extra=0)["T"]
    assert T.tobytes() == h.pose("pose_pairpot", rot, tr, extra=0)["T"].tobytes()
    out = h.iface(c.fr, T, par)
    ph.check_iface(out, ph.iface_ref(c.fr, T, par), c.fr, ph.walk_front(c.fr, T)[0])
    handle = model.interface(rec, par.rec_par, lig, par.lig_par, cen, *par.args)
    try:
        api = handle.energy(rot, tr, per_atom=True)
    finally:
        handle.close()
    for k, col in (("rep_q", 0), ("att_q", 1), ("elec_q", 2), ("n_pairs", 3)):
        assert np.array_equal(np.asarray(api[k], np.int64), out["tot"][:, col]), k
    for k, mine in (("lig_vdw_q", "lig_vdw"), ("lig_elec_q", "lig_elec")):
        assert np.array_equal(api[k], np.where(out[mine] == ph.MARKER, 0, out[mine])), k
    _, c, pot = ph.pairpot_cases()[3]
    out = h.pairpot(c.fr, T, pot)
    ph.check_pairpot(out, ph.pairpot_ref(c.fr, T, pot), c.fr, ph.walk_front(c.fr, T)[0])
    handle = model.pairpot(rec, pot.rec_type, lig, pot.lig_type, cen, pot.edges, pot.table)
    try:
        api = handle.energy(rot, tr, per_atom=True, counts=True)
    finally:
        handle.close()
    assert np.array_equal(np.asarray(api["energy_q"], np.int64), out["tot"][:, 0]) and np.array_equal(np.asarray(api["n_pairs"], np.int64), out["tot"][:, 1])
    assert np.array_equal(api["lig_q"], np.where(out["lig_q"] == ph.MARKER, 0, out["lig_q"])) and np.array_equal(api["counts"], out["counts"])


# ---- hydrogen bonds and salt bridges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hb,T,rot,tr", ph.hbond_cases(), ids=[c[0] for c in ph.hbond_cases()])
def test_hbond_exact(h, name, hb, T, rot, tr):
    """launch_hbond + launch_hbond_finish bitwise against the restatement: every role combination on both sides, c2 = 0 and 0.97,
    antecedents coincident with their atoms (uu = 0), Rc = 0, Lc = 0, Rc = 33, side-chain kinds 0, 1, 2; the four per-atom outputs all
    given (the receptor's added to a base, the ligand's written on the walked blocks only) and all null; tot entries 0 .. 3 added to."""
    ref = ph.hbond_ref(hb, T)
    status = ph.walk_front(hb.fr, T)[0]
    base = np.tile(np.int32([3, -1, 100, 7, 0]), (len(T), 1))
    out = h.hbond(hb, T, base=base, rec_base=5)
    tally("k_hbond", ph.check_hbond(out, ref, hb, status, base=base, rec_base=5))
    ph.check_hbond(h.hbond(hb, T, per_atom=False), ref, hb, status, per_atom=False)


def test_hbond_public_call(h, model):
    """The generic polar complex through engine.Model.hbonds(...).count: bitwise the harness on the pose kernel's T."""
    name, hb, _, rot, tr = ph.hbond_cases()[0]      # c2 = 0 exactly: min_angle = 90 degrees
    T = h.pose("pose_hbond", rot, tr, extra=0)["T"]
    out = h.hbond(hb, T)
    ph.check_hbond(out, ph.hbond_ref(hb, T), hb, ph.walk_front(hb.fr, T)[0])
    handle = model.hbonds(hb.rec, hb.lig, hb.fr.center32, 3.5, 90.0, 4.0)
    try:
        api = handle.count(rot, tr, per_atom=True)
        info = handle.info()
    finally:
        handle.close()
    assert info["n_rec_charged"] == hb.Rc and info["n_lig_charged"] == hb.Lc
    assert np.array_equal(api["hb_kind"], out["tot"][:, :3]) and np.array_equal(api["n_salt_atoms"], out["tot"][:, 3])
    assert np.array_equal(api["n_salt"], out["tot"][:, 4]) and np.array_equal(api["n_hbond"], out["tot"][:, :3].sum(1))
    for k in ("rec_hb", "rec_sb"):
        assert np.array_equal(api[k], out[k]), k
    for k in ("lig_hb", "lig_sb"):
        assert np.array_equal(api[k], np.where(out[k] == ph.MARKER, 0, out[k])), k


# ---- buried surface --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sf,T,rot,tr", ph.surface_cases(), ids=[c[0] for c in ph.surface_cases()])
def test_surface_exact(h, name, sf, T, rot, tr):
    """launch_surface with its finish kernel, bitwise: the rec_bur masks themselves, lig_buried (the walked blocks only), rec_buried,
    class_points (added to a base): G = 1 .. 4, sixteen radius classes, Ar = 1, 255, 256, 257, a block whose queue drains several times,
    rec_bur set by three blocks of one pose; without per-atom outputs the same masks and class counts."""
    ref = ph.surface_ref(sf, T)
    status = ph.walk_front(sf.fr, T)[0]
    base = np.random.default_rng(3).integers(-9, 9, (len(T), 32)).astype(np.int32)
    out = h.surface(sf, T, base=base)
    tally("k_surface points", ph.check_surface(out, ref, sf, status, base=base))
    ph.check_surface(h.surface(sf, T, per_atom=False), ref, sf, status, per_atom=False)


def test_surface_public_call(h, model):
    """The generic complex through engine.Model.surface(...).bsa: bitwise the harness on the pose kernel's T with the restated exposure -
    which ties the numpy frame, the radius classes and exposure_ref to the shipped host preparation."""
    name, sf, _, rot, tr = ph.surface_cases()[0]
    rec, lig, cen, _, _ = ph.generic_atoms(0)
    T = h.pose("pose_surface", rot, tr, extra=0)["T"]
    out = h.surface(sf, T)
    ph.check_surface(out, ph.surface_ref(sf, T), sf, ph.walk_front(sf.fr, T)[0])
    handle = model.surface(rec, sf.rec_radius, lig, sf.lig_radius, cen, 1.4, 128)
    try:
        api = handle.bsa(rot, tr, per_atom=True)
        info = handle.info()
    finally:
        handle.close()
    K = sf.K
    assert np.array_equal(info["rec_exposed"], ph.unpack_bits(sf.rec_exp, K).sum(1)) and np.array_equal(info["lig_exposed"], ph.unpack_bits(sf.lig_exp, K).sum(1))
    assert np.array_equal(api["class_points"], out["class_points"]) and np.array_equal(api["rec_buried"], out["rec_buried"])
    assert np.array_equal(api["lig_buried"], np.where(out["lig_buried"] == ph.MARKER, 0, out["lig_buried"]))
    assert np.array_equal(api["rec_points"], out["class_points"][:, 0].sum(1)) and np.array_equal(api["lig_points"], out["class_points"][:, 1].sum(1))


# ---- every main kernel on non-finite poses, and the residue contacts through the public call ---------------------------------------------------
def test_non_finite_T_in_every_kernel(h):
    """Each of the 12 entries of a pose's T NaN, then +inf, with an ordinary pose before and after, through the five other main launches:
    walk_front is shared, so each must leave those poses at their prefill and give the ordinary ones their reference."""
    def T26(T):
        out = np.tile(T[0], (26, 1))
        for k in range(12):
            out[1 + k, k], out[13 + k, k] = np.nan, np.inf
        return out
    _, c, par = ph.iface_cases()[0]
    T = T26(c.T)
    status = ph.walk_front(c.fr, T)[0]
    assert (status[1:25] == 3).all() and (status[[0, 25]] == 0).any()
    out = h.iface(c.fr, T, par)
    ph.check_iface(out, ph.iface_ref(c.fr, T, par), c.fr, status)
    assert (out["tot"][1:25] == 0).all() and out["tot"][0, 3] > 0 and (out["tot"][0] == out["tot"][25]).all()
    _, c, pot = ph.pairpot_cases()[3]
    out = h.pairpot(c.fr, T, pot)
    ph.check_pairpot(out, ph.pairpot_ref(c.fr, T, pot), c.fr, status)
    assert (out["tot"][1:25] == 0).all() and (out["counts"][1:25] == 0).all() and out["tot"][0, 1] > 0
    _, hb, Th, _, _ = ph.hbond_cases()[0]
    T = T26(Th)
    out = h.hbond(hb, T)
    ph.check_hbond(out, ph.hbond_ref(hb, T), hb, ph.walk_front(hb.fr, T)[0])
    assert (out["tot"][1:25] == 0).all() and (out["bits"][1:25] == 0).all() and out["tot"][0, :4].sum() > 0
    _, sf, Ts, _, _ = ph.surface_cases()[0]
    T = T26(Ts)
    out = h.surface(sf, T)
    ph.check_surface(out, ph.surface_ref(sf, T), sf, ph.walk_front(sf.fr, T)[0])
    assert (out["rec_bur"][1:25] == 0).all() and (out["class_points"][1:25] == 0).all() and out["class_points"][0].sum() > 0
    c = ph.rescon_case()
    T = T26(c.T)
    bits = h.rescon(c.fr, T, c.Rr, c.Lr)
    np.testing.assert_array_equal(bits, ph.rescon_bits_ref(c.fr, T, c.rec_res, c.lig_res, c.Rr, c.Lr))
    assert (bits[1:25] == 0).all() and bits[0].any() and (bits[0] == bits[25]).all()


def test_rescon_chain_and_public_call(h, model):
    """rot / tr through the pose kernel, the bitmap and the finish kernel through the harness: bitwise what
    engine.Model.contacts(...).count returns - totals, both degree arrays and the bitmap itself."""
    c = ph.rescon_case()
    rec, lig, cen, rot, tr = ph.generic_atoms(0)
    rcl, lcl = np.random.default_rng(1).integers(0, 3, c.Rr).astype(np.uint8), np.random.default_rng(2).integers(0, 3, c.Lr).astype(np.uint8)
    T = h.pose("pose_rescon", rot, tr, extra=0)["T"]
    bits = h.rescon(c.fr, T, c.Rr, c.Lr)
    np.testing.assert_array_equal(bits, ph.rescon_bits_ref(c.fr, T, c.rec_res, c.lig_res, c.Rr, c.Lr))
    fin = h.rescon_finish(bits, c.Rr, rcl, lcl.astype(np.int32))
    handle = model.contacts(rec, c.rec_res, rcl, lig, c.lig_res, lcl, cen, ph.GENERIC["contact"])
    try:
        api = handle.count(rot, tr, per_residue=True, bits=True)
    finally:
        handle.close()
    assert np.array_equal(api["contact_bits"], bits)
    assert np.array_equal(api["ic"], fin["tot"][:, :6]) and np.array_equal(api["n_pairs"], fin["tot"][:, 6])
    assert np.array_equal(api["n_rec_res"], fin["tot"][:, 7]) and np.array_equal(api["n_lig_res"], fin["tot"][:, 8])
    assert np.array_equal(api["rec_degree"], fin["rec_degree"]) and np.array_equal(api["lig_degree"], fin["lig_degree"])


# ---- density fit: launch_density alone (the public call always zeroes tot through k_density_pose and builds T from fp32 rot / tr) -----------------
def density_exact(h, dc, T, base=None, atom_q=True, name="k_density"):
    """One launch_density against density_ref, integer for integer: sum_q, n_inside, n_above, atom_q, nothing written past n or [n][Al]."""
    P = len(T)
    base = ph.density_base(P) if base is None else base
    out = h.density(dc, T, atom_q=atom_q, base=base)
    ref = ph.density_ref(dc["grid4"], dc["geo"], dc["lig4"], T, dc["C"], base=base)
    cmp = ph.density_compare(out, ref, P, dc["Al"], base=base, atom_q=atom_q)
    print(name, "Al", dc["Al"], "n", P, cmp)
    assert not any(cmp.values()), (name, dc["dims"], dc["C"], dc["Al"], P, cmp)
    tally(name, P * dc["Al"])
    return out, ref


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", ph.DENSITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_density_exact(h, shape, C):
    """tot and atom_q against density_ref on T = the float64 restatement of pose_transform: grids 2 x 2 x 2 and [3, 5, 4] with anisotropic
    voxels and a negative origin, Al = 1, 63, 64, 65, 130, n = 1, 2, 5.  tot starts as a base of large values of both signs and comes back
    as base + sum on sum_q, n_inside, n_above; the slots of the channels at or above C keep the base although the grid's float4 holds
    non-zero values there; two more poses of tot and of atom_q behind the launch's keep base and marker; every entry of atom_q [n][Al] is
    overwritten (the reference has no marker); without atom_q the same totals."""
    for dc, rot, tr, T, base in ph.density_launches(shape, C):
        assert dc["grid4"][..., C:].all() or C == 4
        out, ref = density_exact(h, dc, T, base)
        bare, _ = density_exact(h, dc, T, base, atom_q=False)
        assert bare["tot"].tobytes() == out["tot"].tobytes()
        assert (out["tot"][:len(T), C:4] == base[:len(T), C:4]).all()


def test_density_exact_transforms(h):
    """T of exact doubles - the identity and the quarter turns about x, y, z, translations that are small binary fractions - with atoms
    planted on nodes, on each face, one fp32 ulp inside and outside each face, at u = -1/2 and at 1e30 / 3e38: the inside decision equals
    the one of exact rational arithmetic under every rotation; u = -0.0 is inside (the IEEE comparison is the definition)."""
    dc, T, labels = ph.planted_density_case()
    out, ref = density_exact(h, dc, T, name="k_density planted")
    exact = ph.density_inside_exact(dc, T)
    assert (out["tot"][:4, 4] - ph.density_base(4)[:4, 4] == exact.sum(1)).all()
    aq = out["atom_q"][:4 * dc["Al"]].reshape(4, dc["Al"])
    assert (aq[~exact] == 0).all() and (aq[exact] != 0).mean() > 0.9
    mz, Tz = ph.minus_zero_density_case()
    out, ref = density_exact(h, mz, Tz, base=np.zeros((3, 6), np.int64), name="k_density u = -0.0")
    assert out["tot"][0, 4] == 1 and ref["inside"].all()


def test_density_ties_to_even(h):
    """(w val) 2^20 exactly on k + 1/2: to even, for both signs; and ties that exist only because w val is rounded before the scale and
    because the lerps run along x first."""
    half, rounded, T = ph.ties_density_case()
    out, _ = density_exact(h, half, T, name="k_density ties")
    assert out["atom_q"][:5].tolist() == [0, 2, 2, 0, -2]
    out, _ = density_exact(h, rounded, T, name="k_density ties")
    assert out["atom_q"][:8].tolist() == [2, 4, 4, 6, 6, 8, 8, 10]


def test_density_non_finite_T(h):
    """NaN, +inf and -inf in each of the 12 slots of T, 36 poses between two ordinary ones: each adds nothing to tot and gets zeros in atom_q;
    the two ordinary poses are bitwise what they are in a launch of their own."""
    dc, rot, tr, T, _ = ph.density_launches((3, 5, 4), 2)[11]      # Al = 65, n = 5
    T38 = ph.nonfinite_density_T(T[0], T[1])
    base = ph.density_base(38, seed=3)
    out, ref = density_exact(h, dc, T38, base, name="k_density non-finite T")
    assert (out["tot"][1:37] == base[1:37]).all() and (out["atom_q"][65:37 * 65] == 0).all()
    assert ref["inside"][0].any() and ref["inside"][37].any()
    alone = h.density(dc, T[:2], base=base[[0, 37, 36, 36]])
    assert (alone["tot"][:2] == out["tot"][[0, 37]]).all()
    assert (alone["atom_q"][:130] == np.concatenate([out["atom_q"][:65], out["atom_q"][37 * 65:38 * 65]])).all()


def test_density_every_atom_outside(h):
    """No atom of any block inside (the wave's early return): tot keeps its base, atom_q is zeros."""
    dc0, rot, tr, T, base = ph.density_launches((3, 5, 4), 3)[14]      # Al = 130, n = 5
    far = dc0["lig4"][:, :3] + ph.f32([500.0, 0.0, 0.0])
    dc = ph.density_case((3, 5, 4), 3, 130, lig=far, w=dc0["lig4"][:, 3], center=dc0["center"])
    out, ref = density_exact(h, dc, T, base, name="k_density all outside")
    assert not ref["inside"].any() and (out["tot"] == base).all() and (out["atom_q"][:5 * 130] == 0).all()


def test_density_largest_n(h):
    """n = 65535 (gridDim.y's limit) with Al = 1 on 2 x 2 x 2: accepted and exact."""
    dc, T = ph.limit_density_case()
    out, ref = density_exact(h, dc, T, name="k_density n 65535")
    assert 0.2 < ref["inside"].mean() < 0.8


@pytest.mark.parametrize("change", [dict(n=65536), dict(n=0), dict(nx=1), dict(ny=1), dict(nz=1), dict(Al=0)], ids=lambda c: "%s=%d" % next(iter(c.items())))
def test_density_refusals_leave_every_block_alone(h, change):
    """The launcher's own refusals (the shim lets these through): hipErrorInvalidValue, tot still the base, atom_q still the marker."""
    dc = ph.density_case((2, 2, 2), 2, 3)
    P = max(change.get("n", 2), 1)
    T = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (P, 1))
    over = dict(change)
    for k, slot in (("nx", 10), ("ny", 11), ("nz", 12)):
        if k in change:
            over["geo"] = dc["geo"].copy()
            over["geo"][slot] = change[k] - 1.0
    base = ph.density_base(P, seed=4)
    out = h.density(dc, T, base=base, check=False, **over)
    assert out["err"] == ph.HIP_INVALID_VALUE
    assert (out["tot"] == base).all() and (out["atom_q"] == ph.MARKER).all()
    assert ph.guards_intact(out, "tot") and ph.guards_intact(out, "atom_q")


def test_density_limits_of_the_sums(h):
    """Grid values of 2^10 and weights of +-2^7: every term is +-2^37 exactly, 130 of them per pose."""
    dc, T = ph.sum_limit_density_case()
    out, ref = density_exact(h, dc, T, base=np.zeros((4, 6), np.int64), name="k_density limits")
    assert set(np.abs(out["atom_q"][:260]).tolist()) == {1 << 37} and (out["tot"][:2, 0] == (117 - 13) * (1 << 37)).all()
    assert (out["tot"][:2, 1] == -out["tot"][:2, 0]).all() and (out["tot"][:2, 4:] == 130).all()
