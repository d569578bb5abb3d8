"""The rigid pose fit on the GPU (dfm_pose_fit, kernels_fit.hip: k_fit_reduce, k_fit_solve, k_fit_resid) against its float64 definition
dfmdock_amd/fit.py, through the public call engine.Model.pose_fit and, launch by launch inside guard bands, through
tests/kernels/fit_harness.hip.  Gates and inputs: tests/fit_harness.py.

Shapes: L = 1, 2, 63, 64, 65, 130 (the lane stride and its edges) x P = 1, 4, 5 (four poses per workgroup and its edge) without a
receptor and with R = 1, 64, 65.  The round trip apply -> fit -> rebuild is asserted at every one of them.  Its bound of 1e-4 A is the
sum of four fp32 roundings for coordinates within 256 A and lever arms within 64 A: 1.5e-5 A for the half-ulp of a coordinate, counted
twice, 2^-24 pi 64 A = 1.2e-5 A for rot, 1.5e-5 A for tr.  Those are the premises without a receptor and with a receptor that stands
where the input's does (the decoy in the input's frame: R = 1, 64, 65 alike), and 1e-4 A is asserted there.  A decoy carried into a
frame of its own went through one more rounding, and its rounded receptor fixes that frame only so well: 1e-4 A is asserted all the same
at R = 64 and 65, and at R = 1 - three atoms within 1.5 A of each other under lever arms of tens of A - the bound derived in
fit_harness.frame_bound from the case's own geometry.
"""
import math

import numpy as np
import pytest

import fit_harness as fh

pytestmark = pytest.mark.gpu

LS, PS, RS = (1, 2, 63, 64, 65, 130), (1, 4, 5), (0, 1, 64, 65)
ROUND_TRIP = fh.ROUND_TRIP


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    return fh.Harness(fh.compile_shim(tmp_path_factory.mktemp("fit_harness_gpu")))


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def call(model, cs, **kw):
    return model.pose_fit(cs["lig_ref"], cs["lig_pos"], cs["center"], cs["rec_ref"], cs["rec_pos"], **kw)


def bits(out, p):
    return tuple(None if out[k] is None else out[k][p].tobytes() for k in ("rot", "tr", "rmsd", "rec_rmsd"))


@pytest.mark.parametrize("L", LS)
def test_public_call_against_the_definition(model, h, L):
    """Every (P, R) of the grid at this L: rot, tr within 2 ulp of the definition rounded to fp32, the RMSDs at the tight gate, the fp64
    rotations behind them (the shim's xf) proper and optimal, and the round trip apply -> fit -> rebuild within 1e-4 A."""
    from dfmdock_amd.cluster import rebuild_backbone
    worst = {}
    for P in PS:
        for R in RS:
            family = (P + R) % 2
            cs = fh.case(1000 * L + 10 * P + R, P, L, R, family)
            rot, tr, rmsd, rec_rmsd = fh.definition(cs)
            got = call(model, cs)
            stats = {"rot ulp": fh.check_ulps(got["rot"], rot), "tr ulp": fh.check_ulps(got["tr"], tr), "rmsd": fh.check_rmsd(got["rmsd"], rmsd)}
            if R:
                stats["rec_rmsd"] = fh.check_rmsd(got["rec_rmsd"], rec_rmsd)
            else:
                assert got["rec_rmsd"] is None
            assert (got["rmsd"] < ROUND_TRIP).all(), "a rigid image of the input fits to fp32 rounding"
            full = h.full(cs)
            stats.update(fh.check_xf(full["xf"], cs))
            for k in ("rot", "tr"):      # the launchers and the call are the same kernels on the same data
                assert full[k].tobytes() == got[k].tobytes(), k
            assert full["rmsd"].tobytes() == got["rmsd"].tobytes()
            back = rebuild_backbone(cs["lig_ref"], got["rot"], got["tr"], family).astype(np.float64)
            start = fh.apply(cs["lig_ref"], cs["rot"], cs["tr"], cs["center"])
            if not R:      # round trip: apply, fit, rebuild
                stats["round trip"] = float(np.abs(back - start.astype(np.float64)).max())
                assert stats["round trip"] <= fh.ROUND_TRIP, (P, R, stats)
            else:
                # through a receptor that stands where the input's does: the decoy in the input's frame, the four roundings and no more
                same = dict(cs, lig_pos=start, rec_pos=np.repeat(cs["rec_ref"][None], P, 0))
                g0 = call(model, same)
                back0 = rebuild_backbone(cs["lig_ref"], g0["rot"], g0["tr"], family).astype(np.float64)
                stats[f"round trip, receptor of {R} in place"] = float(np.abs(back0 - start.astype(np.float64)).max())
                assert stats[f"round trip, receptor of {R} in place"] <= fh.ROUND_TRIP and (g0["rec_rmsd"] == 0.0).all(), (P, R, stats)
                # through a frame of the decoy's own
                dev = np.abs(back - start.astype(np.float64)).reshape(P, -1).max(1)
                bound = np.array([fh.ROUND_TRIP if R >= 64 else fh.frame_bound(cs, p) for p in range(P)])
                stats[f"round trip, receptor of {R} moved"] = float(dev.max())
                stats[f"round trip, receptor of {R} moved / bound"] = float((dev / bound).max())
                assert (dev <= bound).all(), (P, R, dev, bound)
            for k, v in stats.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"L={L}", {k: f"{v:.3g}" for k, v in worst.items()})


def test_special_poses(model, h):
    from dfmdock_amd.pdbio import axis_angle_to_matrix
    rng = np.random.default_rng(7)
    # the identity, without and with a receptor that did not move: rot exactly 0
    for R in (0, 64):
        cs = fh.case(70 + R, 1, 65, R)
        cs["lig_pos"] = cs["lig_ref"][None].copy()
        if R:
            cs["rec_pos"] = cs["rec_ref"][None].copy()
        got = call(model, cs)
        assert not got["rot"].any() and got["rmsd"][0] < 1e-5 and np.abs(got["tr"]).max() == 0.0, got
    # a rotation by exactly pi (w = 0) on lattice coordinates: x -> (-x, -y, z) about the centre is exact in fp32
    lig = (np.round(fh.chain(rng, 65, np.zeros(3)) * 4) / 4).astype(np.float32)
    c = np.array([2.0, -3.0, 1.0], np.float32)
    half = ((lig - c) * np.array([-1, -1, 1], np.float32) + c).astype(np.float32)
    cs = dict(P=1, L=65, R=0, lig_ref=lig, lig_pos=half[None], center=c, rec_ref=None, rec_pos=None)
    got = call(model, cs)
    np.testing.assert_allclose(axis_angle_to_matrix(got["rot"][0]), np.diag([-1.0, -1.0, 1.0]), atol=1e-6)
    assert abs(np.linalg.norm(got["rot"][0].astype(np.float64)) - np.pi) < 1e-6 and got["rmsd"][0] < 1e-5 and np.abs(got["tr"]).max() < 1e-5
    fh.check_xf(h.full(cs)["xf"], cs)
    # a mirrored ligand: a proper rotation all the same, and no rigid image
    mirrored = ((lig - c) * np.array([-1, 1, 1], np.float32) + c).astype(np.float32)
    cs = dict(cs, lig_pos=mirrored[None])
    got = call(model, cs)
    fh.check_xf(h.full(cs)["xf"], cs)
    assert got["rmsd"][0] > 1.0
    fh.check_rmsd(got["rmsd"], fh.definition(cs)[2])
    # collinear atoms: the rotation about the line is free, so only the rmsd and the validity of R
    line = (np.arange(3 * 9, dtype=np.float64)[:, None] * np.array([1.5, -0.75, 0.5]) + np.array([10.0, 20.0, -5.0])).reshape(9, 3, 3).astype(np.float32)
    c = fh.center_of(line, 0)
    rot, tr = fh.random_poses(rng, 4)
    cs = dict(P=4, L=9, R=0, lig_ref=line, lig_pos=fh.apply(line, rot, tr, c), center=c, rec_ref=None, rec_pos=None)
    got = call(model, cs)
    assert (got["rmsd"] < ROUND_TRIP).all()
    xf = h.full(cs)["xf"]
    for p in range(4):
        d_o, d_d = fh.rotation_defects(xf[p, :9])
        assert d_o <= fh.ORTHO_TOL and d_d <= fh.DET_TOL


def test_rejection_and_nan(model):
    """A non-rigid decoy - one residue displaced by 2 A - has an rmsd above the drivers' tolerance of 0.1 A; a pose with a NaN is NaN in
    its four outputs and leaves the other four of its batch bitwise what they are alone."""
    cs = fh.case(11, 5, 65, 64)
    bent = dict(cs, lig_pos=cs["lig_pos"].copy())
    bent["lig_pos"][1, 17] += np.float32(2.0) * np.array([0.6, 0.0, 0.8], np.float32)
    got = call(model, bent)
    assert got["rmsd"][1] > 0.1 and (np.delete(got["rmsd"], 1) < ROUND_TRIP).all() and (got["rec_rmsd"] < ROUND_TRIP).all()
    fh.check_rmsd(got["rmsd"], fh.definition(bent)[2])
    clean = call(model, cs)
    for where in ("lig_pos", "rec_pos"):
        bad = dict(cs, **{where: cs[where].copy()})
        bad[where][2, 40, 1, 2] = np.nan
        got = call(model, bad)
        for k in ("rot", "tr", "rmsd", "rec_rmsd"):
            assert np.isnan(got[k][2]).all(), (where, k)
        for p in (0, 1, 3, 4):
            assert bits(got, p) == bits(clean, p), (where, p)
            alone = {k: (v[p:p + 1] if k in ("lig_pos", "rec_pos") else v) for k, v in cs.items()}
            assert bits(call(model, dict(alone, P=1)), 0) == bits(clean, p), p
        d = fh.definition(bad)
        assert all(np.isnan(x[2]).all() for x in d)


@pytest.mark.parametrize("R", (0, 65))
def test_batch_invariance(model, R):
    """Pose b's bits are the same at P = 1, 5 and 130, at any place in the batch and across a forced chunk boundary."""
    big = fh.case(5, 130, 65, R)
    ref = call(model, big)
    for chunk in (1, 3, 64, 129):
        got = call(model, big, chunk_poses=chunk)
        for k in ("rot", "tr", "rmsd", "rec_rmsd"):
            assert (got[k] is None and ref[k] is None) or got[k].tobytes() == ref[k].tobytes(), (chunk, k)
    order = np.random.default_rng(3).permutation(130)
    for sel in (order[:1], order[:5], order, np.array([129, 0, 64, 63, 65])):
        sub = dict(big, P=len(sel), lig_pos=big["lig_pos"][sel], rec_pos=None if not R else big["rec_pos"][sel])
        got = call(model, sub, chunk_poses=2 if len(sel) == 5 else 0)
        for i, p in enumerate(sel):
            assert bits(got, i) == bits(ref, p), (len(sel), i, p)


def test_per_launch_inside_guard_bands(h):
    """reduce, solve and resid each on their own at L = 65, P = 5 (kernel_harness.collect refuses a byte outside a block): the three
    launches chained through the host give the bits of the one-go run, and the sums are the float64 sums to rounding."""
    for R in (0, 65):
        cs = fh.case(21 + R, 5, 65, R)
        full = h.full(cs)
        red = h.reduce(cs)
        assert red["sums"].tobytes() == full["sums"].tobytes()
        sol = h.solve(cs, red["sums"])
        for k in ("xf", "rot", "tr"):
            assert sol[k].tobytes() == full[k].tobytes(), k
        res = h.resid(cs, sol["xf"])
        assert res["rmsd"].tobytes() == full["rmsd"].tobytes()
        if R:
            assert res["rec_rmsd"].tobytes() == full["rec_rmsd"].tobytes()
        for k in ("sums", "xf", "rot", "tr", "rmsd") + (("rec_rmsd",) if R else ()):
            assert fh.guards_intact(full, k), k
        # the sums against float64: S_pos | C = sum pos ref^T | S_ref in coordinates shifted by the centre
        o = cs["center"].astype(np.float64)
        chains = [(cs["lig_pos"], cs["lig_ref"])] + ([(cs["rec_pos"], cs["rec_ref"])] if R else [])
        for ci, (pos, ref) in enumerate(chains):
            q = ref.astype(np.float64).reshape(-1, 3) - o
            for p in range(5):
                x = pos[p].astype(np.float64).reshape(-1, 3) - o
                terms = np.concatenate([x, (x[:, :, None] * q[:, None, :]).reshape(len(x), 9), q], 1)      # [atoms, 15]
                want = np.array([math.fsum(terms[:, k]) for k in range(15)])      # the exactly rounded sum of the float64 terms
                scale = np.abs(terms).sum(0)
                assert (np.abs(full["sums"][p, ci] - want) <= (len(x) + 8) * 2.0 ** -53 * scale).all(), (R, ci, p)
        fh.check_xf(full["xf"], cs)
