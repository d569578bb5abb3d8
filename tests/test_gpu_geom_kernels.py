"""The graph front end and the pose kernels launch by launch (kernels_geom.hip: k_knn_sample<NPL>, k_edge_feat<0 / 1>, k_l0_pairs,
k_clash_force, k_init_pose), driven through tests/kernels/geom_harness.hip on small host arrays with guard bands around every device
block, against the references of tests/geom_harness.py (written from the model definition; tests/test_geom_harness_cpu.py shows
that the comparisons used here reject seeded mutants of those references).

What is exact and what carries a margin (kernels_geom.hip is compiled with -ffp-contract=off: sum, product, sqrtf and division are
correctly rounded fp32 in the order written, which numpy float32 reproduces bit for bit):
  exact (array_equal)   kNN slots and their order, the distance bin, relpos, radial, every index, row list and counter.
  angle bins            float64 angles from the same fp32 inputs.  An edge is DECIDED when its float64 angle is further than m from every
                        boundary (the 23 angle bounds, 18 q, +-180), m = four times the largest |numpy fp32 restatement - float64| over
                        the case's own gated edges (tests/test_geom_harness_cpu.py prints it: below 0.02 degrees on these inputs, which
                        leaves under 1 % of the edges of any case undecided).  A decided edge has the float64 bin, an undecided one a
                        bin within m.  NaN angles (coincident residues, collinear backbone) bin to 0.
  race keys             float64 -log2(u) d^3 with u from the numpy Philox; the kernel's key differs by the hardware log2 and one fp32
                        product: bound = 2 ((rel |log2 u| + abs) d^3 + 2 u key) with (rel, abs) = geom_harness.LOG2_ENVELOPE, the envelope
                        test_hw_log2_envelope measures on all 2^24 values of u01 (profiles/geom_kernels.txt: 2^-23.01 relative), doubled.
                        A node is decided when its nsamp-th and (nsamp + 1)-th keys are further apart than the sum of their bounds.
  k_clash_force         float64 closed form; the shift is one rounding of a float64 mean and each stored value one fp32 addition:
                        4 u scale (scale = mean of |terms| >= |shift|) + 2 u |value|.
  k_init_pose           injected: the bound of the k_heads update (tests/test_gpu_head_kernels.py) with dR = 0: pose 2 rad 32 u + dtr + 8 u
                        (|x| + |c| + |tr|), dtr = 4 u (|draw| + |c1| + |c2|), rot_update 256 u (angles below 2.5).  Native: each Box-Muller
                        normal z = r cos(2 pi u_b), r = sqrt(-2 ln u_a), carries dz = r (4 pi + 4) u + 3 u |z| + 2 u r (logf 1 ulp, sqrtf,
                        two roundings of the argument, cosf 2 ulp, the product); dR = 4 max dz / |q| + 2 u enters the same formulas;
                        trajectories whose first uniform is below 2^-20 are excluded.
  non-finite poses      five geometries with a NaN or infinite coordinate in one trajectory of three (geom_harness.NONFINITE).  No new
                        margin: the graph follows the ordering rule of include/dfmdock_amd.h (a NaN distance after every number, ties by
                        ascending j, numbers first in the race: geom_harness.order_word / check_sampled), every edge is a residue index,
                        codes / radial / row list / counter are the IEEE restatement (radial NaN by isnan, +inf by its bits), a pair
                        with a non-finite r2 is no table hit, and the finite trajectories have the bits of the launch on the finite
                        twin.  tests/test_geom_harness_cpu.py shows that the selection as it stood before the rule is rejected on
                        these geometries and accepted on the finite ones.
The largest |error| / bound of every toleranced test and the measured log2 envelope go to $DFM_GEOM_PROFILE/geom_kernels_gpu.txt when that
variable names a directory (profiles/geom_kernels.txt holds the MI355X figures).
"""
import os

import numpy as np
import pytest

import geom_harness as gh
from geom_harness import Out

pytestmark = pytest.mark.gpu

U = gh.U
RATIOS = {}
NOTES = {}
SEED = 0x1234567899ABCDEF
STREAM = 3


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    harness = gh.Harness(gh.compile_shim(tmp_path_factory.mktemp("geom_harness_gpu")))
    yield harness
    out = os.environ.get("DFM_GEOM_PROFILE")
    if out:
        with open(os.path.join(out, "geom_kernels_gpu.txt"), "w") as f:
            f.write("test max_error_over_bound\n" + "".join(f"{k} {v:.4g}\n" for k, v in sorted(RATIOS.items())))
            f.write("".join(f"{k} {v}\n" for k, v in sorted(NOTES.items())))


def run(h, op, bufs, **scalars):
    r = h.run(op, bufs, **scalars)
    assert r["err"] == gh.HIP_SUCCESS, f"{op}: hipError {r['err']}"
    for k, v in bufs.items():
        if isinstance(v, Out):
            assert gh.guards_intact(r, k), f"{op}: bytes outside the {k} block changed"
    return r


def check(name, got, ref, bound, key=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ratio = np.abs(got - ref) / np.broadcast_to(bound, ref.shape)
    worst = float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if ratio.size else 0.0
    k = key or name
    RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
    print(f"{name}: max |err| / bound = {worst:.3g}")
    assert worst <= 1.0, f"{name}: worst |err| / bound = {worst:.3g} at {np.argwhere(~(ratio <= 1.0))[:3].tolist()}"


# ---- 1b (first): the hardware log2 itself ----------------------------------------------------------------------------------------
def test_hw_log2_envelope(h):
    """v_log_f32 on all 2^24 values u01 can return against float64 log2: the largest relative error where |log2 u| >= 1, and the largest
    absolute excess over it near u -> 1.  The committed envelope (geom_harness.LOG2_ENVELOPE) must contain every value; log2(1) = 0."""
    n = 1 << 24
    u = gh.u01_np(np.arange(n, dtype=np.uint32) << np.uint32(8))
    r = run(h, "hw_log2", dict(log_in=u, log_out=Out(np.float32, n)), n=n)
    ref = np.log2(u.astype(np.float64))
    err = np.abs(r["log_out"].astype(np.float64) - ref)
    mag = np.abs(ref)
    rel = float((err[mag >= 1.0] / mag[mag >= 1.0]).max())
    rel_all = float((err[mag > 0] / mag[mag > 0]).max())
    absx = float(np.maximum(err - rel * mag, 0.0).max())
    NOTES["hw_log2 rel(|log2 u| >= 1)"] = f"{rel:.4g} = 2^{np.log2(rel):.2f}"
    NOTES["hw_log2 rel(all u < 1)"] = f"{rel_all:.4g} = 2^{np.log2(rel_all):.2f}"
    NOTES["hw_log2 abs excess near 1"] = f"{absx:.4g}" + (f" = 2^{np.log2(absx):.2f}" if absx > 0 else "")
    NOTES["hw_log2(1.0)"] = repr(float(r["log_out"][u == 1.0][0]))
    print(NOTES)
    assert (u == 1.0).any() and (r["log_out"][u == 1.0] == 0.0).all()
    ratio = err / (gh.LOG2_ENVELOPE[0] * mag + gh.LOG2_ENVELOPE[1])
    RATIOS["hw_log2 / committed envelope"] = float(ratio.max())
    assert ratio.max() <= 1.0, f"the hardware log2 leaves the committed envelope: {ratio.max():.3g} x"


# ---- 1 / 1b: k_knn_sample ----------------------------------------------------------------------------------------------------------
def knn_launch(h, ca4, knn, nsamp, seed=SEED, stream=STREAM, ctl=None):
    B, N = ca4.shape[:2]
    K = knn + nsamp
    r = run(h, "knn_sample", dict(ca4=ca4, edges=Out(np.int32, B * N * K), ctl=ctl), B=B, N=N, knn=knn, nsamp=nsamp, seed=seed, stream_id=stream)
    return r["edges"].reshape(B, N, K)


def check_graph(edges, ca4, knn, nsamp, seed=SEED, stream=STREAM):
    """geom_harness.check_graph (the comparison the CPU tests turn on the mutants) with the measured envelope."""
    return gh.check_graph(edges, ca4, knn, nsamp, seed, stream, gh.LOG2_ENVELOPE)


@pytest.mark.parametrize("case", gh.knn_cases(), ids=gh.knn_case_id)
def test_knn_sample(h, case):
    """Every instantiation (N on both sides of 256 / 512 / 768 / 1024 / 2048, and N = 4093 / 4096: the largest complex, where NPL = 64
    has candidates in all 64 bits of a lane's selection mask), the degree clamps (N = 1 .. 61), three kinds
    of geometry (random chain; integer lattice: ties at the knn-th distance on most nodes; coincident residues) and the degrees up to
    knn = 60: slots [0, knn) are the knn smallest (d, j) in ascending order, slots [knn, K) the nsamp smallest race keys."""
    kind, N, B, knn, nsamp = case
    knn, nsamp = gh.degree_of(N, knn, nsamp)
    ca4 = gh.COORDS[kind](B, N, seed=N)
    edges = knn_launch(h, ca4, knn, nsamp)
    check_graph(edges, ca4, knn, nsamp)
    if kind == "chain":
        assert (edges[:, :, 0] == np.arange(N)[None, :]).all(), "slot 0 is the node itself"


def test_knn_sample_refuses_more_candidates_than_it_holds(h):
    """k_knn_sample<64> holds 4 x 64 x 16 = 4096 candidates per node (MAX_NODES).  A longer chain used to be scanned up to j = 4095
    only - at N = 4133 the last node's own slot 0 came back as residue 1179, its nearest neighbour below 4096 - so the launcher
    refuses it with hipErrorInvalidValue and writes nothing."""
    N = gh.KNN_N_REFUSED
    ca4 = gh.chain_coords(1, N, seed=N)
    r = h.run("knn_sample", dict(ca4=ca4, edges=Out(np.int32, N * 60)), B=1, N=N, knn=20, nsamp=40, seed=SEED, stream_id=STREAM)
    assert r["err"] == gh.HIP_INVALID_VALUE
    assert gh.is_sentinel(r["edges"]).all() and gh.guards_intact(r, "edges")


def test_knn_sample_ctl_streams_and_batch(h):
    """The replayed-graph path (seed and evaluation index from three device words) gives the same edges, bit for bit, as the same
    values passed as arguments; two evaluation indices give different graphs with the same kNN slots; each checked against the
    reference.  The counter's node word is b N + i: trajectories holding the SAME pose get the same kNN slots and different
    sampled slots, and trajectory b matches the reference stream of node b N + i (check_graph), not that of node i."""
    N, B, knn, nsamp = 130, 3, 20, 40
    ca4 = np.repeat(gh.chain_coords(1, N, seed=11), B, 0)
    a = knn_launch(h, ca4, knn, nsamp, seed=SEED, stream=5)
    check_graph(a, ca4, knn, nsamp, SEED, 5)
    ctl = np.array([5, SEED & 0xFFFFFFFF, SEED >> 32], np.uint32)
    c = knn_launch(h, ca4, knn, nsamp, seed=99, stream=77, ctl=ctl)
    np.testing.assert_array_equal(a, c)
    b2 = knn_launch(h, ca4, knn, nsamp, seed=SEED, stream=6)
    check_graph(b2, ca4, knn, nsamp, SEED, 6)
    np.testing.assert_array_equal(a[..., :knn], b2[..., :knn])
    assert (np.sort(a[..., knn:], -1) != np.sort(b2[..., knn:], -1)).any(-1).mean() > 0.9
    np.testing.assert_array_equal(a[0, :, :knn], a[1, :, :knn])
    assert (np.sort(a[0, :, knn:], -1) != np.sort(a[1, :, knn:], -1)).any(-1).mean() > 0.9
    one = knn_launch(h, ca4[:1], knn, nsamp, seed=SEED, stream=5)
    np.testing.assert_array_equal(one[0], a[0])      # trajectory 0 IS the B = 1 launch: node word i


def test_knn_sample_uniform_of_one(h):
    """A candidate whose uniform is exactly 1.0f (u01's largest value: geom_harness.TOP_UNIFORM_EDGE, found by a host search) has the race
    key -log2(1) d^3 = 0: it wins its race with certainty.  N = 61 with K = 60: all but one of the candidates are drawn."""
    N, B, knn, nsamp = 61, 3, 20, 40
    stream, node, blk, word = gh.TOP_UNIFORM_EDGE
    ca4 = gh.top_uniform_coords()
    edges = knn_launch(h, ca4, knn, nsamp, seed=gh.TOP_UNIFORM_SEED, stream=stream)
    b, i, j = node // N, node % N, 4 * blk + word
    u = gh.edge_stream_u([node], N, stream, gh.TOP_UNIFORM_SEED)
    assert u[0, j] == np.float32(1.0) and j not in edges[b, i, :knn]
    check_graph(edges, ca4, knn, nsamp, gh.TOP_UNIFORM_SEED, stream)
    assert j in edges[b, i, knn:]


# ---- 2: k_edge_feat<0> -------------------------------------------------------------------------------------------------------------
def feat_launch(h, c, cls=None, eval_ctr=None):
    total = c["B"] * c["N"] * c["K"]
    bufs = dict(n4=c["n4"], ca4=c["ca4"], cb4=c["cb4"], edges=c["edges"], codes=Out(np.uint32, total), radial=Out(np.float32, total))
    if eval_ctr is not None:
        bufs["eval_ctr"] = Out(np.uint32, init=np.array([eval_ctr], np.uint32))
    if cls is not None:
        bufs.update(code0=cls["code0"], src=Out(np.uint32, total), rows=Out(np.uint32, 4 * cls["capacity"]),
                    counter=Out(np.uint32, init=np.array([cls["start"]], np.uint32)))
    return run(h, "edge_feat", bufs, B=c["B"], N=c["N"], R=c["R"], K=c["K"], mask_dist=c["mask_dist"])


@pytest.mark.parametrize("case", gh.EDGE_CASES, ids=lambda c: f"{c[0]}-N{c[1]}-R{c[2]}-K{c[3]}")
def test_edge_feat(h, case):
    """Random index lists (i = j, inter-chain pairs, pairs beyond mask_dist, relpos offsets beyond +-32 in both chain orders) and a pose
    with distances ON bin boundaries, coincident residues and a collinear backbone; total = 255, 256, 257 and larger.  With eval_ctr,
    exactly one increment."""
    c = gh.edge_case(*case)
    r = feat_launch(h, c, eval_ctr=41)
    ref = gh.edge_case_ref(c)
    m = gh.angle_margin(ref)
    und = gh.check_edge_codes(r["codes"], r["radial"], ref, m)
    f = gh.unpack_code(r["codes"])
    masked = ~ref["gate"]
    assert masked.any() and not (f["om"][masked] | f["th"][masked] | f["ph"][masked]).any()
    assert und <= 0.01 * ref["gate"].size, (und, ref["gate"].size)
    assert int(r["eval_ctr"][0]) == 42
    if case[0] == "boundary":
        assert (np.sqrt(ref["r2"])[:, None] == gh.DIST_BOUNDS[None, :]).any(1).sum() >= 5
        nan = np.isnan(ref["a64"]) & ref["gate"][:, None]
        assert nan[:, 1].any() and (case[1] <= 12 or nan[:, 0].any())


def test_edge_feat_on_the_kernels_own_edges(h):
    """The kNN + sampled lists of k_knn_sample as the edges (slot 0 = the node itself: i = j)."""
    N, R, B = 150, 90, 2
    n4, ca4, cb4 = gh.backbone(gh.chain_coords(B, N, seed=21), seed=3)
    edges = knn_launch(h, ca4, 20, 40)
    c = dict(n4=n4, ca4=ca4, cb4=cb4, edges=edges, B=B, N=N, R=R, K=60, mask_dist=22.0)
    r = feat_launch(h, c)
    ref = gh.edge_case_ref(c)
    und = gh.check_edge_codes(r["codes"], r["radial"], ref, gh.angle_margin(ref))
    assert und <= 0.01 * ref["gate"].size


# ---- 3: k_l0_pairs and k_edge_feat<1> ------------------------------------------------------------------------------------------------
def pairs_launch(h, c):
    P = c["R"] * c["R"] + c["L"] * c["L"]
    return run(h, "l0_pairs", dict(n4=c["n4"], ca4=c["ca4"], cb4=c["cb4"], code0=Out(np.uint32, 2 * P), rows=Out(np.uint32, 4 * P)),
               R=c["R"], L=c["L"], mask_dist=c["mask_dist"])


@pytest.mark.parametrize("R,L", gh.PAIR_SIZES)
def test_l0_pairs(h, R, L):
    """rows[q] and code0[q] at q = pair index hold (i, j, code, r2 bits) of every intra-chain ordered pair (receptor block, then ligand
    block), nothing else is written (guard bands; the blocks have exactly R R + L L entries), the codes are the reference's and equal
    k_edge_feat<0> on the same pairs."""
    N = R + L
    n4, ca4, cb4 = gh.backbone(gh.chain_coords(1, N, seed=31), seed=4)
    c = dict(n4=n4, ca4=ca4, cb4=cb4, R=R, L=L, N=N, mask_dist=22.0)
    p = pairs_launch(h, c)
    ii, jj = gh.all_pairs(R, L)
    # the same pairs through k_edge_feat<0>: one "node" per pair is not expressible, so all N x N pairs, then the intra-chain ones
    full = dict(c, B=1, K=N, edges=np.tile(np.arange(N, dtype=np.int32), (1, N, 1)))
    r = feat_launch(h, full)
    sel = ii * N + jj
    ref = gh.edge_ref(n4[0], ca4[0], cb4[0], ii, jj, R, 22.0)
    gh.check_edge_codes(r["codes"][sel], r["radial"][sel], ref, gh.angle_margin(ref))
    gh.check_pairs(p["code0"], p["rows"], R, L, r["codes"][sel], r["radial"][sel])
    assert not gh.is_sentinel(p["rows"]).any() and not gh.is_sentinel(p["code0"]).any()


def classify(h, c, start=0, planted=True, skip_below=0):
    p = pairs_launch(h, c)
    code0 = p["code0"].reshape(-1, 2)
    if planted:
        code0 = gh.plant(code0, code0[:, 1].copy().view(np.float32), np.random.default_rng(0), skip_below)
    total = c["N"] * c["K"]
    r = feat_launch(h, c, cls=dict(code0=code0, capacity=total + start, start=start))
    r0 = feat_launch(h, c)
    np.testing.assert_array_equal(r["codes"], r0["codes"])
    np.testing.assert_array_equal(r["radial"].view(np.uint32), r0["radial"].view(np.uint32))
    ref = gh.edge_case_ref(c)
    gh.check_edge_codes(r["codes"], r["radial"], ref, gh.angle_margin(ref))
    _, i, j = gh.edge_ij(c["edges"], c["N"], c["K"])
    hit, idx = gh.hit_ref(i, j, r["codes"], r["radial"], code0, c["R"], c["L"])
    rows = r["rows"].reshape(-1, 4)
    if start:
        assert gh.is_sentinel(rows[:start]).all()
    n = gh.check_classification(r["src"], rows, r["counter"][0], start, i, j, r["codes"], r["radial"], hit, idx)
    return n, hit, i, j


@pytest.mark.parametrize("total,N,K,R", gh.CLASSIFY_TOTALS)
def test_edge_feat_classification(h, total, N, K, R):
    """The table classification from a planted code0 (one code field changed; r2 moved by 2 x and by 0.5 x the tolerance): every edge is
    a hit with src = its pair index or a miss with src = 0x80000000 | at and rows[at] its record; the positions are exactly
    start .. start + misses - 1 and the counter ends there (started at 0 and at 1000); codes and radial equal k_edge_feat<0>'s bit for
    bit and the reference.  total = 1, 1023, 1024, 1025 (a partial last workgroup) and 5 x 1024 + 7."""
    assert N * K == total
    c = gh.classify_case(N, K, R)
    n0, hit, i, j = classify(h, c)
    n1, _, _, _ = classify(h, c, start=1000)
    assert n0 == n1
    if total > 1000:
        assert hit.any() and (~hit & ((i < R) == (j < R))).any(), "planted misses and hits both occur"


def test_edge_feat_classification_quiet_first_workgroup_and_all_miss(h):
    """A first workgroup without a miss (s_cnt == 0: no reservation), and a launch in which every edge misses."""
    c = gh.classify_case(1709, 3, 1000, "first_clean")
    _, i, j = gh.edge_ij(c["edges"], c["N"], c["K"])
    n, hit, _, _ = classify(h, c, planted=True, skip_below=10 ** 9)      # nothing planted: intra-chain edges all hit
    assert hit[:1024].all() and 0 < n < hit.size
    c = gh.classify_case(1709, 3, 1000, "all_miss")
    n, hit, _, _ = classify(h, c)
    assert n == hit.size and not hit.any()


# ---- 3b: non-finite poses (include/dfmdock_amd.h: in range, contained, the ordering rule of the graph) -----------------------------------
# Every launch here gets the arrays the test built and writes only its own guarded blocks: nothing follows an edge as an index.
@pytest.mark.parametrize("N", gh.NONFINITE_SIZES)
@pytest.mark.parametrize("kind", sorted(gh.NONFINITE))
def test_knn_sample_non_finite(h, kind, N):
    """B = 3 with the non-finite coordinates in trajectory 1 (one NaN CA; a ligand half of +NaN, of NaN with the sign bit, of signalling /
    negative / all-ones NaN; one residue at +inf and one at -inf), N on both sides of 256 and N = 16 (the degree clamps), 600 and 1030
    (NPL = 12, and 32: the count on the vector pipe), degrees (20, 40) and (60, 0), seed and evaluation index as arguments and from
    ctl.  The graph follows the ordering rule (check_graph: a NaN distance after every number, ties by ascending j; numbers first in
    the race), every edge is a residue index, and trajectories 0 and 2 have the bits of the same launch with trajectory 1 finite."""
    B = 3
    ca4 = gh.COORDS[kind](B, N, seed=N)
    twin = gh.finite_twin(kind, B, N, seed=N)
    b = gh.bad_trajectory(B)
    keep = [t for t in range(B) if t != b]
    assert np.array_equal(ca4[keep], twin[keep]) and not np.isfinite(ca4[b]).all()
    ctl = np.array([STREAM, SEED & 0xFFFFFFFF, SEED >> 32], np.uint32)
    for deg in gh.NONFINITE_DEGREES:
        knn, nsamp = gh.degree_of(N, *deg)
        edges = knn_launch(h, ca4, knn, nsamp)
        assert ((edges >= 0) & (edges < N)).all(), f"edges up to {edges.max()} of N = {N}"
        check_graph(edges, ca4, knn, nsamp)
        ref = knn_launch(h, twin, knn, nsamp)
        np.testing.assert_array_equal(edges[keep], ref[keep])
        np.testing.assert_array_equal(knn_launch(h, ca4, knn, nsamp, seed=99, stream=77, ctl=ctl), edges)


def nonfinite_pose(kind, N, B=3):
    """(n4, ca4, cb4) of a non-finite geometry and of its finite twin (the same backbone offsets), and the bad trajectory."""
    bad = gh.backbone(gh.COORDS[kind](B, N, seed=N), seed=2)
    twin = gh.backbone(gh.finite_twin(kind, B, N, seed=N), seed=2)
    return bad, twin, gh.bad_trajectory(B)


@pytest.mark.parametrize("N", (40, 214))
@pytest.mark.parametrize("kind", sorted(gh.NONFINITE))
def test_edge_feat_non_finite(h, kind, N):
    """k_edge_feat<0> on the reference's own graph of a non-finite pose (in-range edges by the ordering rule, not the kernel's): codes and
    radial are the IEEE restatement (a NaN distance: bin 0 and no angle; +inf: bin 39 and no angle; relpos exact; radial NaN or +inf), and
    the two finite trajectories have the bits of the launch on the finite twin."""
    (n4, ca4, cb4), (tn, tca, tcb), b = nonfinite_pose(kind, N)
    knn, nsamp = gh.degree_of(N)
    c = dict(n4=n4, ca4=ca4, cb4=cb4, edges=gh.ref_graph(ca4, knn, nsamp, SEED, STREAM), B=3, N=N, R=N // 2, K=knn + nsamp, mask_dist=22.0)
    r = feat_launch(h, c)
    ref = gh.edge_case_ref(c)
    und = gh.check_edge_codes(r["codes"], r["radial"], ref, gh.angle_margin(ref))
    assert und <= 0.01 * ref["gate"].size
    _, i, j = gh.edge_ij(c["edges"], N, c["K"])
    tb = np.repeat(np.arange(3), N * c["K"])
    badres = ~np.isfinite(ca4[b, :, :3]).all(1)
    touch = (tb == b) & (badres[i] | badres[j])
    assert touch.any() and not np.isfinite(r["radial"][touch]).any() and np.isfinite(r["radial"][~touch]).all()
    f = gh.unpack_code(r["codes"])
    assert not (f["om"][touch] | f["th"][touch] | f["ph"][touch]).any()
    t = feat_launch(h, dict(c, n4=tn, ca4=tca, cb4=tcb))
    for k in ("codes", "radial"):
        np.testing.assert_array_equal(r[k].view(np.uint32)[tb != b], t[k].view(np.uint32)[tb != b])


@pytest.mark.parametrize("N", (40, 600))
@pytest.mark.parametrize("kind", sorted(gh.NONFINITE))
def test_edge_feat_classification_non_finite(h, kind, N):
    """k_edge_feat<1> on the non-finite trajectory against the table entries of the FINITE pose it was cut from (k_l0_pairs on the twin: the
    stored pose of a complex is always finite): every edge that touches a non-finite residue is a miss - also the pair at +inf whose entry
    holds the same code, a finite pair beyond the last distance bin (inf <= inf would pass; planted at N = 40) -, every other intra-chain
    edge a hit; row
    list, src and counter as the restatement has them, the counter = the number of misses.  And k_l0_pairs on the non-finite pose itself:
    records of every pair at their index, codes and radial those of k_edge_feat<0>."""
    (n4, ca4, cb4), (tn, tca, tcb), b = nonfinite_pose(kind, N)
    R = N // 2
    knn, nsamp = gh.degree_of(N)
    K = knn + nsamp
    edges = gh.ref_graph(ca4[b:b + 1], knn, nsamp, SEED, STREAM)
    if kind == "inf_residue":      # the ligand residue at -inf against the ligand residue that the finite pose has furthest from it (54 A at N = 600)
        edges[0, N - 1, K - 1] = R + int(np.argmax(gh.dist32(tca[b, :, :3])[N - 1, R:]))
    c = dict(n4=n4[b:b + 1], ca4=ca4[b:b + 1], cb4=cb4[b:b + 1], edges=edges, B=1, N=N, R=R, L=N - R, K=K, mask_dist=22.0)
    code0 = pairs_launch(h, dict(c, n4=tn[b:b + 1], ca4=tca[b:b + 1], cb4=tcb[b:b + 1]))["code0"].reshape(-1, 2)
    if kind == "inf_residue" and N == 40:
        # no pair of 20 residues lies beyond the last distance bin (50.75 A): the entry of the planted pair is made that of one at 100 A
        # (distance bin 39, no angle, the pair's relpos), which is what a larger complex holds there (N = 600 has it by itself)
        far = int(edges[0, N - 1, K - 1])
        code0 = code0.copy()
        code0[gh.pair_index(N - 1, far, R, N - R)] = (39 | int(np.clip(N - 1 - far + 32, 0, 64)) << 20, np.array([1e4], np.float32).view(np.uint32)[0])
    r = feat_launch(h, c, cls=dict(code0=code0, capacity=N * K, start=0))
    ref = gh.edge_case_ref(c)
    gh.check_edge_codes(r["codes"], r["radial"], ref, gh.angle_margin(ref))
    _, i, j = gh.edge_ij(edges, N, K)
    hit, idx = gh.hit_ref(i, j, r["codes"], r["radial"], code0, R, N - R)
    misses = gh.check_classification(r["src"], r["rows"].reshape(-1, 4), r["counter"][0], 0, i, j, r["codes"], r["radial"], hit, idx)
    badres = ~np.isfinite(ca4[b, :, :3]).all(1)
    touch = badres[i] | badres[j]
    same = (i < R) == (j < R)
    assert touch.any() and not hit[touch].any() and hit[same & ~touch].all()
    assert misses == int((~hit).sum()) == int(r["counter"][0])
    if kind == "inf_residue":
        loose, _ = gh.hit_ref(i, j, r["codes"], r["radial"], code0, R, N - R, mutant="inf_hits")
        assert (loose & ~hit).any(), "no pair at infinity whose finite entry lies beyond the last bin: inf <= inf was never at stake"
    # k_l0_pairs on the non-finite pose
    p = pairs_launch(h, c)
    ii, jj = gh.all_pairs(R, N - R)
    full = feat_launch(h, dict(c, K=N, edges=np.tile(np.arange(N, dtype=np.int32), (1, N, 1))))
    sel = ii * N + jj
    pref = gh.edge_ref(n4[b], ca4[b], cb4[b], ii, jj, R, 22.0)
    gh.check_edge_codes(full["codes"][sel], full["radial"][sel], pref, gh.angle_margin(pref))
    gh.check_pairs(p["code0"], p["rows"], R, N - R, full["codes"][sel], full["radial"][sel])


# ---- 4: k_clash_force --------------------------------------------------------------------------------------------------------------
def clash_launch(h, c):
    B, R, L = c["B"], c["R"], c["L"]
    r = run(h, "clash_force", dict(rec_pos=c["rec"], lig_cur=Out(np.float32, init=c["lig"]), tr_upd=Out(np.float32, init=c["tr0"])), B=B, R=R, L=L)
    return r["lig_cur"].reshape(B, L * 3, 3), r["tr_upd"].reshape(B, 3)


def check_rigid(lig_in, lig_out, tr_in, tr_out, shift64, bound):
    """All atoms of a trajectory move by the same fp32 vector, bit for bit: one s (within `bound` of the reference shift) has
    out = fl(in + s) for every atom and tr_out = fl(tr_in + s)."""
    for b in range(lig_in.shape[0]):
        for k in range(3):
            s = np.float32(shift64[b, k])
            cands = [s]
            for _ in range(4):
                cands = [np.nextafter(cands[0], np.float32(-np.inf))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
            ok = [x for x in cands if abs(float(x) - shift64[b, k]) <= bound[b, k]
                  and np.array_equal(lig_in[b, :, k] + x, lig_out[b, :, k]) and tr_in[b, k] + x == tr_out[b, k]]
            assert ok, f"trajectory {b} axis {k}: no single fp32 shift explains every atom"


@pytest.mark.parametrize("R,L", gh.CLASH_SIZES)
def test_clash_force(h, R, L):
    """B = 3 different poses; R = 1025 reaches the second receptor chunk, L = 342 the second ligand atom per thread; a coincident pair
    (skipped) and pairs inside the fp32 prefilter but outside 4 A (no force); tr_update starts non-zero and is accumulated."""
    c = gh.clash_case(R, L)
    lig_out, tr_out = clash_launch(h, c)
    shift, scale = gh.clash_ref(c["rec"], c["lig"])
    assert (scale > 0).all()
    lig_in = c["lig"].reshape(c["B"], L * 3, 3)
    sb = 4 * U * scale
    check(f"k_clash_force tr_update R {R} L {L}", tr_out, c["tr0"] + shift, sb + 2 * U * np.abs(c["tr0"] + shift), "k_clash_force tr_update")
    want = lig_in + shift[:, None, :]
    check(f"k_clash_force pose R {R} L {L}", lig_out, want, sb[:, None, :] + 2 * U * np.abs(want), "k_clash_force pose")
    check_rigid(lig_in, lig_out, c["tr0"], tr_out, shift, sb + 1e-300)


def test_clash_force_without_contact(h):
    """No pair inside 4 A: the shift is exactly 0, the pose and tr_update unchanged bit for bit."""
    c = gh.clash_case(300, 40)
    c["lig"] = (c["lig"] + np.float32(500.0)).astype(np.float32)
    lig_out, tr_out = clash_launch(h, c)
    np.testing.assert_array_equal(lig_out.view(np.uint32).reshape(-1), c["lig"].view(np.uint32).reshape(-1))
    np.testing.assert_array_equal(tr_out.view(np.uint32), c["tr0"].view(np.uint32))


@pytest.mark.parametrize("R,L", ((300, 40), (9, 342)))
@pytest.mark.parametrize("where,value", (((7, 2), np.nan), ((0, 4), np.inf), ((-1, 8), -np.inf)), ids=("nan_in_N", "inf_in_CA", "neg_inf_in_C"))
def test_clash_force_non_finite(h, R, L, where, value):
    """One NaN or infinite coordinate in ONE atom of trajectory 1 of B = 3.  That atom passes no d^2 < 16.5 and would be dropped from the
    force while the rest of the pose is moved by a finite shift: the pose gets a NaN shift instead - every coordinate of it and its
    tr_update are NaN - and trajectories 0 and 2 have the bits of the launch with trajectory 1 finite (guards: run).  L = 342: the
    second ligand atom per thread."""
    c = gh.clash_case(R, L)
    good_lig, good_tr = clash_launch(h, c)
    bad = dict(c, lig=c["lig"].copy())
    bad["lig"][1, where[0], where[1]] = value
    lig, tr = clash_launch(h, bad)
    assert np.isfinite(good_lig).all() and np.isfinite(good_tr).all()
    for got, ref in ((lig, good_lig), (tr, good_tr)):
        np.testing.assert_array_equal(got[[0, 2]].view(np.uint32), ref[[0, 2]].view(np.uint32))
    assert np.isnan(lig[1]).all() and np.isnan(tr[1]).all(), "a non-finite pose kept numbers through the clash force"


# ---- 5: k_init_pose ----------------------------------------------------------------------------------------------------------------
def init_launch(h, c, all_atoms, R0=None, draw=None, seed=0):
    B, L = c["B"], c["L"]
    r = run(h, "init_pose", dict(rec_pos=c["rec"], lig0=c["lig"], R0=R0, tr_draw=draw, lig_cur=Out(np.float32, B * L * 9),
                                 tr_upd=Out(np.float32, B * 3), rot_upd=Out(np.float32, B * 3)), B=B, R=c["R"], L=L, all_atoms=all_atoms, seed=seed)
    return r["lig_cur"].reshape(B, L * 3, 3), r["tr_upd"].reshape(B, 3), r["rot_upd"].reshape(B, 3)


def check_init(tag, c, all_atoms, got, Rm, draw, dR, ddraw):
    """x' = R0 (x - c2) + c2 + tr, tr = (draw - c2) + c1, rot_update = axis-angle(R0) compared as a rotation matrix."""
    from heads_harness import aa_to_mat64
    lig_out, tr_out, rot_out = got
    c1, c2 = gh.centroid64(c["rec"], all_atoms), gh.centroid64(c["lig"], all_atoms)
    x = c["lig"].reshape(-1, 3).astype(np.float64)
    rad = np.linalg.norm(x - c2, axis=1).max()
    for b in range(c["B"]):
        tr = (draw[b] - c2) + c1
        dtr = ddraw[b] + 4 * U * (np.abs(draw[b]).max() + np.abs(c1).max() + np.abs(c2).max())
        want = (x - c2) @ Rm[b].T + c2 + tr
        dpose = 2 * rad * (dR[b] + 32 * U) + dtr + 8 * U * (np.abs(x).max() + np.abs(c2).max() + np.abs(tr).max())
        check(f"k_init_pose pose {tag} b {b}", lig_out[b], want, dpose, f"k_init_pose pose {tag.split()[0]}")
        check(f"k_init_pose tr_update {tag} b {b}", tr_out[b], tr, dtr, f"k_init_pose tr_update {tag.split()[0]}")
        check(f"k_init_pose rot_update {tag} b {b}", aa_to_mat64(rot_out[b]), Rm[b], 2 * dR[b] + 256 * U, f"k_init_pose rot_update {tag.split()[0]}")


@pytest.mark.parametrize("all_atoms", (0, 1))
@pytest.mark.parametrize("L", (1, 85, 86, 300))
def test_init_pose_injected(h, L, all_atoms):
    """Injected R0 and tr_draw, B = 5; L = 86 is the first ligand with a second pass of the 256-thread atom loop; the centroids over the
    CA atoms and (all_atoms) over all backbone atoms."""
    c = gh.init_case(L)
    got = init_launch(h, c, all_atoms, R0=c["R0"], draw=c["draw"])
    Rm = c["R0"].astype(np.float64).reshape(-1, 3, 3)
    check_init(f"injected L {L} all_atoms {all_atoms}", c, all_atoms, got, Rm, c["draw"].astype(np.float64), np.zeros(c["B"]), np.zeros(c["B"]))


@pytest.mark.parametrize("L,all_atoms,seed", ((86, 0, 0x5EED00000001), (300, 1, 7), (85, 0, gh.TOP_UNIFORM_INIT_SEED)))
def test_init_pose_native(h, L, all_atoms, seed):
    """Native draws: the Philox words recomputed on the host, quaternion and translation in float64.  The third seed gives trajectory
    gh.TOP_UNIFORM_INIT_B a first uniform of exactly 1.0f: sqrt(-2 ln 1) = 0, a zero quaternion component."""
    c = gh.init_case(L)
    got = init_launch(h, c, all_atoms, seed=seed)
    B = c["B"]
    Rm, draw, dR, dd, keep = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros(B), np.zeros(B), []
    for b in range(B):
        q, t, dz, ua = gh.init_draws64(b, seed)
        Rm[b], draw[b] = gh.quat_to_mat64(q), t
        dR[b], dd[b] = 4 * dz[:4].max() / np.linalg.norm(q) + 2 * U, 30 * dz[4:].max() + 2 * U * np.abs(t).max()
        if ua.min() >= 2.0 ** -20:
            keep.append(b)
    assert len(keep) >= B - 1
    if seed == gh.TOP_UNIFORM_INIT_SEED:
        b = gh.TOP_UNIFORM_INIT_B
        assert b in keep and gh.init_draws64(b, seed)[0][0] == 0.0
    sub = dict(c, B=len(keep))
    check_init(f"native L {L} all_atoms {all_atoms}", sub, all_atoms, tuple(g[keep] for g in got), Rm[keep], draw[keep], dR[keep], dd[keep])


# ---- 7: the largest complex ----------------------------------------------------------------------------------------------------------
def test_complex_create_refuses_more_than_4096_residues(blob):
    """k_knn_sample<64> holds 4 x 64 x 16 = 4096 candidates per node and would silently lose the rest: dfm_complex_create refuses
    R + L > 4096 (dfm_internal.h: MAX_NODES) with DFM_E_INVALID before it allocates anything, so no complex exceeds that size.
    Minimal feature arrays: the check comes before any of them is read."""
    import ctypes as C
    from dfmdock_amd import _lib, engine
    model = engine.Model(blob)
    L = _lib.lib()
    z = np.zeros(16, np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    for R, Lg in ((4096, 1), (1, 4096), (16384, 1), (0, 5)):
        hnd = L.dfm_complex_create(model._h, p, p, p, p, R, Lg)
        assert not hnd
        assert b"4096" in L.dfm_last_error()
    model.close()
