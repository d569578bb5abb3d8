"""The kernel harness of the graph front end and the pose kernels without a GPU (tests/geom_harness.py, tests/kernels/geom_harness.hip):
the shim builds and links against the library's launchers; the numpy Philox and u01 equal the library's host functions bit for bit; the
references agree with the project's CPU oracle on a small complex; each seeded mutant of a reference is rejected by the very comparison
the GPU tests use; the exclusion caps (undecided nodes <= 2 %, undecided edges <= 1 %) hold on the GPU tests' own inputs; u01 is
monotone with smallest value 2^-25 and largest value exactly 1.0f.  Non-finite poses: the ordering rule of the graph against a plain
Python sort; the selection as it stood before the rule (present_selection) is rejected on every non-finite geometry and accepted on the
three finite ones; the features and the table-hit predicate on NaN and infinite coordinates."""

import numpy as np
import pytest

import geom_harness as gh
import kernel_harness as kh


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return gh.compile_shim(tmp_path_factory.mktemp("geom_harness"))


@pytest.fixture(scope="module")
def h(shim):
    return gh.Harness(shim)      # also checks that the ctypes call record has the shim's size


def test_library_exports_the_launchers():
    out = kh.exported_symbols(gh.LIBDIR + "/libdfmdock_amd.so", True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in gh.LAUNCHERS:
        assert s in syms, s


def test_shim_links(shim, h):
    out = kh.exported_symbols(shim, False)
    for s in gh.LAUNCHERS:
        assert s in out, s
    assert h.guard >= 1024
    assert h.lib.gh_rng_edges() == gh.RNG_EDGES and h.lib.gh_rng_init() == gh.RNG_INIT
    assert h.lib.gh_pack_code(39, 23, 22, 11, 65) == 39 | 23 << 6 | 22 << 11 | 11 << 16 | 65 << 20
    f = gh.unpack_code(np.array([h.lib.gh_pack_code(39, 23, 22, 11, 65)], np.uint32))
    assert [int(f[k][0]) for k in ("bd", "om", "th", "ph", "rp")] == [39, 23, 22, 11, 65]


# ---- Philox and u01 ----------------------------------------------------------------------------------------------------------------
def test_philox_and_u01_restatements_are_bit_exact(h):
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    c[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 0, 0], [76, 12 << 8, 230, 1]]
    for k0, k1 in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0x99ABCDEF, 0x12345678)):
        np.testing.assert_array_equal(h.philox(c, k0, k1), np.stack(gh.philox_np(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k0, k1), -1))
    x = rng.integers(0, 2 ** 32, 8192, dtype=np.uint64).astype(np.uint32)
    x[:6] = [0, 0xFF, 0x100, 0x7FFFFFFF, 0xFFFFFF00, 0xFFFFFFFF]
    np.testing.assert_array_equal(h.u01(x).view(np.uint32), gh.u01_np(x).view(np.uint32))


def test_u01_range(h):
    """u01 is monotone (non-decreasing: above 2^23 the + 0.5f rounds to even, so neighbours merge) over the 2^24 inputs; its smallest
    value is 2^-25 and its LARGEST IS EXACTLY 1.0f (16777215.5 rounds to 2^24) - 'never 0' holds, 'never 1' does not.  The consumers:
    the race key -log2(1) d^3 is zero (k_knn_sample clears its sign: the candidate wins), Box-Muller's sqrt(-2 ln 1) is 0 and cos(2 pi 1)
    is 1 - both finite (GPU: test_knn_sample_uniform_of_one, test_init_pose_native)."""
    mono, lo, hi = h.u01_scan()
    assert mono == 1
    assert lo == np.float32(2.0 ** -25) and hi == np.float32(1.0)
    assert gh.u01_np(np.uint32(0xFFFFFF00)) == np.float32(1.0) and gh.u01_np(np.uint32(0xFFFFFD00)) < np.float32(1.0)


def test_top_uniform_records(h):
    """The committed counters whose uniform is exactly 1.0f are what the bounded host search finds, and candidate 49 races."""
    assert h.find_top_uniform(183, 16, 256, 1 << 20, 0, gh.RNG_EDGES, gh.TOP_UNIFORM_SEED) == gh.TOP_UNIFORM_EDGE
    assert h.find_top_uniform(5, 4, 1, 1 << 24, 1, gh.RNG_INIT, 0) == (gh.TOP_UNIFORM_INIT_SEED, gh.TOP_UNIFORM_INIT_B, 0, 0)
    stream, node, blk, word = gh.TOP_UNIFORM_EDGE
    j = 4 * blk + word
    assert gh.edge_stream_u([node], 61, stream, gh.TOP_UNIFORM_SEED)[0, j] == np.float32(1.0)
    ca = gh.top_uniform_coords()
    assert j not in gh.knn_ref(gh.dist32(ca[node // 61, :, :3]), 20)[node % 61]
    assert gh.init_draws64(gh.TOP_UNIFORM_INIT_B, gh.TOP_UNIFORM_INIT_SEED)[3][0] == 1.0


# ---- the references against the oracle -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    from dfmdock_amd.synthetic import make_complex
    cx = make_complex(24, 16, seed=5)
    pos = np.concatenate([cx["rec_pos"], cx["lig_pos"]], 0).astype(np.float32)
    pos = pos - pos[24:, 1].mean(0, dtype=np.float64).astype(np.float32)
    return cx, pos


def test_references_agree_with_the_oracle(small):
    """kNN slots (exact), distance / angle bins and relpos of all N x N pairs, and the clash force, against oracle/dfm_oracle.c."""
    from oracle import oracle as ora
    cx, pos = small
    N, R = pos.shape[0], 24
    ca = pos[:, 1]
    np.testing.assert_array_equal(gh.knn_ref(gh.dist32(ca), 20), ora.knn_sample(ca, seed=1)[:, :20])
    n4, ca4, cb4 = (x[0] for x in gh.backbone_from_pos(pos[None]))
    ii, jj = np.repeat(np.arange(N), N), np.tile(np.arange(N), N)
    ref = gh.edge_ref(n4, ca4, cb4, ii, jj, R, 22.0)
    bins = ora.bins_full(pos).reshape(N * N, 4).astype(np.int64)
    np.testing.assert_array_equal(ref["bd"], bins[:, 0])
    np.testing.assert_array_equal(ref["rp"], ora.relpos_full(R, N - R).reshape(-1))
    m = gh.angle_margin(ref)
    und = gh.angle_undecided(ref, m)
    for k, bounds in enumerate((gh.ANGLE_BOUNDS, gh.ANGLE_BOUNDS, gh.PHI_BOUNDS)):
        want = np.where(ref["gate"], gh._bins(ref["a64"][:, k], bounds), 0)
        dec = ~und[:, k]
        np.testing.assert_array_equal(want[dec], bins[dec, 1 + k])
    assert und.any(1).sum() <= 0.01 * N * N
    import torch
    np.testing.assert_array_equal(gh.ANGLE_BOUNDS, torch.linspace(-180, 180, 23).numpy())
    np.testing.assert_array_equal(gh.DIST_BOUNDS, torch.linspace(3.25, 50.75, 39).numpy())
    c = gh.clash_case(30, 12, B=2)
    shift, scale = gh.clash_ref(c["rec"], c["lig"])
    for b in range(2):
        got = ora.clash_force(c["rec"].reshape(-1, 3, 3), c["lig"][b].reshape(-1, 3, 3))
        assert np.abs(got - shift[b]).max() <= 1e-5 * max(1.0, scale[b].max())


# ---- the comparisons have power: seeded mutants of the references are rejected --------------------------------------------------------
def graph_ref(ca4, knn, nsamp, seed, stream, tie=None, race=None, pick=None):
    """The reference's own edges [B][N][K] (optionally a mutant's)."""
    B, N = ca4.shape[:2]
    out = np.zeros((B, N, knn + nsamp), np.int32)
    for b in range(B):
        d = gh.dist32(ca4[b, :, :3])
        near = gh.knn_ref(d, knn, tie)
        key, _ = gh.race_keys(d, near, gh.edge_stream_u(b * N + np.arange(N), N, stream, seed), gh.LOG2_PROVISIONAL, race)
        out[b] = np.concatenate([near, gh.sample_ref(key, nsamp, pick, near=None if np.isfinite(d).all() else near)], 1)
    return out


def graph_check(edges, ca4, knn, nsamp, seed, stream):
    """The comparison of the GPU tests (geom_harness.check_graph), with the provisional envelope."""
    return gh.check_graph(edges, ca4, knn, nsamp, seed, stream, gh.LOG2_PROVISIONAL)


@pytest.mark.parametrize("mutant", ("tie_high", "all_keys", "largest", "stream_per_trajectory"))
def test_graph_mutants_are_rejected(mutant):
    """Ties broken by the highest index; the 40 smallest of ALL keys, kNN winners included; the 40 largest keys; the counter's node word
    i instead of b N + i.  The unmutated reference passes the same comparison."""
    ca4 = gh.lattice_coords(2, 130, seed=9)
    args = (20, 40, 0x1234567899ABCDEF, 3)
    assert graph_check(graph_ref(ca4, *args), ca4, *args) == 0
    if mutant == "stream_per_trajectory":
        bad = np.stack([graph_ref(ca4[b:b + 1], *args)[0] for b in range(2)])
    else:
        bad = graph_ref(ca4, *args, **{"tie_high": dict(tie="tie_high"), "all_keys": dict(race="all_keys"), "largest": dict(pick="largest")}[mutant])
    with pytest.raises(AssertionError):
        graph_check(bad, ca4, *args)


def test_edge_mutant_ge_is_rejected():
    """>= instead of > at a distance-bin boundary, on the pose with distances ON boundaries."""
    c = gh.edge_case(*gh.EDGE_CASES[0])
    _, i, j = gh.edge_ij(c["edges"], c["N"], c["K"])
    ref = gh.edge_case_ref(c)
    m = gh.angle_margin(ref)

    def codes_of(r):
        b = [np.where(r["gate"], gh._bins(r["a64"][:, k], bd), 0) for k, bd in enumerate((gh.ANGLE_BOUNDS, gh.ANGLE_BOUNDS, gh.PHI_BOUNDS))]
        return (r["bd"] | b[0] << 6 | b[1] << 11 | b[2] << 16 | r["rp"] << 20).astype(np.uint32)
    assert gh.check_edge_codes(codes_of(ref), ref["r2"], ref, m) == 0
    bad = gh.edge_ref(c["n4"][0], c["ca4"][0], c["cb4"][0], i, j, c["R"], c["mask_dist"], mutant="ge")
    with pytest.raises(AssertionError):
        gh.check_edge_codes(codes_of(bad), bad["r2"], ref, m)


def test_pair_index_and_tolerance_mutants_are_rejected():
    """The receptor and ligand blocks swapped in the pair index; the r2 tolerance without the max(sqrt(r2), 1) factor."""
    R, L = 17, 16
    N = R + L
    n4, ca4, cb4 = (x[0] for x in gh.backbone(gh.chain_coords(1, N, seed=31), seed=4))
    ii, jj = gh.all_pairs(R, L)
    ref = gh.edge_ref(n4, ca4, cb4, ii, jj, R, 22.0)
    codes = (ref["bd"] | ref["rp"] << 20).astype(np.uint32)
    rec = np.stack([ii, jj, codes, ref["r2"].view(np.uint32)], 1).astype(np.uint32)

    def table(mut):
        q = gh.pair_index(ii, jj, R, L, mut)
        rows, code0 = np.zeros((len(q), 4), np.uint32), np.zeros((len(q), 2), np.uint32)
        rows[q], code0[q] = rec, rec[:, 2:]
        return code0, rows
    gh.check_pairs(*table(None), R, L, codes, ref["r2"])
    with pytest.raises(AssertionError):
        gh.check_pairs(*table("blocks_swapped"), R, L, codes, ref["r2"])
    # classification of every pair against a planted table: the mutant's hit set differs (0.5 x the tolerance at sqrt(r2) > 2)
    code0 = gh.plant(table(None)[0], ref["r2"], None)
    hit, idx = gh.hit_ref(ii, jj, codes, ref["r2"], code0, R, L)
    bad, _ = gh.hit_ref(ii, jj, codes, ref["r2"], code0, R, L, mutant="no_sqrt")
    assert hit.any() and (~hit).any() and (hit != bad).any()

    def outputs(hm):
        src = np.where(hm, idx, 0).astype(np.uint32)
        at = np.cumsum(~hm) - 1
        src[~hm] = gh.MISS | at[~hm].astype(np.uint32)
        rows = np.full((len(hm), 4), 0xFFFFFFFF, np.uint32)
        rows[at[~hm]] = rec[~hm]
        return src, rows, int((~hm).sum())
    gh.check_classification(*outputs(hit), 0, ii, jj, codes, ref["r2"], hit, idx)
    with pytest.raises(AssertionError):
        gh.check_classification(*outputs(bad), 0, ii, jj, codes, ref["r2"], hit, idx)


# ---- the exclusion caps on the GPU tests' inputs ---------------------------------------------------------------------------------------
def test_lattice_inputs_have_ties_at_the_knn_th_distance():
    for N in (61, 257, 1025):
        ca = gh.lattice_coords(1, N, seed=N)
        d = np.sort(gh.dist32(ca[0, :, :3]), axis=1)
        assert (d[:, 19] == d[:, 20]).mean() > 0.5, N


# every sampling case up to N = 1025, and one per wide instantiation (NPL = 32: N = 2049, NPL = 64: N = 4093); the other large cases are
# left to the GPU test, which repeats the count at every size (the float64 race of 4096 x 4096 candidates costs seconds here)
CAP_CASES = [c for c in gh.knn_cases() if c[4] > 0 and (c[1] <= 1025 or c in (("chain", 2049, 1, 20, 40), ("chain", 4093, 1, 20, 40)))]


@pytest.mark.parametrize("case", CAP_CASES, ids=gh.knn_case_id)
def test_undecided_nodes_stay_under_the_cap(case):
    """At most 2 % of the nodes of a case are undecided with the provisional envelope (2^-20 relative, 2^-24 absolute), which contains
    the measured one (the GPU test repeats the count with the measured envelope at every size)."""
    kind, N, B, knn, nsamp = case
    knn, nsamp = gh.degree_of(N, knn, nsamp)
    if nsamp == 0:
        return
    assert gh.LOG2_ENVELOPE[0] <= gh.LOG2_PROVISIONAL[0] and gh.LOG2_ENVELOPE[1] <= gh.LOG2_PROVISIONAL[1]
    ca4 = gh.COORDS[kind](B, N, seed=N)
    und = graph_check(graph_ref(ca4, knn, nsamp, 0x1234567899ABCDEF, 3), ca4, knn, nsamp, 0x1234567899ABCDEF, 3)
    assert und <= 0.02 * B * N, (und, B * N)


def test_undecided_edges_stay_under_the_cap():
    """The angle margin m of every edge case (printed; the GPU docstring quotes its size) leaves at most 1 % of the edges undecided,
    the boundary pose has distances ON bin boundaries and NaN angles."""
    worst = 0.0
    for case in gh.EDGE_CASES:
        ref = gh.edge_case_ref(gh.edge_case(*case))
        m = gh.angle_margin(ref)
        worst = max(worst, m)
        print(case, "m =", m, "undecided", int(gh.angle_undecided(ref, m).any(1).sum()), "of", ref["gate"].size)
        assert gh.angle_undecided(ref, m).any(1).sum() <= 0.01 * ref["gate"].size
        assert (~ref["gate"]).any(), "no masked pair"
        if case[0] == "chain":      # relpos offsets below -32 (field 0) and above +32 (64), and inter-chain pairs (65) in both chain orders
            c = gh.edge_case(*case)
            _, i, j = gh.edge_ij(c["edges"], c["N"], c["K"])
            assert {0, 64, 65} <= set(ref["rp"].tolist())
            assert ((i < c["R"]) & (j >= c["R"])).any() and ((j < c["R"]) & (i >= c["R"])).any()
            assert (ref["rp"][(i < c["R"]) != (j < c["R"])] == 65).all() and (ref["rp"][(i < c["R"]) == (j < c["R"])] <= 64).all()
        if case[0] == "boundary":
            assert (np.sqrt(ref["r2"])[:, None] == gh.DIST_BOUNDS[None, :]).any(1).sum() >= 5
    assert worst < 0.02


def test_batches_cover_the_early_wave_exit():
    """B N is no multiple of 4 at least once in every instantiation class."""
    cls = lambda N: 4 if N <= 256 else 8 if N <= 512 else 12 if N <= 768 else 16 if N <= 1024 else 32 if N <= 2048 else 64
    seen = {cls(c[1]) for c in gh.knn_cases() if (c[1] * c[2]) % 4}
    assert seen == {4, 8, 12, 16, 32, 64}


# ---- non-finite poses: the ordering rule of the graph, the selection as it stood as a named mutant ------------------------------------
MUTANT_SIZES = (40, 214, 257, 600)


def rule5_rows(d, knn, rows):
    """The ordering rule written out with Python's sort, independent of knn_ref's packed word: numbers by (d, j), then NaN by j."""
    return np.array([sorted(range(d.shape[1]), key=lambda j: (bool(np.isnan(d[i, j])), 0.0 if np.isnan(d[i, j]) else float(d[i, j]), j))[:knn]
                     for i in rows], np.int32)


@pytest.mark.parametrize("N", MUTANT_SIZES)
@pytest.mark.parametrize("kind", sorted(gh.NONFINITE))
def test_present_selection_is_rejected_on_non_finite_poses(kind, N):
    """knn_ref follows the ordering rule (against a plain Python sort, on the nodes that see a non-finite distance and on a sample of the
    others).  The selection as it stood (gh.present_selection: words of the raw distances, +inf in the padding slots) is rejected by the
    comparison the GPU tests use, on the trajectory that holds the non-finite coordinates.  Where a node has fewer than knn number
    distances it takes padding slots (j >= N) or, with the sign bit set in every word, nothing at all - check_knn alone rejects that.
    inf_residue has ONE NaN per row (inf - inf, the residue at infinity against itself), which orders above the padding just as the
    rule asks, and the +inf distances tie with the padding by ascending index with the residues first: its kNN slots are right, and the
    assertion below says so.  Its defect is in the race - `d != inf` took every residue at infinity, and from it every other residue,
    for no candidate and the kNN winners were drawn a second time - and check_sampled rejects the race as it stood
    (gh.present_race: the same word-level selection on the old race words)."""
    B, knn = 3, 20
    ca4 = gh.COORDS[kind](B, N, seed=N)
    b = gh.bad_trajectory(B)
    assert not np.isfinite(ca4[b]).all() and np.isfinite(np.delete(ca4, b, 0)).all()
    d = gh.dist32(ca4[b, :, :3])
    ref = gh.knn_ref(d, knn)
    rows = np.unique(np.concatenate([np.flatnonzero(~np.isfinite(d).all(1))[:40], np.arange(0, N, 37)]))
    np.testing.assert_array_equal(ref[rows], rule5_rows(d, knn, rows))
    gh.check_knn(ref, ref)
    bad = gh.present_selection(d, knn)
    if kind == "inf_residue":
        gh.check_knn(bad, ref)
        nsamp = min(40, N - knn)
        u = gh.edge_stream_u(b * N + np.arange(N), N, 3, 0x1234567899ABCDEF)
        key, bound = gh.race_keys(d, ref, u, gh.LOG2_PROVISIONAL)
        assert gh.check_sampled(gh.sample_ref(key, nsamp, near=ref), ref, key, bound, nsamp) == 0
        # the race as it stood, word for word through present_select: it is right on the nodes that see the two residues at infinity
        # from afar, and wrong on those two nodes - every word of their rows is +inf, the ties go by index from slot 0 on, and the
        # kNN winners are drawn a second time
        old = gh.present_race(d, ref, u, nsamp)
        rows = np.flatnonzero(np.isinf(d).sum(1) > 2)
        assert rows.size == 2 and ((old[rows][:, :, None] == ref[rows][:, None, :]).any(2)).any()
        with pytest.raises(AssertionError):
            gh.check_sampled(old, ref, key, bound, nsamp)
    else:
        with pytest.raises(AssertionError):
            gh.check_knn(bad, ref)
        assert (bad >= N).any() or (bad < 0).any(), "the defect is an index out of range or a slot never written"


@pytest.mark.parametrize("N", MUTANT_SIZES + (256,))
@pytest.mark.parametrize("kind", ("chain", "lattice", "coincident"))
def test_present_selection_is_accepted_on_finite_poses(kind, N):
    """On the three finite geometries the selection as it stood IS the reference (ties at the knn-th distance and coincident residues
    included): the extended comparison sees the defect and nothing else."""
    ca4 = gh.COORDS[kind](1, N, seed=N)
    d = gh.dist32(ca4[0, :, :3])
    gh.check_knn(gh.present_selection(d, 20), gh.knn_ref(d, 20))


def test_issue_table_of_the_present_selection():
    """One NaN node, knn = 20: 20 of 20 picks in the padding at N = 40, 214, 600 (largest j = N + 19) with either sign; at N = 256 (no
    padding) the picks are in range with a positive NaN and NOTHING is picked with the sign bit set."""
    for N, neg in ((40, 0), (40, 1), (214, 0), (214, 1), (600, 0), (600, 1), (256, 0), (256, 1)):
        keys = np.full(64 * gh.npl_of(N), 0x7F800000, np.uint32)
        keys[:N] = 0xFFC00000 if neg else 0x7FC00000
        win = np.flatnonzero(gh.present_select(keys, 20))
        if N == 256:
            assert (win.size == 0) if neg else (win.tolist() == list(range(20)))
        else:
            assert win.tolist() == list(range(N, N + 20))


@pytest.mark.parametrize("kind", sorted(gh.NONFINITE))
def test_graph_reference_and_mutants_on_non_finite_poses(kind):
    """The reference's own graph passes check_graph on every non-finite geometry (N = 40: fewer than nsamp number candidates on the nodes
    of the NaN ligand; N = 214: enough of them).  Rejected: NaN candidates drawn before the numbers; an edge out of range; on the
    finite trajectories, the old mutants still (ties broken high)."""
    args = (0x1234567899ABCDEF, 3)
    for N in (40, 214):
        knn, nsamp = gh.degree_of(N)
        ca4 = gh.COORDS[kind](3, N, seed=N)
        good = graph_ref(ca4, knn, nsamp, *args)
        assert graph_check(good, ca4, knn, nsamp, *args) <= 0.02 * 3 * N
        b = gh.bad_trajectory(3)
        d = gh.dist32(ca4[b, :, :3])
        near = gh.knn_ref(d, knn)
        key, _ = gh.race_keys(d, near, gh.edge_stream_u(b * N + np.arange(N), N, args[1], args[0]), gh.LOG2_PROVISIONAL)
        cand_nan = np.isnan(key)
        np.put_along_axis(cand_nan, near.astype(np.int64), False, axis=1)
        bad = good.copy()
        bad[b, :, knn:] = gh.sample_ref(key, nsamp, "nan_first", near=near)
        differs = (np.sort(bad[b, :, knn:], 1) != np.sort(good[b, :, knn:], 1)).any()
        # (at N = 40, K = N: every candidate of a node is drawn, in whichever order)
        assert cand_nan.any() and (differs or N == 40)
        if differs:
            with pytest.raises(AssertionError):
                graph_check(bad, ca4, knn, nsamp, *args)
        bad = good.copy()
        bad[b, N - 1, knn + nsamp - 1] = N
        with pytest.raises(AssertionError):
            graph_check(bad, ca4, knn, nsamp, *args)
        bad = good.copy()
        bad[0] = graph_ref(ca4[:1], knn, nsamp, *args, tie="tie_high")[0]
        if (bad[0] != good[0]).any():
            with pytest.raises(AssertionError):
                graph_check(bad, ca4, knn, nsamp, *args)


def test_edge_reference_on_non_finite_poses():
    """edge_ref and hit_ref with IEEE comparisons: on an edge that touches a NaN residue every `>` count is 0 (distance bin 0, angle bins
    0: the gate d < mask_dist fails), on one that touches a residue at infinity the distance bin is 39 and the gate fails; relpos is exact;
    radial is NaN resp. +inf; such a pair is never a table hit - also not against an entry that holds the very same code and r2 bits
    (mutant 'inf_hits', the comparison inf <= inf: rejected by check_classification)."""
    N, R, K = 40, 20, 40
    for kind in sorted(gh.NONFINITE):
        ca4 = gh.COORDS[kind](1, N, seed=N)
        n4, ca4, cb4 = gh.backbone(ca4, seed=2)
        badres = ~np.isfinite(ca4[0, :, :3]).all(1)
        i, j = np.repeat(np.arange(N), K), np.tile(np.arange(K), N)
        ref = gh.edge_ref(n4[0], ca4[0], cb4[0], i, j, R, 22.0)
        touch = badres[i] | badres[j]
        assert touch.any() and (~touch).any()
        assert not np.isfinite(ref["r2"][touch]).any() and np.isfinite(ref["r2"][~touch]).all()
        assert not ref["gate"][touch].any()
        nan = np.isnan(ref["r2"])
        assert (ref["bd"][nan] == 0).all() and (ref["bd"][np.isinf(ref["r2"])] == 39).all()
        same = (i < R) == (j < R)
        np.testing.assert_array_equal(ref["rp"], np.where(same, np.clip(i - j + 32, 0, 64), 65))
        codes = (ref["bd"] | ref["rp"] << 20).astype(np.uint32)
        P = R * R + (N - R) * (N - R)
        code0 = np.zeros((P, 2), np.uint32)
        q = gh.pair_index(i[same], j[same], R, N - R)
        # the entry of every pair IS this pose's record; a pair at infinity has the entry of a finite pair beyond the last bin (100 A)
        code0[q, 0], code0[q, 1] = codes[same], np.where(np.isinf(ref["r2"][same]), np.float32(1e4), ref["r2"][same]).view(np.uint32)
        hit, idx = gh.hit_ref(i, j, codes, ref["r2"], code0, R, N - R)
        assert not hit[touch].any() and hit[same & ~touch].all()
        if kind == "inf_residue":
            loose, _ = gh.hit_ref(i, j, codes, ref["r2"], code0, R, N - R, mutant="inf_hits")
            assert (loose & ~hit).any()
            src = np.where(loose, idx, 0).astype(np.uint32)
            at = np.cumsum(~loose) - 1
            src[~loose] = gh.MISS | at[~loose].astype(np.uint32)
            rows = np.full((i.size, 4), 0xFFFFFFFF, np.uint32)
            rows[at[~loose]] = np.stack([i, j, codes, ref["r2"].view(np.uint32)], 1).astype(np.uint32)[~loose]
            with pytest.raises(AssertionError):
                gh.check_classification(src, rows, int((~loose).sum()), 0, i, j, codes, ref["r2"], hit, idx)
