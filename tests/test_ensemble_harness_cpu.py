"""The kernel harness of the clustering and consensus kernels without a GPU (tests/ensemble_harness.py,
tests/kernels/ensemble_harness.hip): the shim builds and links against the library's launchers and every refusal leaves the host
guards zero; the numpy restatements of the kernels agree with the float64 definitions on the GPU tests' own inputs (the RMSD within
the gate, every integer exactly); the border pairs stay under the caps on those inputs; and each seeded mutant of a restatement is
refused by a comparison the GPU tests use."""
import fractions

import numpy as np
import pytest

import ensemble_harness as eh
import kernel_harness as kh
from ensemble_harness import Out, f32, i32, u32, u64


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return eh.compile_shim(tmp_path_factory.mktemp("ensemble_harness"))


def test_library_exports_the_launchers():
    out = kh.exported_symbols(eh.LIBDIR + "/libdfmdock_amd.so", True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in eh.LAUNCHERS:
        assert s in syms, s


def test_shim_links(shim):
    out = kh.exported_symbols(shim, False)
    for s in eh.LAUNCHERS:
        assert s in out, s
    own = kh.exported_symbols(shim, True)
    assert "kh_run" in own and "__device_stub__" not in own, "the shim adds no kernel of its own"
    h = eh.Harness(shim)      # also checks that the ctypes call record has the shim's size
    assert h.guard >= 1024 and h.check


def refused(h, op, bufs, **scalars):
    r = h.run(op, bufs, check=False, **scalars)
    assert r["err"] == eh.HIP_INVALID_VALUE, (op, sorted(scalars))
    for k, v in bufs.items():
        if isinstance(v, Out):
            assert not r[k + "_guard"][0].any() and not r[k + "_guard"][1].any(), f"{op}: the {k} block was touched"
    return True


def test_shim_refuses_before_touching_a_device(shim):
    """Every check of the shim: hipErrorInvalidValue, and the host guards of every output stay zero - nothing was allocated, uploaded,
    launched or copied back (this runs without a GPU)."""
    h = eh.Harness(shim)
    B, L = 5, 4
    x = np.zeros((B, L, 9), f32)
    W = eh.words32(B)
    pose = dict(B=B, L=L, n_res=L, radius=1.0)
    assert refused(h, "pose_rmsd", dict(X=x, rmsd=Out(f32, B * B - 1)), **pose)                              # output too small
    assert refused(h, "pose_rmsd", dict(X=x[:-1], rmsd=Out(f32, B * B)), **pose)                             # input too small
    assert refused(h, "pose_rmsd", dict(X=x, rmsd=np.zeros(B * B, f32)), **pose)                             # output not flagged
    assert refused(h, "pose_rmsd", dict(X=x, rmsd=Out(f32, B * B)), **dict(pose, n_res=2))                   # no subset, n_res != L
    assert refused(h, "pose_rmsd", dict(X=x, rmsd=Out(f32, B * B)), **dict(pose, B=0))
    assert refused(h, "pose_rmsd", dict(X=x, rmsd=Out(f32, B * B)), **dict(pose, B=65537))
    for res in ([0, 4], [-1, 2], [1, 1]):                                                                   # out of [0, L), repeated
        assert refused(h, "pose_rmsd", dict(X=x, res=np.array(res, i32), rmsd=Out(f32, B * B)), **dict(pose, n_res=2))
    assert refused(h, "pose_rmsd", dict(X=x, res=np.array([0], i32), rmsd=Out(f32, B * B)), **dict(pose, n_res=2))      # subset too short
    assert refused(h, "pose_mask", dict(X=x, mask=Out(u32, B * W - 1)), **pose)
    assert refused(h, "pose_mask", dict(X=x, mask=Out(u32, B * W)), **dict(pose, radius=0.0))

    mask = eh.pack32(np.eye(B, dtype=bool))
    order, pos = np.array([2, 0, 1, 4, 3], i32), np.array([1, 2, 0, 4, 3], i32)
    lead = lambda **k: dict(dict(mask=mask, order=order, cluster_of=Out(i32, B), center=Out(i32, 3), size=Out(i32, 3), n_out=Out(i32, 1)), **k)
    assert refused(h, "leader", lead(order=np.array([2, 0, 1, 4, 4], i32)), B=B, max_clusters=3)             # no permutation
    assert refused(h, "leader", lead(order=np.array([2, 0, 1, 4, 5], i32)), B=B, max_clusters=3)
    assert refused(h, "leader", lead(order=order[:-1]), B=B, max_clusters=3)
    assert refused(h, "leader", lead(), B=B, max_clusters=0)
    assert refused(h, "leader", lead(), B=B, max_clusters=4)                                                 # center / size: 3 < min(4, B)
    assert refused(h, "leader", lead(mask=mask[:-1]), B=B, max_clusters=3)
    assert refused(h, "leader", lead(cluster_of=Out(i32, init=np.zeros(B))), B=B, max_clusters=3)            # in / out where an output is due
    assert refused(h, "count", dict(mask=mask, counts=Out(i32, B - 1), U=Out(u32, W), cluster_of=Out(i32, B), state=Out(i32, 3)), B=B)
    assert refused(h, "count", dict(mask=mask, counts=Out(i32, B), U=Out(u32, W), cluster_of=Out(i32, B), state=Out(i32, 2)), B=B)

    st = eh.fresh_state(B, 3)
    st.update(eh.restate_count(np.eye(B, dtype=bool)))
    step = lambda **k: dict(dict(mask=mask, pos=pos, order=order, **{n: Out(u32 if n == "U" else i32, init=st[n]) for n in eh.STEP_KEYS}), **k)
    assert refused(h, "step", step(pos=np.array([1, 2, 0, 3, 4], i32)), B=B, max_clusters=3)                 # pos is not the inverse of order
    assert refused(h, "step", step(mlist=Out(i32, init=np.zeros(B - 1))), B=B, max_clusters=3)
    assert refused(h, "step", step(state=Out(i32, init=[3, 0, 0])), B=B, max_clusters=3)                     # the next cluster has no slot
    assert refused(h, "step", step(U=Out(u32, init=[0x3f])), B=B, max_clusters=3)                            # U names pose 5 of 5
    assert refused(h, "step", step(counts=Out(i32, B)), B=B, max_clusters=3)                                 # in / out state given as output
    full = dict(mask=mask, pos=pos, order=order, counts=Out(i32, B), U=Out(u32, W), cluster_of=Out(i32, B), center=Out(i32, 3),
                size=Out(i32, 3), mlist=Out(i32, B), state=Out(i32, 3))
    assert refused(h, "size_full", dict(full, mlist=Out(i32, B - 1)), B=B, max_clusters=3)
    assert refused(h, "size_full", dict(full, size=Out(i32, 2)), B=B, max_clusters=3)
    assert refused(h, "size_full", full, B=B, max_clusters=-1)

    n, R, Lg = 2, 3, 70
    Wl = eh.words64(Lg)
    rec, lig, mem = np.zeros((R, 9), f32), np.zeros((n, Lg, 9), f32), np.ones(n, np.uint8)
    bits = np.zeros((n, Wl, R), u64)
    cons = dict(n=n, R=R, L=Lg)
    assert refused(h, "contact_bits", dict(rec=rec, lig=lig, bits=Out(u64, n * Wl * R - 1)), cutoff=5.5, **cons)
    assert refused(h, "contact_bits", dict(rec=rec, lig=lig[:1], bits=Out(u64, n * Wl * R)), cutoff=5.5, **cons)
    assert refused(h, "contact_bits", dict(rec=rec, lig=lig, bits=bits), cutoff=5.5, **cons)
    cnt = lambda **k: dict(dict(bits=bits, member=mem, count=Out(i32, init=np.zeros(R * Lg)), rec_count=Out(i32, init=np.zeros(R)),
                                lig_count=Out(i32, init=np.zeros(Lg))), **k)
    assert refused(h, "contact_count", cnt(count=np.zeros(R * Lg, i32)), **cons)                             # not flagged as in / out
    assert refused(h, "contact_count", cnt(lig_count=Out(i32, init=np.zeros(Lg - 1))), **cons)
    assert refused(h, "contact_count", cnt(member=mem[:1]), **cons)
    high = bits.copy()
    high[1, 1, 2] = u64(1) << u64(Lg % 64)      # a contact with ligand residue L: k_contact_score would follow it out of count
    sc = lambda **k: dict(dict(bits=bits, count=np.zeros(R * Lg, i32), n_contacts=Out(i32, n), score_sum=Out(np.int64, n)), **k)
    assert refused(h, "contact_score", sc(bits=high), **cons)
    assert refused(h, "contact_score", sc(score_sum=Out(np.int64, n - 1)), **cons)
    assert refused(h, "contact_score", sc(count=np.zeros(R * Lg - 1, i32)), **cons)
    assert refused(h, "contact_score", sc(), **dict(cons, n=0))
    fullc = dict(cnt(bits=Out(u64, n * Wl * R)), rec=rec, lig=lig, n_contacts=Out(i32, n), score_sum=Out(np.int64, n))
    assert refused(h, "consensus_full", dict(fullc, n_contacts=Out(i32, 1)), cutoff=5.5, **cons)
    assert refused(h, "consensus_full", fullc, cutoff=0.0, **cons)


# ---- k_pose_dist --------------------------------------------------------------------------------------------------------------------------
def exact_fma(d, acc):
    d, acc = fractions.Fraction(float(d)), fractions.Fraction(float(acc))
    return eh.round32(d * d + acc)


def test_fma32_is_one_rounding():
    """fma32 against the all-fractions evaluation: random operands, and the planted case where float64's own rounding lands on the
    half-way point of two float32 (a plain float64 -> float32 conversion then rounds the wrong way)."""
    rng = np.random.default_rng(3)
    d = (rng.standard_normal(4000) * 10.0 ** rng.integers(-4, 3, 4000)).astype(f32)
    acc = np.abs(rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 5, 4000)).astype(f32)
    got = eh.fma32(d, acc)
    assert all(got[i] == exact_fma(d[i], acc[i]) for i in range(4000))
    # d = 2^11 * 4097: d * d = 2^46 + 2^35 + 2^22 sits half way between two float32, and acc = 2^-10 is lost in float64
    d = np.array([2.0 ** 11 * 4097], f32)
    acc = np.array([2.0 ** -10], f32)
    naive = (acc.astype(np.float64) + d.astype(np.float64) ** 2).astype(f32)
    assert naive[0] == f32(2.0 ** 46 + 2.0 ** 35) and eh.fma32(d, acc)[0] == f32(2.0 ** 46 + 2.0 ** 35 + 2.0 ** 23) == exact_fma(d[0], acc[0])


def test_pose_cases_cover_the_shapes():
    cs = eh.pose_cases()
    assert {c.B for c in cs} == {1, 31, 32, 33, 63, 64, 65, 96, 97, 129, 200}
    assert {c.D for c in cs} == {9, 27, 36, 63, 72, 288}
    kinds = {s[3] for s in eh.POSE_SHAPES}
    assert kinds == {"none", "sorted", "unsorted", "perm"}
    for c, s in zip(cs, eh.POSE_SHAPES):
        if s[3] == "sorted":
            assert (np.diff(c.res) > 0).all() and c.L * 9 > c.D
        if s[3] == "unsorted":
            assert not (np.diff(c.res) > 0).all() and c.L * 9 > c.D
        if s[3] == "perm":
            assert sorted(c.res) == list(range(c.L)) and not (np.diff(c.res) > 0).all()
    assert {c.kind for c in cs} == {"rigid", "noise", "far", "origin", "lattice", "planted"}
    assert all(np.abs(c.x).min() > 8000 for c in cs if c.kind == "far")
    for c in cs:
        if c.kind == "origin":      # a zero pose is within the radius of every pose, and some B is no multiple of the tile
            z = np.sqrt((eh.subset_coords(c.x, c.res).astype(np.float64) ** 2).sum(1) / (3 * c.n_res))
            assert (z < c.radius).all()
        if c.kind in ("lattice", "planted"):
            assert (c.x * 4 == np.round(c.x * 4)).all()
    assert any(c.kind == "origin" and c.B % 32 for c in cs)


def test_lattice_sums_are_exact_and_the_radius_lies_between_two():
    for c in eh.pose_cases():
        if c.kind != "lattice":
            continue
        xs = eh.subset_coords(c.x, c.res).astype(np.float64)
        S = ((xs[:, None] - xs[None]) ** 2).sum(-1)
        assert (np.abs(xs[:, None] - xs[None]) <= 4.0).all() and S.max() * 16 < 2 ** 24
        t = c.radius ** 2 * 3 * c.n_res      # the radius as a sum
        below, above = S[S <= t].max(), S[S > t].min()
        assert above - below >= 1.0 / 16 and below + 1.0 / 64 < t < above - 1.0 / 64, (c, below, t, above)
        assert eh.border_pairs(c)[1] == 0


def test_planted_pair_sits_on_the_radius():
    c = [c for c in eh.pose_cases() if c.kind == "planted"][0]
    rm, words = c.restated
    assert rm[0, c.B - 1] == f32(c.radius) and rm[0, c.B - 1] > 0
    nb = eh.unpack32(words, c.B)
    assert nb[0, c.B - 1] and nb[c.B - 1, 0], "<= at the radius"
    _, lt = eh.restate_pose(c.x, c.res, c.radius, "lt_radius")
    assert not eh.unpack32(lt, c.B)[0, c.B - 1]


def test_pose_restatement_against_the_definition_and_the_border_caps():
    """The restatement passes every comparison the GPU tests use on the GPU tests' inputs; the largest |restated - float64| / gate is
    printed per D; border pairs: at most 0.5 % of the generic pairs, none of the lattice pairs."""
    worst, pairs, border = {}, {}, {}
    for c in eh.pose_cases():
        rm, words = c.restated
        worst[c.D] = max(worst.get(c.D, 0.0), eh.check_rmsd(rm, c))
        n, b = eh.check_mask(words, c)
        g = "lattice" if c.kind == "lattice" else "generic"
        pairs[g], border[g] = pairs.get(g, 0) + n, border.get(g, 0) + b
    print("restatement, |error| / gate per D:", {k: f"{v:.3g}" for k, v in sorted(worst.items())})
    print("pairs", pairs, "border pairs", border)
    assert border["lattice"] == 0 and pairs["lattice"] > 5000
    assert pairs["generic"] > 50000 and border["generic"] <= eh.BORDER_CAP * pairs["generic"]


def test_poisoned_pose_in_the_restatement():
    """A NaN pose and a +inf pose: the whole row and column clear, diagonal included; every other bit as without them; the same poison
    outside the subset changes nothing."""
    seen = 0
    for c in eh.pose_cases():
        p = eh.poisoned(c, "both", True)
        if p is None:
            continue
        seen += 1
        assert (~p.finite).sum() == 2
        rm, words = p.restated
        eh.check_rmsd(rm, p)
        eh.check_mask(words, p)
        keep = np.outer(p.finite, p.finite)
        assert np.array_equal(rm[keep].view(u32), c.restated[0][keep].view(u32))
        assert np.array_equal(eh.unpack32(words, c.B)[keep], eh.unpack32(c.restated[1], c.B)[keep])
        assert np.isnan(rm[c.B // 2]).all() and not np.isfinite(rm[c.B - 1]).any()
        q = eh.poisoned(c, "both", False)
        if q is not None:
            assert q.finite.all() and q.restated[0].tobytes() == c.restated[0].tobytes() and np.array_equal(q.restated[1], c.restated[1])
    assert seen >= 10


@pytest.mark.parametrize("mutant", eh.POSE_MUTANTS)
def test_pose_mutants_are_rejected(mutant):
    """By the comparisons with float64 and the structure alone (restatement = False) - but for < at the radius, which only the planted
    pair's bit shows."""
    hits = []
    for c in eh.pose_cases():
        rm, words = eh.restate_pose(c.x, c.res, c.radius, mutant)
        own = mutant == "lt_radius"
        if eh.rejected(lambda: eh.check_rmsd(rm, c, restatement=own)) or eh.rejected(lambda: eh.check_mask(words, c, restatement=own)):
            hits.append(c.name)
    print(mutant, "rejected on", hits)
    must = {"gram": [c.name for c in eh.pose_cases() if c.kind == "far"],
            "last_chunk_dropped": [c.name for c in eh.pose_cases() if c.D % eh.KC and c.B > 1],
            "subset_ignored": [c.name for c, s in zip(eh.pose_cases(), eh.POSE_SHAPES) if s[3] in ("sorted", "unsorted") and c.kind != "origin"],
            "lt_radius": [c.name for c in eh.pose_cases() if c.kind == "planted"],
            "mean_over_residues": [c.name for c in eh.pose_cases() if c.B > 1],
            "transpose_not_written": [c.name for c in eh.pose_cases() if c.B > 64],
            "padding_not_skipped": [c.name for c in eh.pose_cases() if c.kind == "origin" and c.B % 32]}[mutant]
    assert must and all(name in hits for name in must), (mutant, [n for n in must if n not in hits])


# ---- the clustering kernels -----------------------------------------------------------------------------------------------------------------
def test_graph_cases_cover_the_shapes():
    cs = eh.graph_cases()
    assert {c.B for c in cs} == set(eh.GRAPH_B)
    for kind in eh.GRAPH_KINDS:
        assert any(kind in c.name and "nonfinite" in c.name for c in cs) and any(kind in c.name and "nonfinite" not in c.name for c in cs)
    for kk in eh.KEY_KINDS:
        assert any(f"key {kk}" in c.name for c in cs)
    assert all(c.adj.diagonal().all() != ("nonfinite" in c.name) for c in cs)
    assert any(c.B > 1 and len(c.limits()) == 3 for c in cs)
    p = eh.planted_scan_case()
    first = p.order[:2100]
    assert p.adj[np.ix_(first, first)].all() and not p.adj[first][:, p.order[2100:]].any(), "ranks 1 .. 2099 are swallowed by cluster 0"
    last = p.order[-1]
    assert p.adj[last].sum() == 1 and p.natural == {"energy": 4, "size": 4}
    # a path: the two rules differ
    from dfmdock_amd.cluster import cluster_adjacency
    path = [c for c in cs if "path" in c.name and c.B >= 31 and "nonfinite" not in c.name][0]
    assert cluster_adjacency(path.adj, path.key, "energy")["n_clusters"] != cluster_adjacency(path.adj, path.key, "size")["n_clusters"] or \
        not np.array_equal(cluster_adjacency(path.adj, path.key, "energy")["center"], cluster_adjacency(path.adj, path.key, "size")["center"])


def steps_of(case, max_clusters, extra=2, most=12, mutant=None):
    """The states before and after each of the first steps of rule `size`, and `extra` steps after the run has ended."""
    cap = min(max_clusters, case.B)
    st = eh.fresh_state(case.B, cap)
    st.update(eh.restate_count(case.adj, mutant))
    out = []
    for _ in range(min(cap, most)):
        nxt = eh.restate_step(case.adj, case.pos, case.order, st, mutant)
        out.append((st, nxt))
        st = nxt
    return out


def small(cs, most=1100):
    return [c for c in cs if c.B <= most]


def test_cluster_restatements_equal_the_definition():
    for c in eh.graph_cases():
        eh.check_count(eh.restate_count(c.adj), c)
        for maxc in c.limits():
            eh.check_leader(eh.restate_leader(c.adj, c.order, maxc), c, maxc)
            if c.B <= 1100 or maxc < c.B:
                eh.check_size_full(eh.restate_size_full(c.adj, c.pos, c.order, maxc), c, maxc)
    for c in small(eh.graph_cases(), 70):
        for before, after in steps_of(c, c.B):
            eh.check_step(after, before, c, c.B)
        done = eh.restate_size_full(c.adj, c.pos, c.order, c.B)
        if done["state"][1]:
            eh.check_step(eh.restate_step(c.adj, c.pos, c.order, done), done, c, c.B)


def test_non_finite_poses_open_no_cluster():
    from dfmdock_amd.cluster import cluster_adjacency
    for c in eh.graph_cases():
        if "nonfinite" not in c.name:
            continue
        bad = ~c.adj.diagonal()
        for rule in ("energy", "size"):
            r = cluster_adjacency(c.adj, c.key, rule)
            assert (r["cluster_of"][bad] == -1).all() and (r["size"] >= 1).all() and not bad[r["center"]].any()
            assert r["size"].sum() == (~bad).sum()


@pytest.mark.parametrize("mutant", eh.CLUSTER_MUTANTS)
def test_cluster_mutants_are_rejected(mutant):
    hits = []
    for c in eh.graph_cases():
        for maxc in c.limits():
            bad = eh.rejected(lambda: eh.check_leader(eh.restate_leader(c.adj, c.order, maxc, mutant), c, maxc))
            if c.B <= 70 or maxc <= 200:      # (the long runs of the large cases: the restatement itself is checked on them above)
                bad = bad or eh.rejected(lambda: eh.check_size_full(eh.restate_size_full(c.adj, c.pos, c.order, maxc, mutant), c, maxc))
            if maxc == c.B and not bad:
                bad = eh.rejected(lambda: eh.check_count(eh.restate_count(c.adj, mutant), c))
            if maxc == c.B and not bad and c.B <= 70:
                for before, _ in steps_of(c, c.B):
                    bad = bad or eh.rejected(lambda: eh.check_step(eh.restate_step(c.adj, c.pos, c.order, before, mutant), before, c, c.B))
            if bad:
                hits.append(f"{c.name} / {maxc}")
    print(mutant, "rejected on", len(hits), "of the launches, e.g.", hits[:4])
    assert hits, mutant
    if mutant == "leader_one_stride":
        assert any(h.startswith("B2500 planted scan") for h in hits)
    if mutant == "nonfinite_opens":
        assert all("nonfinite" in h for h in hits) and len({h.split(" / ")[0] for h in hits}) == sum("nonfinite" in c.name for c in eh.graph_cases())


# ---- the consensus kernels ----------------------------------------------------------------------------------------------------------------
def test_contact_cases_cover_the_shapes():
    from dfmdock_amd.consensus import contacts
    cs = eh.contact_cases()
    assert {c.R for c in cs} == {1, 63, 64, 65, 130} and {c.L for c in cs} == {1, 63, 64, 65, 129} and {c.n for c in cs} == {1, 3}
    total = {}
    for c in cs:
        cc = contacts(c.rec, c.lig, c.cutoff)
        total[c.kind] = total.get(c.kind, 0) + int(cc.sum())
        for p, i, j, want in c.planted:
            assert cc[p, i, j] == want, (c, p, i, j)
        if c.kind == "lattice":
            assert cc.sum() == sum(1 for pl in c.planted if pl[3]), "nothing but the planted pair inside the cutoff"
            assert (False in [pl[3] for pl in c.planted]) and (c.n * c.L == 1 or True in [pl[3] for pl in c.planted])
    assert total["generic"] > 200 and total["stretched"] > 20 and total["origin"] > 200
    far = 0
    for c in cs:
        if c.kind == "stretched":
            cc = contacts(c.rec, c.lig, c.cutoff)
            ca = np.linalg.norm(c.rec[None, :, None, 3:6].astype(np.float64) - c.lig[:, None, :, 3:6], axis=-1)
            far += int((cc & (ca > 60.0)).sum())
    assert far > 10, "contacts between residues whose CAs are more than 60 A apart"
    assert any(c.kind == "origin" and c.L % 64 for c in cs)


def test_device_bits_is_the_transposed_host_layout():
    from dfmdock_amd.consensus import pack_bits
    rng = np.random.default_rng(5)
    for n, R, L in ((1, 1, 1), (2, 5, 64), (3, 66, 130)):
        c = rng.random((n, R, L)) < 0.4
        d = eh.device_bits(c)
        assert d.shape == (n, eh.words64(L), R) and np.array_equal(d.transpose(0, 2, 1), pack_bits(c))
        back, high = eh.host_bits(d, L)
        assert high == 0 and np.array_equal(back, c)


def test_consensus_restatements_equal_the_definition():
    for c in eh.contact_cases():
        eh.check_contact_bits(eh.restate_contact_bits(c.rec, c.lig, c.cutoff), c.rec, c.lig, c.cutoff)
        for how in ("nan", "inf"):
            for where in ("lig", "rec"):
                p = eh.contact_poisoned(c, how, where)
                bits = eh.restate_contact_bits(p.rec, p.lig, p.cutoff)
                eh.check_contact_bits(bits, p.rec, p.lig, p.cutoff)
                check_poison_kept_to_itself(bits, eh.restate_contact_bits(c.rec, c.lig, c.cutoff), c, where)
    for name, cc, mem, pre in eh.count_cases():
        bits, L = eh.device_bits(cc), cc.shape[2]
        got = eh.restate_contact_count(bits, mem, L, **pre)
        eh.check_contact_count(got, bits, mem, L, pre)
        eh.check_contact_score(eh.restate_contact_score(bits, got["count"], L), bits, got["count"], L)
    cc, count = eh.big_score_case()
    got = eh.restate_contact_score(eh.device_bits(cc), count, 192)
    assert (got["score_sum"] == 2415919104).all() and 2415919104 > 2 ** 31
    eh.check_contact_score(got, eh.device_bits(cc), count, 192)


def check_poison_kept_to_itself(bits, clean, case, where):
    """The poisoned ligand residue's column (of its pose) or the receptor residue's row has no contact; everything else keeps its bits."""
    got, _ = eh.host_bits(bits, case.L)
    ref, _ = eh.host_bits(clean, case.L)
    hit = np.zeros_like(ref)
    if where == "lig":
        hit[case.n - 1, :, case.L // 2] = True
    else:
        hit[:, case.R // 2, :] = True
    assert not got[hit].any() and np.array_equal(got[~hit], ref[~hit])


@pytest.mark.parametrize("mutant", eh.CONSENSUS_MUTANTS)
def test_consensus_mutants_are_rejected(mutant):
    hits = []
    if mutant in ("le_at_cutoff", "reject_without_reach", "reach_from_n_only", "fp32_distance", "high_bits_leak", "row_tail_lost"):
        for c in eh.contact_cases():
            if eh.rejected(lambda: eh.check_contact_bits(eh.restate_contact_bits(c.rec, c.lig, c.cutoff, mutant), c.rec, c.lig, c.cutoff)):
                hits.append(c.name)
        kinds = {h.split()[-1] for h in hits}
        want = {"le_at_cutoff": "lattice", "reject_without_reach": "stretched", "reach_from_n_only": "stretched", "fp32_distance": "lattice",
                "high_bits_leak": "origin", "row_tail_lost": "generic"}[mutant]
        assert want in kinds, (mutant, hits)
    else:
        for name, cc, mem, pre in eh.count_cases():
            bits, L = eh.device_bits(cc), cc.shape[2]
            got = eh.restate_contact_count(bits, mem, L, mutant=mutant, **pre)
            bad = eh.rejected(lambda: eh.check_contact_count(got, bits, mem, L, pre))
            count = eh.restate_contact_count(bits, mem, L, **pre)["count"]
            bad = bad or eh.rejected(lambda: eh.check_contact_score(eh.restate_contact_score(bits, count, L, mem, mutant), bits, count, L))
            if bad:
                hits.append(name)
        cc, count = eh.big_score_case()
        if eh.rejected(lambda: eh.check_contact_score(eh.restate_contact_score(eh.device_bits(cc), count, 192, None, mutant), eh.device_bits(cc), count, 192)):
            hits.append("big score")
        if mutant == "score_sum_32bit":
            assert hits == ["big score"]
    print(mutant, "rejected on", hits)
    assert hits, mutant
