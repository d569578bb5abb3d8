"""Pose clustering on the CPU: the float64 definition in dfmdock_amd/cluster.py against a brute-force restatement of the two rules on small
hand-built sets (chains, exact ties in key and count, NaN keys, the max_clusters cut-off, residue subsets), the backbone rebuild, the
new command-line options, the unchanged outputs without them, and the two entry points of the C ABI."""
import math
import subprocess

import numpy as np
import pytest


def _brute(lig_pos, radius, key=None, rule="energy", max_clusters=None, residues=None):
    """The rules of include/dfmdock_amd.h: dfm_pose_cluster restated with plain Python loops."""
    x = np.asarray(lig_pos, np.float64).reshape(len(lig_pos), -1, 3, 3)
    if residues is not None:
        x = x[:, list(residues)]
    x = x.reshape(len(x), -1, 3)
    B = len(x)
    nb = [[math.sqrt(sum(float(((x[a][t] - x[b][t]) ** 2).sum()) for t in range(x.shape[1])) / x.shape[1]) <= radius
           for b in range(B)] for a in range(B)]

    def better(i, j):      # True when pose i comes before pose j in key order
        if key is None:
            return i < j
        ki, kj = float(key[i]), float(key[j])
        if math.isnan(ki) != math.isnan(kj):
            return math.isnan(kj)
        if not math.isnan(ki) and ki != kj:
            return ki < kj
        return i < j

    maxc = B if max_clusters is None else max_clusters
    free, of, center, size = {i for i in range(B) if nb[i][i]}, [-1] * B, [], []      # (a pose with a NaN is not its own neighbour)
    if rule == "energy":
        order = list(range(B))
        for i in range(B):      # selection sort with `better`
            for j in range(i + 1, B):
                if better(order[j], order[i]):
                    order[i], order[j] = order[j], order[i]
        for p in order:
            if len(center) == maxc:
                break
            if p in free:
                m = [j for j in sorted(free) if nb[p][j]]
                for j in m:
                    of[j] = len(center)
                free -= set(m)
                center.append(p)
                size.append(len(m))
    else:
        while free and len(center) < maxc:
            best = None
            for i in sorted(free):
                c = sum(nb[i][j] for j in free)
                if best is None or c > best[0] or (c == best[0] and better(i, best[1])):
                    best = (c, i)
            p = best[1]
            m = [j for j in sorted(free) if nb[p][j]]
            for j in m:
                of[j] = len(center)
            free -= set(m)
            center.append(p)
            size.append(len(m))
    return {"n_clusters": len(center), "center": center, "size": size, "cluster_of": of}


def _same(got, want):
    assert got["n_clusters"] == want["n_clusters"]
    assert list(got["center"]) == list(want["center"])
    assert list(got["size"]) == list(want["size"])
    assert list(got["cluster_of"]) == list(want["cluster_of"])


def _chain(n, step, L=3):
    """n copies of one small ligand translated step A apart along x: pose i neighbours i - 1 and i + 1 at radius step."""
    rng = np.random.default_rng(0)
    base = rng.normal(0, 5, (L, 3, 3))
    return np.stack([base + np.array([step * i, 0, 0]) for i in range(n)]).astype(np.float32)


def test_pose_rmsd_is_the_direct_definition():
    from dfmdock_amd.cluster import pose_rmsd
    rng = np.random.default_rng(1)
    x = rng.normal(0, 10, (7, 5, 3, 3)).astype(np.float32)
    r = pose_rmsd(x)
    for a in range(7):
        for b in range(7):
            d = x[a].astype(np.float64).reshape(-1, 3) - x[b].astype(np.float64).reshape(-1, 3)
            assert r[a, b] == pytest.approx(np.sqrt((d ** 2).sum(-1).mean()), rel=1e-12, abs=1e-12)
    assert (np.diag(r) == 0).all() and (r == r.T).all()
    sub = pose_rmsd(x, residues=[4, 0])
    d = x[0, [4, 0]].astype(np.float64) - x[3, [4, 0]].astype(np.float64)
    assert sub[0, 3] == pytest.approx(np.sqrt((d ** 2).sum(-1).mean()), rel=1e-12)
    # a rigid translation by t moves every atom by |t|
    y = x.copy()
    y[1] = x[0] + np.array([3.0, 4.0, 0.0], np.float32)
    assert pose_rmsd(y)[0, 1] == pytest.approx(5.0, rel=1e-6)


@pytest.mark.parametrize("rule", ["energy", "size"])
def test_chain_of_poses(rule):
    from dfmdock_amd.cluster import cluster_poses
    x = _chain(7, 2.0)
    got = cluster_poses(x, 2.5, rule=rule)
    _same(got, _brute(x, 2.5, rule=rule))
    if rule == "energy":      # index order: 0 takes 1, 2 takes 3, ...
        assert list(got["center"]) == [0, 2, 4, 6] and list(got["size"]) == [2, 2, 2, 1]
    else:                     # every inner pose has 3 neighbours: 1 wins the tie by index, then 4 (3 left: 3, 4, 5 free), ...
        assert list(got["center"]) == [1, 4, 6] and list(got["size"]) == [3, 3, 1]


def test_key_ties_and_nan_go_last():
    from dfmdock_amd.cluster import cluster_poses, rank_order
    key = np.array([1.0, np.nan, 0.5, 0.5, np.nan, -2.0], np.float32)
    assert list(rank_order(key, 6)) == [5, 2, 3, 0, 1, 4]
    x = _chain(6, 10.0)      # nobody neighbours anybody: every pose is its own cluster, in key order
    got = cluster_poses(x, 1.0, key=key)
    assert list(got["center"]) == [5, 2, 3, 0, 1, 4]
    _same(got, _brute(x, 1.0, key=key))
    got = cluster_poses(x, 1.0, key=key, rule="size")      # all counts tie at 1: the key decides
    assert list(got["center"]) == [5, 2, 3, 0, 1, 4]


def test_count_ties_go_to_the_better_key_then_the_lower_index():
    from dfmdock_amd.cluster import cluster_poses
    x = _chain(6, 2.0)[[0, 1, 2, 3, 4, 5]]
    x[3:] += np.float32(100.0)      # two chains of three: poses 1 and 4 have three neighbours each
    assert list(cluster_poses(x, 2.5, rule="size")["center"]) == [1, 4]
    key = np.array([0, 5, 0, 0, 1, 0], np.float32)
    assert list(cluster_poses(x, 2.5, key=key, rule="size")["center"]) == [4, 1]
    _same(cluster_poses(x, 2.5, key=key, rule="size"), _brute(x, 2.5, key=key, rule="size"))


@pytest.mark.parametrize("rule", ["energy", "size"])
def test_max_clusters_leaves_the_rest_unassigned(rule):
    from dfmdock_amd.cluster import cluster_poses
    x = _chain(9, 2.0)
    got = cluster_poses(x, 2.5, rule=rule, max_clusters=2)
    assert got["n_clusters"] == 2 and (got["cluster_of"] == -1).sum() == 9 - got["size"].sum()
    _same(got, _brute(x, 2.5, rule=rule, max_clusters=2))


@pytest.mark.filterwarnings("ignore:invalid value")
@pytest.mark.parametrize("max_clusters", [None, 2, 6])
@pytest.mark.parametrize("rule", ["energy", "size"])
def test_a_non_finite_pose_opens_no_cluster(rule, max_clusters):
    """A pose with a non-finite coordinate is no pose's neighbour, itself included: it never opens a cluster, keeps cluster_of = -1,
    every cluster formed has a member, and the run ends when no pose that is its own neighbour is left - keyed first, keyed last, and
    when every pose is such a pose."""
    from dfmdock_amd.cluster import cluster_poses
    x = _chain(6, 2.0)
    x[3:] += np.float32(100.0)      # two chains of three
    kw = {} if max_clusters is None else {"max_clusters": max_clusters}
    for bad, value in ((0, np.nan), (5, np.nan), (2, np.inf)):
        y = x.copy()
        y[bad, 1, 2, 0] = value
        for key in (None, np.where(np.arange(6) == bad, -9.0, np.arange(6)).astype(np.float32),      # keyed first
                    np.where(np.arange(6) == bad, 99.0, np.arange(6)).astype(np.float32)):           # keyed last
            got = cluster_poses(y, 2.5, key=key, rule=rule, **kw)
            _same(got, _brute(y, 2.5, key=key, rule=rule, **kw))
            assert got["cluster_of"][bad] == -1 and bad not in list(got["center"]) and (got["size"] >= 1).all()
            if max_clusters != 2:
                assert got["size"].sum() == 5 and (np.delete(got["cluster_of"], bad) >= 0).all()
        sub = cluster_poses(y, 2.5, rule=rule, residues=[0, 2], **kw)      # the non-finite coordinate is in residue 1: not compared
        _same(sub, cluster_poses(x, 2.5, rule=rule, residues=[0, 2], **kw))
    allbad = x.copy()
    allbad[:, 0, 0, 0] = np.nan
    got = cluster_poses(allbad, 2.5, key=np.arange(6, dtype=np.float32), rule=rule, **kw)
    assert got["n_clusters"] == 0 and got["center"].size == 0 and got["size"].size == 0 and (got["cluster_of"] == -1).all()
    # the case of the record: 6 poses, one with a NaN, one cluster of the five others
    far = _chain(6, 1.0)
    far[3, 0, 0, 0] = np.nan
    got = cluster_poses(far, 50.0, rule=rule, **kw)
    assert got["n_clusters"] == 1 and list(got["center"]) == [0] and list(got["size"]) == [5] and list(got["cluster_of"]) == [0, 0, 0, -1, 0, 0]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("rule", ["energy", "size"])
def test_random_sets_against_the_brute_force(seed, rule):
    from dfmdock_amd.cluster import cluster_poses
    rng = np.random.default_rng(seed)
    B, L = int(rng.integers(1, 40)), int(rng.integers(1, 6))
    centres = rng.normal(0, 6, (3, 1, 1, 3))
    x = (rng.normal(0, 4, (L, 3, 3))[None] + centres[rng.integers(0, 3, B)] + rng.normal(0, 1.5, (B, 1, 1, 3))).astype(np.float32)
    key = rng.normal(size=B).astype(np.float32)
    key[rng.random(B) < 0.2] = np.nan
    key[rng.random(B) < 0.2] = 0.25      # exact ties
    residues = rng.permutation(L)[: max(1, L // 2)] if seed % 2 else None
    for kw in ({}, {"key": key}, {"max_clusters": 3}, {"key": key, "residues": residues}):
        _same(cluster_poses(x, 3.0, rule=rule, **kw), _brute(x, 3.0, rule=rule, **kw))


def test_residue_subset_changes_the_neighbours():
    from dfmdock_amd.cluster import cluster_poses
    x = _chain(2, 0.0, L=4)
    x[1, 3] += np.float32(40.0)      # residue 3 of pose 1 far off: neighbours on residues 0..2 only
    assert cluster_poses(x, 1.0)["n_clusters"] == 2
    assert cluster_poses(x, 1.0, residues=[0, 1, 2])["n_clusters"] == 1


@pytest.mark.parametrize("bad", [dict(residues=[0, 0]), dict(residues=[5]), dict(residues=[-1]), dict(residues=[])])
def test_bad_residues(bad):
    from dfmdock_amd.cluster import cluster_poses
    with pytest.raises(ValueError):
        cluster_poses(_chain(3, 1.0), 1.0, **bad)


@pytest.mark.parametrize("radius", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_radius(radius):
    from dfmdock_amd.cluster import cluster_poses
    with pytest.raises(ValueError):
        cluster_poses(_chain(3, 1.0), radius)


def test_bad_rule_and_max_clusters():
    from dfmdock_amd.cluster import cluster_poses
    with pytest.raises(ValueError):
        cluster_poses(_chain(3, 1.0), 1.0, rule="kmeans")
    with pytest.raises(ValueError):
        cluster_poses(_chain(3, 1.0), 1.0, max_clusters=0)


@pytest.mark.parametrize("family", [0, 1])
def test_rebuild_backbone_is_the_composed_sampler_step(family):
    """Two steps of modify_coords (each about the current centroid) equal one rebuild from the composed (rot_update, tr_update)."""
    from dfmdock_amd.cluster import rebuild_backbone
    from dfmdock_amd.pdbio import axis_angle_to_matrix
    from dfmdock_amd.restraints import rot_compose
    rng = np.random.default_rng(family)
    x0 = rng.normal(0, 8, (12, 3, 3))
    cen = (lambda x: x.reshape(-1, 3).mean(0)) if family == 1 else (lambda x: x[:, 1].mean(0))
    x, rot, tr = x0.copy(), np.zeros(3), np.zeros(3)
    for _ in range(2):
        r, t = rng.normal(0, 0.7, 3), rng.normal(0, 3, 3)
        c = cen(x)
        x = (x - c) @ axis_angle_to_matrix(r).T + c + t
        rot, tr = rot_compose(rot, r), tr + t
    got = rebuild_backbone(x0.astype(np.float32), rot[None], tr[None], family)
    assert got.dtype == np.float32 and got.shape == (1, 12, 3, 3)
    np.testing.assert_allclose(got[0], x, atol=1e-4)


def test_satisfied_key_first_pose_is_the_restraint_ranking_choice():
    from dfmdock_amd.cluster import rank_order, satisfied_key
    from dfmdock_amd.restraints import rank_key
    rng = np.random.default_rng(5)
    for _ in range(20):
        e = rng.integers(-3, 3, 15).astype(np.float32)      # many exact energy ties
        s = rng.integers(0, 3, 15)
        assert rank_order(satisfied_key(e, s), 15)[0] == rank_key(e, s)


def test_cli_parses_the_clustering_options():
    from dfmdock_amd import cli
    base = ["dock", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz"]
    a = cli.build_parser().parse_args(base)
    assert a.top_k is None and a.cluster_radius == 4.0 and a.cluster_rule == "energy"
    a = cli.build_parser().parse_args(base + ["--top-k", "5", "--cluster-radius", "3", "--cluster-rule", "size"])
    assert (a.top_k, a.cluster_radius, a.cluster_rule) == (5, 3.0, "size")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--top-k", "5", "--cluster-rule", "kmeans"])
    s = cli.build_parser().parse_args(["sweep", "--db5", "d", "--ckpt", "m.ckpt"])
    assert s.cluster_radius is None and s.top_k == 10 and s.cluster_rule == "energy"
    s = cli.build_parser().parse_args(["sweep", "--db5", "d", "--ckpt", "m.ckpt", "--cluster-radius", "4", "--top-k", "3"])
    assert s.cluster_radius == 4.0 and s.top_k == 3


_ROWS = [{"id": "A", "index": "0", "DockQ": 0.9, "energy": -1.0, "cluster": 1, "is_center": 1},
         {"id": "A", "index": "1", "DockQ": 0.1, "energy": -2.0, "cluster": 0, "is_center": 1},
         {"id": "A", "index": "2", "DockQ": 0.95, "energy": -1.5, "cluster": 0, "is_center": 0},
         {"id": "B", "index": "0", "DockQ": 0.3, "energy": -5.0, "cluster": 0, "is_center": 1},
         {"id": "B", "index": "1", "DockQ": 0.5, "energy": -4.0, "cluster": -1, "is_center": 0}]


def test_plain_table_is_unchanged_without_clustering():
    from dfmdock_amd import cli
    rows = [{k: v for k, v in r.items() if k not in ("cluster", "is_center")} for r in _ROWS]
    per, table = cli.success_table(rows)
    assert set(per["A"]) == {"n", "top1_DockQ", "top1_energy", "best_DockQ", "mean_DockQ"}
    assert set(table["acceptable"]) == {"threshold", "top1", "best_of_n"}
    assert cli.format_table(per, table) == "\n".join([
        "id          n  top1 DockQ  best DockQ  top1 energy",
        "A           3      0.1000      0.9500      -2.0000",
        "B           2      0.3000      0.5000      -5.0000",
        "success rate over 2 complexes (DockQ of the minimum-energy trajectory | best of the trajectories):",
        "  acceptable DockQ >= 0.23:  50.0 % | 100.0 %",
        "  medium     DockQ >= 0.49:   0.0 % | 100.0 %",
        "  high       DockQ >= 0.80:   0.0 % |  50.0 %"])


def test_topk_success_counts_the_first_k_cluster_centres():
    from dfmdock_amd import cli
    per, table = cli.success_table(_ROWS, top_k=2)
    assert per["A"]["top2_DockQ"] == 0.9 and per["B"]["top2_DockQ"] == 0.3      # a member (0.95) or an unclustered pose does not count
    assert table["high"]["top2"] == 0.5 and table["high"]["top1"] == 0.0 and table["high"]["best_of_n"] == 0.5
    per1, table1 = cli.success_table(_ROWS, top_k=1)
    assert per1["A"]["top1_DockQ"] == per1["A"]["top1_DockQ"] == 0.1 and table1["high"]["top1"] == 0.0
    txt = cli.format_table(per, table, top_k=2)
    assert "top2 DockQ" in txt and "first 2 cluster centres" in txt
    for name in table:
        assert table[name]["top1"] <= table[name]["top2"] <= table[name]["best_of_n"]


def test_driver_fields():
    from dfmdock_amd import driver
    assert driver.CSV_FIELDS == ["id", "index", "c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ", "energy", "num_clashes"]
    assert driver.CLUSTER_FIELDS == ["cluster", "is_center"]
    assert driver.model_path("out/output.pdb", 3) == "out/output_3.pdb"


def test_cluster_entry_points_are_exported_and_bound():
    from dfmdock_amd import _lib
    lib = _lib.lib()
    for s in ("dfm_pose_rmsd", "dfm_pose_cluster", "dfm_pose_last_timing"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and getattr(lib, s).argtypes
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert " T dfm_pose_rmsd" in out and " T dfm_pose_cluster" in out
    assert len(lib.dfm_pose_cluster.argtypes) == 14 and len(lib.dfm_pose_rmsd.argtypes) == 7


def test_invalid_arguments_are_refused_before_any_device_work():
    """Validation happens on the host: these return DFM_E_INVALID even without a GPU (a NULL model is refused first)."""
    import ctypes as C
    from dfmdock_amd import _lib
    lib = _lib.lib()
    x = np.zeros((2, 3, 9), np.float32)
    n = C.c_int32(0)
    o = np.zeros(2, np.int32)
    p = lambda a, t=_lib.I32P: a.ctypes.data_as(t)
    assert lib.dfm_pose_cluster(None, 2, 3, p(x, _lib.F32P), None, 0, None, 1.0, 0, 2, C.byref(n), p(o), p(o), p(o)) == -1
    assert lib.dfm_pose_rmsd(None, 2, 3, p(x, _lib.F32P), None, 0, p(np.zeros(4, np.float32), _lib.F32P)) == -1
