"""The contract of the pair drivers (driver.dock_pair - plain and with restraints - and driver.refine_pair) on the CPU: which entries the
result holds under which options, which trajectory is kept, what is written and when the handle is closed.  No GPU and no library: the
engine's handle is a fake that draws its trajectories from numpy, and every GPU call of the post-processing is answered by its float64
definition (cluster.cluster_poses, consensus.consensus, sterics.sterics + capri_flags, metrics.compute_metrics_batch,
restraints.evaluate).  The same calls run on the device in tests/test_gpu_{consensus,sterics,cluster,restraints,refine,metrics}.py."""
import numpy as np
import pytest

N_TRAJ, MAX_BATCH, SEED = 10, 4, 11      # batches of 4, 4 and 2
OVERLAP = 5      # this trajectory is pushed into the receptor and given the lowest energy: the one pose CAPRI's rule flags
COLUMNS = ("energy", "rot_update", "tr_update")
BASE = {"energy", "rot_update", "tr_update", "lig_aa_coords", "precision", "selfcheck"}


def make_chain(n_rows, z, chain, shift):
    """A pdbio.backbone_from_atoms dict of 4 n_rows residues on a grid in the plane `z`: N, CA, C, O, a CB towards the other chain and
    one hydrogen per residue."""
    from dfmdock_amd import pdbio
    up = 1.0 if z == 0 else -1.0
    atoms = []
    for r in range(4 * n_rows):
        ca = np.array([3.8 * (r % 4) + shift, 3.8 * (r // 4) + shift, z])
        for name, d in (("N", (-1.2, 0.5, 0)), ("CA", (0, 0, 0)), ("C", (1.2, 0.5, 0)), ("O", (1.2, 1.7, 0)), ("CB", (0, -0.8, 1.2 * up)),
                        ("HA", (0, 0.6, -0.9 * up))):
            atoms.append({"hetero": False, "name": name, "res_name": "ALA", "chain": chain, "res_id": r + 1, "ins": " ",
                          "coord": tuple(float(v) for v in ca + np.array(d)), "element": name[0]})
    return pdbio.backbone_from_atoms(atoms)


@pytest.fixture(scope="module")
def pair():
    return make_chain(3, 0.0, "A", 0.0), make_chain(2, 5.0, "B", 1.9)      # 12 + 8 residues, the planes 5 A apart


def restraint_groups():
    from dfmdock_amd.restraints import RestraintGroup
    return [RestraintGroup(((0, 0),), 6.5), RestraintGroup(((5, 2), (6, 2)), 6.5), RestraintGroup(((11, 7),), 7.0), RestraintGroup(((8, 0),), 7.5)]


class FakeModel:
    """What the drivers ask of engine.Model, answered by the float64 definitions.  `log` receives the order of events."""

    def __init__(self, family, nan=False):
        self.hp = type("Hp", (), {"family": family})()
        self.nan, self.log, self.handles = nan, [], []

    def pose_cluster(self, lig_pos, radius, key=None, rule="energy", max_clusters=None):
        from dfmdock_amd.cluster import cluster_poses
        self.log.append("cluster")
        return cluster_poses(lig_pos, radius, key, rule, max_clusters)

    def consensus(self, rec_pos, lig_pos, cutoff=5.5, members=None):
        from dfmdock_amd import consensus as CS
        self.log.append("consensus")
        return CS.consensus(rec_pos, lig_pos, cutoff, members)

    def atoms(self, rec_atoms, lig_atoms, center, clash_cutoff=3.0, contact_cutoff=5.0):
        return FakeAtoms(self, rec_atoms, lig_atoms, center, clash_cutoff, contact_cutoff)

    def native(self, rec_pos, lig_pos):
        return FakeNative(self, rec_pos, lig_pos)


class FakeAtoms:
    def __init__(self, model, *args):
        self.model, self.args = model, args
        self.clash_cutoff, self.contact_cutoff = float(np.float32(args[3])), float(np.float32(args[4]))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def sterics(self, rot, tr, per_atom=False):
        from dfmdock_amd import sterics as ST
        self.model.log.append("sterics")
        o = ST.sterics(*self.args[:3], np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3), *self.args[3:],
                       per_atom=per_atom)
        o["flags"], o["threshold"], o["ensemble_mean"], o["ensemble_std"] = ST.capri_flags(o["n_clash"])
        return o


class FakeNative:
    def __init__(self, model, rec_pos, lig_pos):
        self.model, self.native = model, (np.asarray(rec_pos), np.asarray(lig_pos))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def metrics(self, lig_pos, rec_pos=None):
        from dfmdock_amd.metrics import compute_metrics_batch
        self.model.log.append("metrics")
        return compute_metrics_batch(np.asarray(lig_pos), self.native, models_rec=rec_pos)


class FakeComplex:
    """engine.Complex without a device: `sample` and `refine` draw (energy, rot_update, tr_update) from default_rng(seed) and rebuild
    the pose from them; the first N_TRAJ draws are kept as `cols`, what the driver's columns must equal."""

    def __init__(self, model, rec_x, lig_x, rec_pos, lig_pos):
        self.model, self.rec_pos, self._lig0 = model, np.asarray(rec_pos, np.float32), np.asarray(lig_pos, np.float32)
        self.calls = {"lig_pos0": 0, "set_restraints": 0, "close": 0}
        self.groups, self.params, self.drawn, self.cols = None, None, 0, {c: [] for c in COLUMNS + ("restraint_energy", "restraints_satisfied")}
        model.handles.append(self)

    @property
    def lig_pos0(self):
        self.calls["lig_pos0"] += 1
        return self._lig0

    def set_restraints(self, groups, params=None):
        self.calls["set_restraints"] += 1
        self.groups, self.params = list(groups), params

    def close(self):
        self.calls["close"] += 1
        self.model.log.append("close")

    def _draw(self, B, seed, start, restraints):
        from dfmdock_amd.cluster import rebuild_backbone
        assert self.calls["close"] == 0, "the handle is used after close()"
        assert bool(restraints) == (self.groups is not None)
        rng = np.random.default_rng(seed)
        r = {"energy": rng.normal(size=B).astype(np.float32), "rot_update": (0.3 * rng.normal(size=(B, 3))).astype(np.float32),
             "tr_update": (1.5 * rng.normal(size=(B, 3))).astype(np.float32), "num_clashes": np.zeros(B, np.int32)}
        for k in range(B):
            g = self.drawn + k      # the trajectory's index in the driver's run
            if g == OVERLAP:
                r["energy"][k], r["rot_update"][k], r["tr_update"][k] = -9.0, 0.0, (-1.9, -1.9, -5.0)
            if self.model.nan and g == N_TRAJ - 2:
                r["energy"][k] = -100.0      # the lowest finite energy, in the last batch next to ...
            if self.model.nan and g == N_TRAJ - 1:
                r["energy"][k] = np.nan      # ... the NaN that hides that batch from the batchwise rule
        r["lig_pos"] = np.stack([rebuild_backbone(start[k], r["rot_update"][k], r["tr_update"][k], self.model.hp.family)[0] for k in range(B)])
        if self.drawn < N_TRAJ:
            for c in COLUMNS:
                self.cols[c].append(r[c])
        self.model.log.append("draw")
        self.drawn += B
        return r

    def sample(self, B=1, num_steps=40, seed=0, restraints=False, **kw):
        return self._draw(B, seed, np.repeat(self._lig0[None], B, 0), restraints)

    def refine(self, B=1, t_begin=0.1, start_pos=None, perturb=True, num_steps=40, seed=0, restraints=False, **kw):
        start = np.repeat(self._lig0[None], B, 0) if start_pos is None else np.asarray(start_pos, np.float32).reshape(B, -1, 3, 3)
        return self._draw(B, seed, start, restraints)

    def restraint_eval(self, lig_pos):
        from dfmdock_amd import restraints as RS
        center = "all_atoms" if self.model.hp.family == 1 else "ca"
        ev = [RS.evaluate(self.groups, self.rec_pos, p, self.params, center) for p in np.asarray(lig_pos)]
        out = {"energy": np.array([e["energy"] for e in ev], np.float32), "n_satisfied": np.array([e["n_satisfied"] for e in ev], np.int32)}
        if len(self.cols["restraint_energy"]) < len(self.cols["energy"]):
            self.cols["restraint_energy"].append(out["energy"])
            self.cols["restraints_satisfied"].append(out["n_satisfied"])
        return out

    def columns(self):
        return {c: np.concatenate(v, 0) for c, v in self.cols.items() if v}


DRIVERS = ("dock", "dock_satisfied", "dock_restraint_energy", "refine")
OPTIONS = {"none": {}, "consensus": {"consensus": True}, "rank_consensus": {"rank": "consensus"}, "clash_screen": {"clash_screen": True},
           "clash_filter": {"clash_filter": True}, "top_k": {"top_k": 3}, "top_k_refine_t": {"top_k": 3, "refine_t": 0.1, "refine_samples": 2},
           "native": {"native": True},
           "all": {"rank": "consensus", "clash_filter": True, "top_k": 3, "refine_t": 0.1, "refine_samples": 2, "native": True}}


def run(monkeypatch, tmp_path, pair, kind, opts, family, nan=False):
    """One driver call on the fakes.  Returns (result, handle, model, out_pdb, the writes in order)."""
    from dfmdock_amd import driver, pdbio
    rec, lig = pair
    model = FakeModel(family, nan)
    monkeypatch.setattr(driver.engine, "Complex", FakeComplex)
    monkeypatch.setattr(driver, "checked_precision", lambda gx, precision, *a, **k: (precision, None))
    real_write = pdbio.write_complex_pdb

    def write(path, *a, **k):
        model.log.append("write")
        return real_write(path, *a, **k)
    monkeypatch.setattr(pdbio, "write_complex_pdb", write)
    kw = dict(opts)
    if kw.pop("native", False):      # the input pose itself, in another frame
        kw["native"] = (np.asarray(rec["bb_coords"], np.float32) + 3.0, np.asarray(lig["bb_coords"], np.float32) + 3.0)
    if kind == "refine":
        kw = {k: v for k, v in kw.items() if k not in ("top_k", "refine_t", "refine_samples")}      # refine_pair has no clustering stage
    elif kind != "dock":
        kw.update(restraints=restraint_groups(), restraint_rank=kind[len("dock_"):].replace("restraint_", ""))
    out = str(tmp_path / f"{kind}_{family}.pdb")
    fn = driver.refine_pair if kind == "refine" else driver.dock_pair
    res = fn(model, rec, lig, None, None, num_samples=N_TRAJ, num_steps=5, seed=SEED, max_batch=MAX_BATCH, out_pdb=out, consensus_cutoff=6.0,
             **kw)
    assert len(model.handles) == 1
    return res, model.handles[0], model, out, kw


def screen_flags(rec, lig, cols, family):
    """CAPRI's flags of the trajectories, from the definition."""
    from dfmdock_amd import driver
    from dfmdock_amd import sterics as ST
    ra, la, cen = driver.sterics_inputs(rec, lig, family)
    return ST.capri_flags(ST.sterics(ra, la, cen, cols["rot_update"], cols["tr_update"])["n_clash"])[0]


def batchwise_minimum(energy):
    """The reference's pair loop: the first strict minimum over the batches' own first minima."""
    best = None
    for lo in range(0, len(energy), MAX_BATCH):
        k = lo + int(np.argmin(energy[lo:lo + MAX_BATCH]))
        if best is None or energy[k] < energy[best]:
            best = k
    return best


def expected_index(kind, kw, rec, lig, cols, family):
    """The kept trajectory, restated: drop the flagged poses unless all are flagged, then consensus.pick or the driver's own rule."""
    from dfmdock_amd import consensus as CS
    from dfmdock_amd.cluster import rebuild_backbone
    e = cols["energy"]
    ok = np.ones(len(e), bool)
    if kw.get("clash_filter"):
        flags = screen_flags(rec, lig, cols, family)
        if not flags.all():
            ok = ~flags
    if kw.get("rank") == "consensus":
        poses = rebuild_backbone(lig["bb_coords"], cols["rot_update"], cols["tr_update"], family)
        score = np.where(ok, CS.consensus(rec["bb_coords"], poses, 6.0, CS.energy_members(e, 1.0))["consensus"], np.nan)
        k = CS.pick(score, e)
        if k is not None:
            return int(k)
    if kind == "dock" and not any(k in kw for k in ("consensus", "rank", "clash_screen", "clash_filter")):
        return batchwise_minimum(e)
    idx = np.nonzero(ok)[0]
    if kind == "dock_satisfied":
        s = cols["restraints_satisfied"]
        idx = idx[s[idx] == s[idx].max()]
    return int(idx[np.argmin(e[idx])])


def expected_keys(kind, kw):
    keys = set(BASE)
    cons, screen = "consensus" in kw or "rank" in kw, "clash_screen" in kw or "clash_filter" in kw
    if kind == "refine":
        keys |= {"index", "t_begin", "trajectories"}
    elif kind != "dock":
        keys |= {"index", "restraints", "restraint_rank", "restraint_energy", "restraints_satisfied", "trajectories"}
    elif cons or screen:
        keys |= {"index", "trajectories"}
    if cons:
        keys |= {"consensus", "consensus_data"}
    if screen:
        keys |= {"sterics", "sterics_data"}
    if "native" in kw:
        keys |= {"metrics"} | ({"start_metrics"} if kind == "refine" else set())
    if "top_k" in kw:
        keys |= {"models", "cluster_of"}
    return keys


def test_the_fixture_exercises_every_path(pair):
    """One pose is flagged (and has the lowest energy), some but not all poses have consensus contacts and the satisfied groups vary: so
    the filter, rank="consensus" and restraint_rank="satisfied" each keep another trajectory than the energy does."""
    from dfmdock_amd import consensus as CS
    from dfmdock_amd.cluster import rebuild_backbone
    rec, lig = pair
    assert len(rec["bb_coords"]) == 12 and len(lig["bb_coords"]) == 8
    for family in (0, 1):
        gx = FakeComplex(FakeModel(family), None, None, rec["bb_coords"], lig["bb_coords"])
        gx.set_restraints(restraint_groups())
        for lo in range(0, N_TRAJ, MAX_BATCH):
            gx.restraint_eval(gx.sample(B=min(MAX_BATCH, N_TRAJ - lo), seed=SEED + lo, restraints=True)["lig_pos"])
        cols = gx.columns()
        flags = screen_flags(rec, lig, cols, family)
        assert np.nonzero(flags)[0].tolist() == [OVERLAP] and int(np.argmin(cols["energy"])) == OVERLAP
        poses = rebuild_backbone(lig["bb_coords"], cols["rot_update"], cols["tr_update"], family)
        score = CS.consensus(rec["bb_coords"], poses, 6.0)["consensus"]
        assert 2 <= np.isfinite(score).sum() and CS.pick(np.where(flags, np.nan, score), cols["energy"]) != np.argmin(np.where(flags, np.inf, cols["energy"]))
        assert len(set(cols["restraints_satisfied"].tolist())) > 1
        kinds = {k: expected_index(k, {}, rec, lig, cols, family) for k in DRIVERS}
        assert kinds["dock_satisfied"] != kinds["dock_restraint_energy"] == kinds["dock"] == OVERLAP


@pytest.mark.parametrize("name", list(OPTIONS))
@pytest.mark.parametrize("kind", DRIVERS)
def test_result_entries_kept_pose_files_and_handle(monkeypatch, tmp_path, pair, kind, name):
    import os
    from dfmdock_amd import driver, pdbio
    rec, lig = pair
    for family in (0, 1):
        res, gx, model, out, kw = run(monkeypatch, tmp_path, pair, kind, OPTIONS[name], family)
        cols, log = gx.columns(), list(model.log)
        # the entries of the result
        assert set(res) == expected_keys(kind, kw), (kind, name, sorted(res))
        if kind == "refine":
            assert res["t_begin"] == 0.1 and list(res["trajectories"]) == list(COLUMNS)
        elif kind != "dock":
            assert list(res["trajectories"]) == ["energy", "restraint_energy", "restraints_satisfied"]
            assert res["restraints"] == 4 and res["restraint_rank"] == kw["restraint_rank"]
        elif "trajectories" in res:
            assert list(res["trajectories"]) == list(COLUMNS)
        for c, v in res.get("trajectories", {}).items():
            assert np.array_equal(v, cols[c]) and len(v) == N_TRAJ, c
        # the kept pose
        k = expected_index(kind, kw, rec, lig, cols, family)
        if "index" in res:
            assert res["index"] == k and type(res["index"]) is int
        assert res["energy"] == float(cols["energy"][k]) and type(res["energy"]) is float
        assert np.array_equal(res["rot_update"], cols["rot_update"][k]) and np.array_equal(res["tr_update"], cols["tr_update"][k])
        if kind.startswith("dock_"):
            assert res["restraint_energy"] == float(cols["restraint_energy"][k]) and res["restraints_satisfied"] == int(cols["restraints_satisfied"][k])
            assert gx.calls["set_restraints"] == 1
        else:
            assert gx.calls["set_restraints"] == 0
        aa = pdbio.apply_pose_all_atom(lig["aa_coords"], lig["bb_coords"], cols["rot_update"][k], cols["tr_update"][k],
                                       center="all_atoms" if family == 1 else "ca")
        assert np.array_equal(res["lig_aa_coords"], aa)
        flags = screen_flags(rec, lig, cols, family)
        if "sterics" in res:
            assert np.array_equal(res["sterics_data"]["flags"], flags) and res["sterics"]["flagged"] == bool(flags[k])
            assert res["sterics"]["filtered"] == bool(kw.get("clash_filter")) and not res["sterics"]["fallback"]
        if "consensus" in res:
            assert res["consensus"]["ranked_by"] == kw.get("rank", "energy") and not res["consensus"]["fallback"]
        models = res.get("models", [])
        if kw.get("clash_filter"):      # a flagged pose is neither kept nor a model
            assert not flags[k] and not any(flags[m["index"]] for m in models)
        # the files: output.pdb holds the kept pose; model 1 under rule "energy" is that pose
        lines = open(out).read().splitlines()
        assert [l.startswith("REMARK dfmdock_amd sterics") for l in lines[:2]] == ["sterics" in res, False]
        ref = str(tmp_path / "ref.pdb")
        pdbio.write_complex_pdb(ref, list(rec["atoms"]), lig["atoms"], aa, remarks=driver._remarks(res.get("sterics_data"), k))
        assert open(out).read() == open(ref).read()
        if "top_k" in kw:
            assert 1 <= len(models) <= 3 and [m["rank"] for m in models] == list(range(1, len(models) + 1)) and models[0]["index"] == k
            assert len(res["cluster_of"]) == N_TRAJ
            assert all(os.path.exists(driver.model_path(out, m["rank"])) for m in models)
            if "refine_t" not in kw:
                assert open(driver.model_path(out, 1)).read() == open(out).read()
            assert all(("refined_energy" in m) == ("refine_t" in kw) and ("metrics" in m) == ("native" in kw) and
                       ("refined_metrics" in m) == ("native" in kw and "refine_t" in kw) and ("sterics" in m) == ("sterics" in res) for m in models)
        if "native" in kw:
            assert set(res["metrics"]) == set(driver.METRIC_FIELDS)
        if "start_metrics" in res:      # the native is the input pose
            assert res["start_metrics"]["DockQ"] == pytest.approx(1.0) and res["start_metrics"]["l_rmsd"] == pytest.approx(0.0, abs=1e-4)
        # the handle: closed once - after the refinement of the centres, else right after sampling and before any post-processing
        assert gx.calls["close"] == 1 and log.count("close") == 1
        at = log.index("close")
        if "refine_t" in kw:
            assert at == len(log) - 1 and log.count("draw") == 4
        else:
            assert log[:at] == ["draw"] * 3 and "draw" not in log[at:] and "write" in log[at:]


@pytest.mark.parametrize("opts", [{}, {"top_k": 3}], ids=["none", "top_k"])
def test_plain_dock_pair_keeps_the_batchwise_minimum(monkeypatch, tmp_path, pair, opts):
    """A NaN energy makes np.argmin of its batch point at the NaN, which no strict `<` accepts: the plain path then keeps the minimum of
    the batches before - neither the NaN (np.argmin of all energies) nor the lower finite energy next to it (np.nanargmin)."""
    res, gx, _, _, _ = run(monkeypatch, tmp_path, pair, "dock", opts, 0, nan=True)
    e = gx.columns()["energy"]
    k = batchwise_minimum(e)
    assert k == OVERLAP and int(np.argmin(e)) == N_TRAJ - 1 and int(np.nanargmin(e)) == N_TRAJ - 2
    assert res["energy"] == float(e[k]) and np.array_equal(res["tr_update"], gx.columns()["tr_update"][k]) and "index" not in res


RANKS = ("energy", "consensus", "interface", "distogram", "pairpot")
EVERY = dict(consensus=True, clash_filter=True, bsa=True, min_bsa=150.0, interface_energy=True, affinity=True, hbonds=True, native=True, top_k=3,
             refine_t=0.1, refine_samples=2)
MODEL_KEYS = ["rank", "index", "energy", "cluster_size", "sterics", "bsa", "bsa_rec", "bsa_lig", "interface_energy", "affinity", "dist_nll",
              "dist_nll_near", "exp_contacts", "n_hbond", "hb_bb_bb", "hb_bb_sc", "hb_sc_sc", "n_salt", "n_unsat", "pair_potential", "metrics",
              "refined_metrics", "refined_energy", "refined_index"]      # in the order the result line prints them
DISTOGRAM_KEYS = {"dist_nll", "dist_nll_near", "exp_contacts"}


def stub_analyses(monkeypatch, seen):
    """Every analysis of the pair drivers that would need the device, answered by fixed seeded arrays of N_TRAJ poses; each call appends its
    name to the model's log and its arguments of interest to `seen`."""
    from dfmdock_amd import driver
    rng = np.random.default_rng(77)
    n = N_TRAJ
    draw = lambda: rng.permutation(n).astype(np.float64) - 4.5      # no ties; the minimum is somewhere else every time
    total, ppe, nll = draw(), draw(), draw()
    kind = rng.integers(0, 5, (n, 3))

    def ensemble_surface(model, rec, lig, rot, tr, probe, points, per_atom=False):
        model.log.append("surface")
        seen.setdefault("surface", []).append((probe, points, per_atom))
        bd = {"bsa": np.arange(n) * 100.0, "bsa_rec": np.arange(n) * 60.0, "bsa_lig": np.arange(n) * 40.0, "probe": probe, "sphere_points": points}
        if per_atom:
            bd.update(rec_exposed=np.int32([4, 0, 0, 6]), lig_exposed=np.int32([0, 5]), rec_buried=np.int32([[4, 0, 0, 5]] * n), lig_buried=np.int32([[0, 5]] * n))
        return bd

    def ensemble_interface_energy(model, rec, lig, rot, tr, cutoff, weights):
        model.log.append("interface")
        return {"rep": np.arange(n) + 0.5, "att": -np.arange(n) - 0.25, "elec": np.zeros(n), "total": total.copy(), "n_pairs": np.arange(100, 100 + n)}

    def ensemble_pairpot(model, rec, lig, rot, tr, pot):
        model.log.append("pairpot")
        return {"energy": ppe.copy(), "n_pairs": np.arange(200, 200 + n), "n_untyped": 2, "T": 3, "NB": 30, "cutoff": 15.0}

    def pose_affinity(model, rec, lig, rot, tr, cutoff, probe, points, surface=None):
        model.log.append("affinity")
        seen["affinity_surface"] = surface
        ic = np.arange(6 * n).reshape(n, 6)
        return {"ic": ic, "n_pairs": ic.sum(1), "n_rec_res": np.arange(n), "n_lig_res": np.arange(n) + 1, "nis_apolar": np.linspace(30, 40, n),
                "nis_charged": np.linspace(20, 25, n), "dg": -np.arange(n) - 7.0, "kd": np.full(n, 1e-6), "cutoff": cutoff}

    def ensemble_hbonds(model, rec, lig, rot, tr, hb_cutoff, min_angle, salt_cutoff, per_atom=False):
        model.log.append("hbonds")
        seen["hbonds_per_atom"] = per_atom
        hd = {"n_hbond": kind.sum(1), "hb_kind": kind, "n_salt": np.arange(n) + 2, "untyped": (0, 0),
              "rec_polar": {"role": np.uint8([1, 2]), "index": np.array([0, 3])}, "lig_polar": {"role": np.uint8([3]), "index": np.array([1])}}
        if per_atom:
            hd.update(rec_hb=np.zeros((n, 2), np.int32), lig_hb=(np.arange(n)[:, None] % 2).astype(np.int32))
        return hd

    def ensemble_distogram(gx, rot, tr, t, precision, max_batch, maps=False, seed=0):
        gx.model.log.append("distogram")
        assert gx.calls["close"] == 0, "the distogram needs the open handle"
        return {"nll": nll.copy(), "nll_near": nll + 0.5, "n_near": np.arange(n), "exp_contacts": np.arange(n) + 10.0, "t": float(t), "contact_bins": 7}
    for f in (ensemble_surface, ensemble_interface_energy, ensemble_pairpot, pose_affinity, ensemble_hbonds, ensemble_distogram):
        monkeypatch.setattr(driver, f.__name__, f)
    return {"interface": total, "pairpot": ppe, "distogram": nll}


def seeded_table():
    rng = np.random.default_rng(3)
    return {"edges": np.linspace(0.0, 15.0, 31).astype(np.float32), "table": rng.uniform(-1.0, 1.0, (3, 3, 30)).astype(np.float32),
            "type_names": ["@C", "@N", "*"]}


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("kind", DRIVERS)
def test_every_analysis_at_once(monkeypatch, tmp_path, pair, kind, rank):
    """Every analysis switched on together, under every rank: the order of the calls, the entries of the result and of every model, which
    pose is kept, who says it ranked, and that every summary describes that one pose."""
    from dfmdock_amd import driver
    rec, lig = pair
    for family in (0, 1):
        seen = {}
        column = stub_analyses(monkeypatch, seen)
        opts = dict(EVERY, rank=rank, pair_potential=seeded_table(), **({"distogram": True} if family == 1 else {}))
        if rank == "distogram" and family == 0:      # the head exists in the second family only: refused before a handle is made
            monkeypatch.setattr(driver.engine, "Complex", FakeComplex)
            with pytest.raises(ValueError, match="family-1"):
                (driver.refine_pair if kind == "refine" else driver.dock_pair)(FakeModel(0), rec, lig, None, None, **{k: v for k, v in opts.items() if k != "native"})
            continue
        res, gx, model, out, kw = run(monkeypatch, tmp_path, pair, kind, opts, family)
        cols, log, models = gx.columns(), list(model.log), res.get("models", [])
        dock, dg = kind != "refine", family == 1
        # the order of events
        want = ["draw"] * 3 + (["close"] if not dock and not dg else []) + ["sterics"] + (["distogram"] if dg else []) + \
               (["close"] if not dock and dg else []) + ["interface", "pairpot", "consensus", "surface", "affinity", "hbonds", "write", "metrics"]
        if dock:
            want += ["cluster"] + ["write"] * len(models) + ["metrics", "draw", "metrics"] + ["write"] * len(models) + ["close"]
        else:
            want += ["metrics"]      # start_metrics
        assert log == want, (kind, rank, family, log)
        assert seen["surface"] == [(float(np.float32(1.4)), 128, True)] and seen["affinity_surface"] is res["bsa_data"] and seen["hbonds_per_atom"] is True
        # the entries of the result and of every model
        keys = expected_keys(kind, {k: v for k, v in kw.items() if k in ("consensus", "rank", "clash_filter", "native", "top_k")}) | {
            "index", "trajectories", "bsa", "bsa_rec", "bsa_lig", "bsa_data", "probe", "sphere_points", "min_bsa", "interface_energy", "interface_data",
            "pair_potential", "pairpot_data", "affinity", "affinity_data", "n_hbond", "hb_bb_bb", "hb_bb_sc", "hb_sc_sc", "n_salt", "n_unsat", "hbond_data"}
        keys |= ({"distogram", "distogram_data"} if dg else set()) | ({"bsa_dropped"} if dock else set())
        assert set(res) == keys, (kind, rank, family, sorted(set(res) ^ keys))
        assert list(res["trajectories"]) == (list(COLUMNS) if kind in ("dock", "refine") else ["energy", "restraint_energy", "restraints_satisfied"])
        assert len(models) >= 1 if dock else "models" not in res
        for m in models:
            assert list(m) == [k for k in MODEL_KEYS if dg or k not in DISTOGRAM_KEYS], list(m)
        # the kept pose: the lowest value of the rank's column among the poses the filter left
        flags = screen_flags(rec, lig, cols, family)
        assert np.nonzero(flags)[0].tolist() == [OVERLAP]
        if rank in column:
            k = int(np.argmin(np.where(flags, np.inf, column[rank])))
        else:
            k = expected_index(kind, {k: v for k, v in kw.items() if k in ("rank", "clash_filter")}, rec, lig, cols, family)
        assert res["index"] == k and res["energy"] == float(cols["energy"][k]) and np.array_equal(res["rot_update"], cols["rot_update"][k])
        if dock:
            assert res["bsa_dropped"] + len(models) <= 3 and all(m["bsa"] >= 150.0 and not flags[m["index"]] for m in models)
            if k >= 2:
                assert models[0]["index"] == k      # under rule "energy" model 1 is the kept pose, unless min_bsa drops it
        # who ranked
        assert res["consensus"]["ranked_by"] == rank and res["consensus"]["fallback"] is False
        assert res["interface_energy"]["ranked_by"] == rank
        if dg:
            assert res["distogram"]["ranked_by_distogram"] is (rank == "distogram")
        assert res["sterics"]["filtered"] is True and res["sterics"]["fallback"] is False and res["min_bsa"] == 150.0
        # every summary is that of the kept pose, every model's that of its own
        has = lambda whole, part: {key: whole[key] for key in part} == part
        for at, into in [(k, res)] + [(m["index"], m) for m in models]:
            assert has(into["sterics"], driver._pose_sterics(res["sterics_data"], at)) and has(into, driver._pose_bsa(res["bsa_data"], at))
            assert has(into["interface_energy"], driver._pose_interface(res["interface_data"], at))
            assert into["pair_potential"] == driver._pose_pairpot(res["pairpot_data"], at) and into["affinity"] == driver._pose_affinity(res["affinity_data"], at)
            assert has(into, driver._pose_hbonds(res["hbond_data"], at)) and "n_unsat" in driver._pose_hbonds(res["hbond_data"], at)
            if dg:
                assert has(into["distogram"] if into is res else into, driver._pose_distogram(res["distogram_data"], at))
        assert res["consensus"]["n_contacts"] == int(res["consensus_data"]["n_contacts"][k])
        for name in ("pairpot_data", "hbond_data"):      # they carry the poses their arrays are of
            assert np.array_equal(res[name]["rot_update"], cols["rot_update"]) and np.array_equal(res[name]["tr_update"], cols["tr_update"])
        assert gx.calls["close"] == 1


@pytest.mark.parametrize("rank", ("energy", "interface", "distogram", "pairpot"))
def test_ranked_by_without_consensus(monkeypatch, tmp_path, pair, rank):
    """Without the consensus option `interface_energy` names the rule that kept the pose - except rank "distogram", which it reports as
    "energy" (the distogram object says ranked_by_distogram)."""
    column = stub_analyses(monkeypatch, {})
    res, gx, _, _, _ = run(monkeypatch, tmp_path, pair, "refine", dict(rank=rank, interface_energy=True, distogram=True, pair_potential=seeded_table()), 1)
    want = int(np.argmin(column[rank])) if rank in column else int(np.argmin(gx.columns()["energy"]))
    assert res["index"] == want and "consensus" not in res
    assert res["interface_energy"]["ranked_by"] == {"distogram": "energy"}.get(rank, rank) and res["distogram"]["ranked_by_distogram"] is (rank == "distogram")
