"""A fixed list of calls over the whole public surface of the engine, for runs under the allocator diagnostics (DFM_ALLOC_POISON,
DFM_ALLOC_GUARD: dfmdock_amd/csrc/dfm_host.h).  Every call stores ALL of its outputs under a stable key; the only things left out are
clocks (`*_last_timing`, the millisecond / cycle fields of `profile()`).

Three groups - trunk, start, analysis - one child process each (`python tests/alloc_recipe.py GROUP OUT.npz`; the diagnostic switches are
read once per process).  The child opens the group's handles, runs the group (pass 1), makes a dirtying pass on the SAME handles - other
engines and flags, a larger then a smaller batch so that the workspace grows and is then under-used, another restraint set - and runs
the group again (pass 2).  It stores pass 1, the keys at which pass 2 differs from it bit for bit (and pass 2's arrays at those keys),
then closes every handle, trims the block cache and stores `alloc_diag()` and `config_string()`.

The recipe is sized for a device of 256 compute units (MI355X): the trunk group's B = 44 launch on 120 + 94 residues is the
dynamic-task form of the message and coordinate kernels there, which the child asserts (edge_harness.task_form / coord_form on the
device's own CU count) before it stores anything - on another CU count the trunk child fails at that assert.

`compare(a, b)` is the comparer of tests/test_gpu_alloc_diag.py: dtype, shape and bytes, so NaNs compare by their bits.
tests/test_alloc_recipe_cpu.py holds it against seeded mutants.  Importing this module needs numpy only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GROUPS = ("trunk", "start", "analysis")
META = ("__pass2_differs", "__diag", "__config", "__seconds")      # what the child adds to the recipe's keys
DIAG = ("blocks", "poisoned_bytes", "bands_checked", "bands_damaged", "first_damaged_size", "first_damaged_offset")
PROFILE_COUNTS = ("edge_kernel_launches", "edge_rows", "l0_evals", "l0_edges", "l0_miss_rows", "edge_lig_launches")
ENGINES = {"fp32": {}, "mfma16": dict(mfma16=True), "f16": dict(f16=True), "bf16_ops": dict(mfma16=True, bf16_ops=True)}
# The launch on the dynamic-task form of the message AND the coordinate kernel: B >= 8, B * N >= 2 * CUs * EDGE_WAVES without the tile form
# winning (edge_harness.tile_tasks: on 256 CUs B = 20 .. 23 of these 214 nodes still run as tiles), and B * L >= 2 * CUs * EDGE_WAVES
DYN = dict(R=120, L=94, B=44, steps=3)


# ---------------------------------------------------------------------------------------------------------------------------------
def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def compare(a, b):
    """The keys (in a's order, then b's extra ones) at which two result sets differ in dtype, shape or bytes, or which one of them lacks.
    Keys that begin with "__" are the child's own (META, pass 2's arrays at the keys where it differs), not the recipe's."""
    out = [k for k in a if not k.startswith("__") and (k not in b or not same(a[k], b[k]))]
    return out + [k for k in b if not k.startswith("__") and k not in a]


class Results(dict):
    """key -> array, in the order of the calls; a key is stored once"""

    def put(self, name, value):
        if isinstance(value, dict):
            for k, v in value.items():
                self.put(f"{name}/{k}", v)
            return
        assert name not in self and not name.startswith("__"), name
        a = np.asarray(value)
        assert a.dtype != object, name
        self[name] = a.copy()


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def complex_7cei():
    from dfmdock_amd.synthetic import seq_to_onehot
    d = load_golden("cx_7CEI")
    rx = np.concatenate([d["rec_esm16"].astype(np.float32), seq_to_onehot(str(d["rec_seq"]))], 1)
    lx = np.concatenate([d["lig_esm16"].astype(np.float32), seq_to_onehot(str(d["lig_seq"]))], 1)
    return {"rec_x": rx, "lig_x": lx, "rec_pos": d["rec_pos"], "lig_pos": d["lig_pos"]}


def moved(lig_pos, n, seed, spread=3.0, jitter=0.0):
    """n poses [n,L,3,3]: the pose translated by N(0, spread^2) per axis (pose 0 stays), every atom jittered by N(0, jitter^2)"""
    rng = np.random.default_rng(seed)
    tr = (spread * rng.standard_normal((n, 1, 1, 3))).astype(np.float32)
    tr[0] = 0
    p = np.asarray(lig_pos, np.float32)[None] + tr
    if jitter:
        p = p + (jitter * rng.standard_normal(p.shape)).astype(np.float32)
    return np.ascontiguousarray(p, np.float32)


def profile_counts(gx):
    p = gx.profile()
    return {k: np.int64(p[k]) for k in PROFILE_COUNTS}


def close_all(handles):
    for h in handles:
        h.close()


def device_cus():
    """compute units of device 0, from the HIP runtime the engine itself is linked against (dlsym searches a library's dependencies)"""
    import ctypes as C
    from dfmdock_amd import _lib
    n = C.c_int(0)
    e = _lib.lib().hipDeviceGetAttribute(C.byref(n), 63, 0)      # hipDeviceAttributeMultiprocessorCount
    assert e == 0 and n.value > 0, (e, n.value)
    return n.value


# --------------------------------------------------------------------------------------------------------------------------- trunk
class Trunk:
    def __init__(self):
        from dfmdock_amd import engine
        from dfmdock_amd.synthetic import make_complex
        from dfmdock_amd.weights import HParams, make_random_weights, pack_blob
        hp1 = HParams(family=1, mask_dist=20.0)
        hp67 = HParams(family=1, mask_dist=20.0, positional_embed_dim=67)
        self.m0 = engine.Model(pack_blob(make_random_weights(0)))
        self.m1 = engine.Model(pack_blob(make_random_weights(0, hp1), hp1), hp1)
        self.m67 = engine.Model(pack_blob(make_random_weights(0, hp67), hp67), hp67)
        self.syn, self.c7, self.big = make_complex(24, 16, seed=5), complex_7cei(), make_complex(DYN["R"], DYN["L"], seed=3)
        mk = lambda m, c: engine.Complex(m, c["rec_x"], c["lig_x"], c["rec_pos"], c["lig_pos"])
        self.g0, self.g1, self.g67 = mk(self.m0, self.syn), mk(self.m1, self.syn), mk(self.m67, self.syn)
        self.g7, self.gbig, self.gpose = mk(self.m0, self.c7), mk(self.m0, self.big), mk(self.m0, self.syn)
        self.handles = [self.g0, self.g1, self.g67, self.g7, self.gbig, self.gpose, self.m0, self.m1, self.m67]
        self.cus = device_cus()

    def run(self):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import edge_harness as eh
        r = Results()
        g, g2, g7 = load_golden("fwd_syn_24_16"), load_golden("fwd2_syn_24_16"), load_golden("fwd_7CEI_p0")
        poses = np.concatenate([g["lig_pos"].reshape(1, 16, 3, 3), moved(self.syn["lig_pos"], 3, 21, 2.0)[1:]])
        t3 = np.float32([float(g["t"]), 0.9, 0.05])
        # score: every engine with the debug taps and the interface head, on engine-drawn graphs; the table where an engine has one
        for name, kw in ENGINES.items():
            r.put(f"score/{name}", self.g0.score(poses, t3, seed=11, debug=True, ires=True, **kw))
            if name in ("fp32", "mfma16"):
                r.put(f"score_l0/{name}", self.g0.score(poses, t3, seed=11, debug=True, ires=True, l0_table=True, **kw))
        r.put("score_golden_edges/mfma16", self.g0.score(g["lig_pos"], float(g["t"]), edges=g["edges"], mfma16=True, debug=True))
        r.put("score_7cei/mfma16", self.g7.score(g7["lig_pos"], float(g7["t"]), edges=g7["edges"], mfma16=True, ires=True, return_edges=True))
        r.put("score_7cei_l0/fp32", self.g7.score(moved(self.c7["lig_pos"], 2, 22), 0.3, seed=5, l0_table=True, debug=True))
        # the second family: pair heads, confidence, dist_logits
        for name, kw in ENGINES.items():
            r.put(f"score_pair/{name}", self.g1.score(np.concatenate([g2["lig_pos"].reshape(1, 16, 3, 3), poses[1:]]), t3, seed=12, dist=True,
                                                     debug=True, ires=True, **kw))
        # sample: three engines x table on / off, traced; then the flags
        for name in ("fp32", "mfma16", "f16"):
            for l0 in (True, False):
                r.put(f"sample/{name}/l0_{int(l0)}", self.g0.sample(B=3, num_steps=4, seed=31, trace=True, l0_table=l0, **ENGINES[name]))
        r.put("sample_pair/mfma16", self.g1.sample(B=3, num_steps=4, seed=32, trace=True, mfma16=True))
        r.put("sample_graph/mfma16", self.g0.sample(B=3, num_steps=4, seed=33, graph=True, mfma16=True))
        r.put("sample_graph/fp32", self.g0.sample(B=2, num_steps=4, seed=33, graph=True))
        r.put("sample_graph_clash/mfma16", self.g0.sample(B=3, num_steps=4, seed=34, graph=True, mfma16=True, use_clash_force=True, l0_table=False))
        r.put("sample_ode/mfma16", self.g0.sample(B=3, num_steps=4, seed=35, trace=True, mfma16=True, ode=True))
        r.put("sample_annealing/mfma16", self.g0.sample(B=3, num_steps=4, seed=36, trace=True, mfma16=True, noise_annealing=True))
        r.put("sample_clash/mfma16", self.g0.sample(B=3, num_steps=4, seed=37, trace=True, mfma16=True, use_clash_force=True))
        r.put("sample_untraced/mfma16", self.g7.sample(B=2, num_steps=4, seed=38, mfma16=True))
        r.put("sample_profile/mfma16", self.g0.sample(B=2, num_steps=4, seed=39, mfma16=True, profile=True))
        r.put("sample_profile/mfma16/profile", profile_counts(self.g0))
        # one launch on the dynamic-task form of the message and coordinate kernels
        B, N, Lg = DYN["B"], DYN["R"] + DYN["L"], DYN["L"]
        assert eh.task_form(B, N, self.gbig.K, self.cus) == "dynamic" and eh.coord_form(B, Lg, self.cus) == "dynamic", (B, N, self.cus)
        r.put("sample_dynamic/mfma16", self.gbig.sample(B=B, num_steps=DYN["steps"], seed=40, mfma16=True))
        # selfcheck
        for name in ("mfma16", "f16"):
            r.put(f"selfcheck/{name}", {k: v for k, v in self.g0.selfcheck(n_eval=3, seed=41, precision=name).items() if k != "precision"})
        # set_pose: the table is rebuilt; then back
        self.gpose.set_pose(rec_pos=self.syn["rec_pos"] + np.float32(0.25), lig_pos=poses[1])
        r.put("set_pose/sample", self.gpose.sample(B=2, num_steps=4, seed=42, mfma16=True, trace=True))
        r.put("set_pose/score_l0", self.gpose.score(poses[:2], 0.4, seed=43, l0_table=True, debug=True))
        self.gpose.set_pose(rec_pos=self.syn["rec_pos"], lig_pos=self.syn["lig_pos"])
        r.put("set_pose/back", self.gpose.sample(B=2, num_steps=4, seed=42, mfma16=True, trace=True))
        # the 67th position channel
        for flag in (1, 0):
            self.g67.set_homomer(bool(flag))
            r.put(f"homomer_{flag}/score", self.g67.score(poses[:2], 0.5, seed=44, mfma16=True, debug=True))
            r.put(f"homomer_{flag}/sample", self.g67.sample(B=2, num_steps=4, seed=45, mfma16=True, trace=True))
        return r

    def dirty(self):
        """largest B of the group on other engines with other flags; a larger, then a smaller batch on every complex"""
        self.gbig.sample(B=DYN["B"] + 3, num_steps=2, seed=90, f16=True, use_clash_force=True, l0_table=False)
        self.gbig.score(moved(self.big["lig_pos"], 2, 91), 0.7, seed=91, ires=True, l0_table=True)
        self.gbig.sample(B=1, num_steps=2, seed=92)
        for gx, c in ((self.g0, self.syn), (self.g1, self.syn), (self.g67, self.syn), (self.gpose, self.syn), (self.g7, self.c7)):
            gx.sample(B=7, num_steps=3, seed=93, f16=True, noise_annealing=True, graph=True)
            gx.score(moved(c["lig_pos"], 9, 94, 6.0), 0.95, seed=94, mfma16=True, bf16_ops=True, ires=True)
            gx.sample(B=1, num_steps=2, seed=95, use_clash_force=True, trace=True)


# --------------------------------------------------------------------------------------------------------------------------- start
def restraint_sets(R, Lg):
    """(the set of the recipe, another one for the dirtying pass): single pairs, one group above RS_SMALL = 16 pairs (a wave of its own),
    a zero-weight group"""
    from dfmdock_amd.restraints import RestraintGroup as G
    rng = np.random.default_rng(7)
    big = [(int(i), int(j)) for i, j in zip(rng.integers(0, R, 23), rng.integers(0, Lg, 23))]
    a = [G([(1, 2)], 6.0), G([(5, 0)], 8.0, 2.0), G(big, 5.0), G([(3, 3), (4, 9)], 7.0, 0.0), G([(R - 1, Lg - 1)], 4.0)]
    b = [G([(int(i), int(j)) for i, j in zip(rng.integers(0, R, 40), rng.integers(0, Lg, 40))], 3.0, 0.5)] + \
        [G([(int(i), int(i) % Lg)], 9.0) for i in range(0, R, 2)]
    return a, b


class Start:
    def __init__(self):
        from dfmdock_amd import engine
        from dfmdock_amd.synthetic import make_complex
        from dfmdock_amd.weights import HParams, make_random_weights, pack_blob
        hp1 = HParams(family=1, mask_dist=20.0)
        self.m0 = engine.Model(pack_blob(make_random_weights(0)))
        self.m1 = engine.Model(pack_blob(make_random_weights(0, hp1), hp1), hp1)
        self.syn = make_complex(24, 16, seed=5)
        mk = lambda m, c: engine.Complex(m, c["rec_x"], c["lig_x"], c["rec_pos"], c["lig_pos"])
        self.g0, self.g1, self.gr = mk(self.m0, self.syn), mk(self.m1, self.syn), mk(self.m0, self.syn)
        self.handles = [self.g0, self.g1, self.gr, self.m0, self.m1]
        self.sets = restraint_sets(24, 16)

    def run(self):
        r = Results()
        for t in (0.05, 0.1, 0.6):
            r.put(f"igso3_table/{t}", self.m0.igso3_table(t))
        r.put("igso3_table/pair/0.1", self.m1.igso3_table(0.1))
        for t in (0.1, 0.6):
            r.put(f"forward_marginal/{t}", self.g0.forward_marginal(5, t, seed=51))
        start = moved(self.syn["lig_pos"], 3, 52, 1.5)
        for fam, gx in (("score", self.g0), ("pair", self.g1)):
            r.put(f"refine/{fam}", gx.refine(B=3, t_begin=0.1, num_steps=4, seed=53, mfma16=True, trace=True))
            r.put(f"refine_fp32/{fam}", gx.refine(B=3, t_begin=0.3, num_steps=4, seed=54, trace=True))
            r.put(f"refine_start_pos/{fam}", gx.refine(B=3, t_begin=0.1, start_pos=start, num_steps=4, seed=55, mfma16=True, trace=True))
            r.put(f"refine_no_perturb/{fam}", gx.refine(B=3, t_begin=0.1, start_pos=start, perturb=False, num_steps=4, seed=56, mfma16=True,
                                                       trace=True))
        r.put("refine_graph/score", self.g0.refine(B=3, t_begin=0.2, num_steps=4, seed=57, mfma16=True, graph=True))
        # restraints
        self.gr.set_restraints(self.sets[0])
        r.put("restraint_eval", self.gr.restraint_eval(moved(self.syn["lig_pos"], 4, 58, 4.0)))
        r.put("restrained/sample", self.gr.sample(B=3, num_steps=4, seed=59, mfma16=True, trace=True, restraints=True))
        r.put("restrained/sample_clash", self.gr.sample(B=3, num_steps=4, seed=60, mfma16=True, trace=True, restraints=True, use_clash_force=True))
        r.put("restrained/sample_graph", self.gr.sample(B=3, num_steps=4, seed=61, mfma16=True, graph=True, restraints=True))
        r.put("restrained/refine", self.gr.refine(B=3, t_begin=0.1, num_steps=4, seed=62, mfma16=True, trace=True, restraints=True))
        self.gr.set_restraints(None)
        r.put("cleared/sample", self.gr.sample(B=3, num_steps=4, seed=59, mfma16=True, trace=True, restraints=True))
        return r

    def dirty(self):
        self.gr.set_restraints(self.sets[1])
        self.gr.sample(B=9, num_steps=3, seed=96, f16=True, restraints=True, use_clash_force=True)
        self.gr.restraint_eval(moved(self.syn["lig_pos"], 11, 97, 9.0))
        self.gr.refine(B=1, t_begin=0.5, num_steps=2, seed=98, restraints=True)
        for gx in (self.g0, self.g1):
            gx.refine(B=8, t_begin=0.9, num_steps=3, seed=99, f16=True, noise_annealing=True, l0_table=False)
            gx.forward_marginal(17, 0.95, seed=100)
            gx.sample(B=1, num_steps=2, seed=101, graph=True)
        self.m0.igso3_table(0.33)


# ------------------------------------------------------------------------------------------------------------------------ analysis
def rigid_poses(seed):
    """9 poses of the rigid-body calls: 0 the identity, 1-4 near, 5-7 far from the receptor (waves that leave early), 8 not a number"""
    rng = np.random.default_rng(seed)
    rot, tr = (0.2 * rng.standard_normal((9, 3))).astype(np.float32), (2.0 * rng.standard_normal((9, 3))).astype(np.float32)
    rot[0], tr[0] = 0, 0
    tr[5:8] += np.float32([[300.0, 0, 0], [0, -250.0, 0], [40.0, 40.0, 40.0]])
    rot[8, 1] = np.nan
    return rot, tr


class Analysis:
    def __init__(self):
        from dfmdock_amd import engine, pdbio
        from dfmdock_amd.synthetic import make_complex
        from dfmdock_amd.weights import make_random_weights, pack_blob
        self.m0 = engine.Model(pack_blob(make_random_weights(0)))
        self.c7 = complex_7cei()
        self.small, self.mid = make_complex(9, 7, seed=6), make_complex(70, 65, seed=8)
        self.nat = self.m0.native(self.c7["rec_pos"], self.c7["lig_pos"])
        five = lambda bb: pdbio.full_backbone(bb).reshape(-1, 3)
        rec, lig = five(self.c7["rec_pos"]), five(self.c7["lig_pos"])
        d2 = ((lig.astype(np.float64)[:, None] - rec.astype(np.float64)[None]) ** 2).sum(-1).min(1)
        order = np.argsort(d2, kind="stable")
        near = lambda Al: lig[np.sort(order[:Al])]      # the Al ligand atoms nearest the receptor, in their own order
        self.cen = np.asarray(self.c7["lig_pos"], np.float64)[:, 1].mean(0).astype(np.float32)
        radius = lambda n: np.tile(np.float32([1.55, 1.70, 1.70, 1.52, 1.70]), (n + 4) // 5)[:n]
        self.atoms = {Al: self.m0.atoms(rec, near(Al), self.cen) for Al in (1, 65, 130)}
        self.surf = {(Al, K): self.m0.surface(rec, radius(rec.shape[0]), near(Al), radius(Al), self.cen, points=K)
                     for Al, K in ((130, 64), (65, 128), (1, 64))}
        self.handles = [self.nat] + list(self.atoms.values()) + list(self.surf.values()) + [self.m0]

    def run(self):
        r = Results()
        Lg = self.c7["lig_pos"].shape[0]
        for B in (33, 257):
            poses = moved(self.c7["lig_pos"], B, 70 + B, 3.0, 0.3)
            key = np.random.default_rng(B).standard_normal(B).astype(np.float32)
            sub = np.arange(0, Lg, 3)
            r.put(f"pose_rmsd/{B}", self.m0.pose_rmsd(poses))
            r.put(f"pose_rmsd_sub/{B}", self.m0.pose_rmsd(poses, residues=sub))
            for rule in ("energy", "size"):
                r.put(f"pose_cluster/{rule}/{B}", self.m0.pose_cluster(poses, 5.0, key=key, rule=rule))
                r.put(f"pose_cluster_sub/{rule}/{B}", self.m0.pose_cluster(poses, 4.0, key=key, rule=rule, residues=sub, max_clusters=5))
            r.put(f"pose_cluster_nokey/{B}", self.m0.pose_cluster(poses, 5.0))
        r.put("native/info", self.nat.info())
        for P in (1, 9):
            lp = moved(self.c7["lig_pos"], P, 80 + P, 2.0, 0.2)
            rp = moved(self.c7["rec_pos"], P, 85 + P, 0.5, 0.1)
            r.put(f"metrics/{P}", self.nat.metrics(lp))
            r.put(f"metrics_rec/{P}", self.nat.metrics(lp, rp))
        for name, c in (("9_7", self.small), ("70_65", self.mid)):
            lp = moved(c["lig_pos"], 11, 88, 2.0)
            mem = np.arange(11) % 3 != 1
            r.put(f"consensus/{name}", self.m0.consensus(c["rec_pos"], lp, cutoff=8.0, bits=True))
            r.put(f"consensus_members/{name}", self.m0.consensus(c["rec_pos"], lp, cutoff=8.0, members=mem, bits=True))
        rot, tr = rigid_poses(89)
        for Al, at in self.atoms.items():
            for chunk in (0, 1, 7):
                r.put(f"sterics/{Al}/chunk_{chunk}", at.sterics(rot, tr, per_atom=True, chunk_poses=chunk))
            r.put(f"sterics_totals/{Al}", at.sterics(rot[:5], tr[:5]))
        for (Al, K), sf in self.surf.items():
            r.put(f"surface_info/{Al}/{K}", sf.info())
            for chunk in (0, 1, 7):
                r.put(f"bsa/{Al}/{K}/chunk_{chunk}", sf.bsa(rot, tr, per_atom=True, chunk_poses=chunk))
            r.put(f"bsa_totals/{Al}/{K}", sf.bsa(rot[:5], tr[:5]))
        return r

    def dirty(self):
        rng = np.random.default_rng(5)
        big = moved(self.c7["lig_pos"], 300, 102, 8.0, 1.0)
        self.m0.pose_cluster(big, 9.0, rule="size", max_clusters=3)
        self.m0.pose_rmsd(big[:40], residues=np.arange(5))
        self.nat.metrics(big[:40], moved(self.c7["rec_pos"], 40, 103, 1.0))
        self.nat.metrics(big[:2])
        self.m0.consensus(self.mid["rec_pos"], moved(self.mid["lig_pos"], 40, 104, 1.0), cutoff=12.0, bits=True)
        self.m0.consensus(self.small["rec_pos"], moved(self.small["lig_pos"], 3, 105, 1.0), cutoff=4.0)
        rot, tr = (0.5 * rng.standard_normal((40, 3))).astype(np.float32), (1.0 * rng.standard_normal((40, 3))).astype(np.float32)
        for at in self.atoms.values():
            at.sterics(rot, tr, per_atom=True, chunk_poses=16)
            at.sterics(rot[:2], tr[:2])
        for sf in self.surf.values():
            sf.bsa(rot, tr, per_atom=True, chunk_poses=16)
            sf.bsa(rot[:2], tr[:2])


# ---------------------------------------------------------------------------------------------------------------------------------
def run_group(group):
    """pass 1, the dirtying pass, pass 2 on the same handles; every handle closed, the cache trimmed; -> the dict the child stores"""
    import time
    from dfmdock_amd import engine
    t0 = time.perf_counter()
    engine.set_device(0)
    G = {"trunk": Trunk, "start": Start, "analysis": Analysis}[group]()
    one = G.run()
    G.dirty()
    two = G.run()
    differs = compare(one, two)
    close_all(G.handles)
    engine.trim_cache()
    out = dict(one)
    for k in differs:
        if k in two:
            out["__pass2/" + k] = two[k]
    d = engine.alloc_diag()
    out["__pass2_differs"] = np.array(differs, dtype="U200")
    out["__diag"] = np.array([d[k] for k in DIAG], np.int64)
    out["__config"] = np.array(engine.config_string())
    out["__seconds"] = np.float64(time.perf_counter() - t0)
    return out


def main(argv):
    if len(argv) != 3 or argv[1] not in GROUPS:
        print(f"usage: {argv[0]} {'|'.join(GROUPS)} OUT.npz", file=sys.stderr)
        return 2
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    out = run_group(argv[1])
    np.savez(argv[2], **out)
    print(f"{argv[1]}: {len(out) - len(META)} keys, pass 2 differs at {len(out['__pass2_differs'])}, {float(out['__seconds']):.1f} s, "
          f"diag {out['__diag'].tolist()}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
