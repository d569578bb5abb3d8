"""Non-finite poses through the whole trunk calls (include/dfmdock_amd.h, "non-finite poses in the trunk calls"):
dfm_score, dfm_sample, dfm_refine and dfm_score_distogram take poses unchecked, and an injected draw or a NaN step can make a trajectory
non-finite in the middle of a run.  For every call here:
  in range    every edge the call reports is a residue index in [0, N);
  contained   the other poses of the batch have, bit for bit, the outputs of the same call with the bad poses replaced by finite ones;
  visible     the bad pose's floating-point outputs are NaN (the energy too), its num_clashes is 0;
  refused     dfm_complex_create / dfm_complex_set_pose return DFM_E_INVALID for a non-finite stored pose and keep what was stored.
The kernels behind these calls are tested launch by launch, on guarded arrays, in tests/test_gpu_geom_kernels.py (the graph and its
ordering rule, the features, the table classification) and tests/test_gpu_head_kernels.py (pose preparation, energy, heads, pair heads):
those run first and this file relies on them - a graph with an edge out of range would be followed as an index here."""
import numpy as np
import pytest

from conftest import complex_for, pair_hparams

pytestmark = pytest.mark.gpu

NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
ENGINES = {"fp32": {}, "mfma16": dict(mfma16=True), "f16": dict(f16=True)}
FLOATS = ("tr_score", "rot_score", "energy", "f")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    m = engine.Model(blob)
    yield m
    m.close()


@pytest.fixture(scope="module")
def model_pair(blob_pair):
    from dfmdock_amd import engine
    m = engine.Model(blob_pair, pair_hparams())
    yield m
    m.close()


@pytest.fixture(scope="module")
def complexes(model):
    from dfmdock_amd import engine
    out = {}
    for case in ("syn_24_16", "7CEI"):
        cx = complex_for(case)
        out[case] = (engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"]), cx)
    yield out
    for gx, _ in out.values():
        gx.close()


def score_poses(lig):
    """B = 6: poses 0 and 2 finite (2 shifted); 1: one NaN coordinate in an N atom of one ligand residue; 3: all +NaN; 4: all NaN with
    the sign bit; 5: one +inf.  Returns (poses, the same with the four bad ones replaced by the stored pose, the bad indices)."""
    lig = np.asarray(lig, np.float32)
    good = np.repeat(lig[None], 6, 0)
    good[2] += np.float32(1.5)
    bad = good.copy()
    bad[1, lig.shape[0] // 2, 0, 1] = np.nan
    bad[3] = np.nan
    bad[4] = NEG_NAN
    bad[5, 0, 1, 2] = np.inf
    return bad, good, [1, 3, 4, 5]


def check_score(r, ref, badidx, N):
    ok = [b for b in range(len(r["energy"])) if b not in badidx]
    for k in FLOATS + ("num_clashes",):
        assert np.array_equal(bits(r[k][ok]), bits(ref[k][ok])), f"{k} of a finite pose changed beside a non-finite one"
        assert np.isfinite(ref[k]).all()
    for b in badidx:
        for k in FLOATS:
            assert np.isnan(r[k][b]).all(), f"pose {b}: {k} = {np.ravel(r[k][b])[:6]} is not NaN"
        assert r["num_clashes"][b] == 0
    if "edges" in r:
        assert ((r["edges"] >= 0) & (r["edges"] < N)).all(), f"edges up to {r['edges'].max()} of N = {N}"
        assert np.array_equal(r["edges"][ok], ref["edges"][ok])


# (the layer-0 table serves the fp32 and the mfma16 engine, a table each)
@pytest.mark.parametrize("engine_name,l0_table", [("fp32", False), ("fp32", True), ("mfma16", False), ("mfma16", True), ("f16", False)])
@pytest.mark.parametrize("case", ("syn_24_16", "7CEI"))
def test_score(complexes, case, engine_name, l0_table):
    """B = 6 with four bad poses; debug=True (the node taps and edge codes too) on the fp32 engine."""
    gx, cx = complexes[case]
    bad, good, badidx = score_poses(cx["lig_pos"])
    kw = dict(ENGINES[engine_name], seed=3, energy=True, l0_table=l0_table, return_edges=True)
    if engine_name == "fp32" and not l0_table:
        kw.update(debug=True, return_edges=False)
    r, ref = gx.score(bad, 0.5, **kw), gx.score(good, 0.5, **kw)
    check_score(r, ref, badidx, gx.N)


def test_score_pair_family(model_pair):
    from dfmdock_amd import engine
    cx = complex_for("syn_24_16")
    gx = engine.Complex(model_pair, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    bad, good, badidx = score_poses(cx["lig_pos"])
    for kw in ENGINES.values():
        kw = dict(kw, seed=3, energy=True, return_edges=True)
        check_score(gx.score(bad, 0.5, **kw), gx.score(good, 0.5, **kw), badidx, gx.N)
    # the distogram head, B = 3 with pose 1 NaN: per-pose outputs and map slices NaN, n_near 0, every entry of the pooled map NaN
    maps = ("pair_nll", "pcontact", "edist", "pcontact_mean")
    r, ref = gx.distogram(bad[:3], 0.5, seed=3, maps=maps), gx.distogram(good[:3], 0.5, seed=3, maps=maps)
    for k in ("nll", "nll_near", "exp_contacts", "n_near", "pair_nll", "pcontact", "edist"):
        assert np.array_equal(bits(r[k][[0, 2]]), bits(ref[k][[0, 2]])), k
        if k != "n_near":
            assert np.isnan(r[k][1]).all(), k
    assert r["n_near"][1] == 0 and np.isfinite(ref["pcontact_mean"]).all() and np.isnan(r["pcontact_mean"]).all()
    gx.close()


def traj_inject(B, S, bad, value, seed=0):
    rng = np.random.default_rng(seed)
    draw = (rng.standard_normal((B, 3)) * 30).astype(np.float32)
    good = dict(tr_draw=draw)
    nan = dict(tr_draw=draw.copy())
    nan["tr_draw"][bad] = value
    return nan, good


TRAJ_FLOATS = ("lig_pos", "rot_update", "tr_update", "energy", "final_scores")


def check_traj(r, ref, bad):
    B = len(r["energy"])
    ok = [b for b in range(B) if b != bad]
    for k in TRAJ_FLOATS + ("num_clashes",):
        assert np.array_equal(bits(r[k][ok]), bits(ref[k][ok])), f"{k} of a finite trajectory changed beside a non-finite one"
        assert np.isfinite(ref[k]).all(), k
    assert not np.isfinite(r["lig_pos"][bad]).any()
    for k in ("energy", "tr_update", "rot_update", "final_scores"):
        assert np.isnan(r[k][bad]).all(), f"{k} = {np.ravel(r[k][bad])}"
    assert r["num_clashes"][bad] == 0


SAMPLE_MODES = {"plain": {}, "graph": dict(graph=True), "clash_force": dict(use_clash_force=True), "restraints": dict(restraints=True),
                "fp32_no_table": dict(l0_table=False), "fp32": {}, "f16": dict(f16=True)}
# every mode on the small complex (N = 40: K = N, every residue an edge); the three engines and the clash force also on 7CEI (N = 214:
# a node without a number distance has 42 padding slots of the selection in front of it, and the race has more candidates than slots)
SAMPLE_CASES = [("syn_24_16", m) for m in sorted(SAMPLE_MODES)] + [("7CEI", m) for m in ("plain", "fp32", "f16", "clash_force", "graph")]


@pytest.mark.parametrize("case,mode", SAMPLE_CASES)
def test_sample(complexes, case, mode):
    """B = 5, three steps, tr_draw[2] = NaN: trajectory 2 is non-finite from its first pose on."""
    gx, cx = complexes[case]
    kw = dict(SAMPLE_MODES[mode], seed=5)
    if mode not in ("fp32_no_table", "fp32", "f16"):
        kw.update(mfma16=True)
    if mode == "restraints":
        from dfmdock_amd.restraints import native_contact_groups
        gx.set_restraints(native_contact_groups(cx["rec_pos"], cx["lig_pos"], 5, cutoff=8.0, seed=0))
    try:
        nan, good = traj_inject(5, 3, 2, np.nan)
        check_traj(gx.sample(B=5, num_steps=3, inject=nan, **kw), gx.sample(B=5, num_steps=3, inject=good, **kw), 2)
    finally:
        if mode == "restraints":
            gx.set_restraints([])


def test_sample_symmetry(model):
    from dfmdock_amd import engine
    from dfmdock_amd.synthetic import make_complex
    cx = make_complex(20, 20, seed=9)
    gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    gx.set_symmetry(3)
    nan, good = traj_inject(5, 3, 2, np.nan)
    kw = dict(seed=5, mfma16=True, symmetry=True)
    check_traj(gx.sample(B=5, num_steps=3, inject=nan, **kw), gx.sample(B=5, num_steps=3, inject=good, **kw), 2)
    gx.close()


@pytest.mark.parametrize("case", ("syn_24_16", "7CEI"))
def test_refine(complexes, case):
    gx, cx = complexes[case]
    start = np.repeat(np.asarray(cx["lig_pos"], np.float32)[None], 3, 0)
    bad = start.copy()
    bad[1, 3, 1, 0] = np.nan
    kw = dict(B=3, num_steps=3, t_begin=0.2, seed=7, mfma16=True)
    check_traj(gx.refine(start_pos=bad, **kw), gx.refine(start_pos=start, **kw), 1)


@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf), ids=("nan", "inf", "neg_inf"))
def test_stored_pose_is_refused(model, value):
    """dfm_complex_create and dfm_complex_set_pose: DFM_E_INVALID (ValueError) for a non-finite rec_pos / lig_pos; set_pose keeps BOTH
    stored poses - also the finite one given in the same call - and a following score returns the bits it returned before."""
    from dfmdock_amd import _lib, engine
    cx = complex_for("syn_24_16")
    for side in ("rec_pos", "lig_pos"):
        p = {k: np.array(cx[k], np.float32) for k in ("rec_pos", "lig_pos")}
        p[side][-1, 2, 2] = value
        with pytest.raises(_lib.DfmError, match=side + ": residue .* is not finite"):
            engine.Complex(model, cx["rec_x"], cx["lig_x"], p["rec_pos"], p["lig_pos"])
    gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    kw = dict(seed=3, energy=True, l0_table=True, mfma16=True)
    before = gx.score(cx["lig_pos"], 0.5, **kw)
    s0 = gx.sample(B=2, num_steps=2, seed=1, mfma16=True)
    moved = np.array(cx["lig_pos"], np.float32) + np.float32(3.0)
    for side in ("rec_pos", "lig_pos"):
        p = dict(rec_pos=np.array(cx["rec_pos"], np.float32) + np.float32(1.0), lig_pos=moved.copy())
        p[side][0, 0, 0] = value
        with pytest.raises(ValueError, match="is not finite"):
            gx.set_pose(**p)
        assert _lib.lib().dfm_complex_set_pose(gx._h, p["rec_pos"].ctypes.data_as(_lib.F32P), p["lig_pos"].ctypes.data_as(_lib.F32P)) == -1
    after = gx.score(cx["lig_pos"], 0.5, **kw)
    s1 = gx.sample(B=2, num_steps=2, seed=1, mfma16=True)
    for k in FLOATS + ("num_clashes",):
        assert np.array_equal(bits(before[k]), bits(after[k])), k
    assert np.array_equal(bits(s0["lig_pos"]), bits(s1["lig_pos"])), "the stored ligand pose (the sampler's start) changed"
    gx.close()
