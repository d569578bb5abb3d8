"""The distogram head reduced on the GPU (Complex.distogram, dfm_score_distogram, kernels_pair.hip: k_pair_dist_sum) against its
float64 definition (dfmdock_amd/distogram.py) on the committed second-family fixtures, which hit every tile edge of the kernel
(workgroup = 32 receptor residues x a 64-residue ligand chunk, 16 ligand residues per wave):

    fwd2_syn_9_7           9 x 7     less than one tile, L not a multiple of 4
    fwd2_syn_24_16        24 x 16
    fwd2_syn_64_48_p0..2  64 x 48    exactly two row tiles, a partial chunk, t = 1 ... 0.001
    fwd2_7CEI_p0 / p1     87 x 127   R = 2 32 + 23, L = 64 + 63

(a) against the REFERENCE's logits (fwd2_dist.npz: syn_24_16 whole, 7CEI pose 1 on its stride-8 grid).  Derived bound: logits that differ
    by eps in the max norm move every log-probability by at most 2 eps; the project's gates on these logits (test_gpu_pair_family.py) are
    eps = 1e-4 max|z| for the fp32 engine and 1e-2 max|z| for the 16-bit engines, so |d nll|, |d pair_nll| <= 2 eps, |d pcontact| <=
    2.1 eps pcontact, |d edist| <= 2.1 eps 51.
(b) against the definition applied to the dist_logits `score(dist=True)` returns for the same inputs and engine.  What separates the two
    is k_pair_head_m's arithmetic (LayerNorm statistics from moments, rsq, exp2 / rcp SiLU, fp32 softmax): measured, not derivable.
    Largest deviations over the seven cases x three engines on an MI355X (profiles/distogram.txt), gates at four times that:
        pair_nll 1.95e-6   nll 3.4e-7   nll_near 4.2e-7   pcontact 7.95e-7 relative   edist 1.18e-5 A   exp_contacts 5.1e-8 relative
(c) pair_nll depends on the integer bin of D, and the engine centres the pose in fp32: pairs whose float64 d^2 lies within a relative
    1e-5 of some bounds^2 are left out of the per-pair comparison (at most 0.5 % of a case's pairs; the fixtures have 0 - 3 such pairs,
    closest approach 1.4e-6 on syn_64_48_p1).  Per-pose nll is compared with every pair in.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alloc_recipe as ar
from conftest import ROOT, complex_for, load_golden, pair_hparams

pytestmark = pytest.mark.gpu

CASES = ["fwd2_syn_9_7", "fwd2_syn_24_16", "fwd2_syn_64_48_p0", "fwd2_syn_64_48_p1", "fwd2_syn_64_48_p2", "fwd2_7CEI_p0", "fwd2_7CEI_p1"]
ENGINES = {"fp32": {}, "mfma16": dict(mfma16=True), "f16": dict(f16=True)}
MAPS = ("pair_nll", "pcontact", "edist", "pcontact_mean")
POSE_KEYS = ("nll", "nll_near", "n_near", "exp_contacts")
REF_EPS = {"fp32": 1e-4, "mfma16": 1e-2, "f16": 1e-2}      # x max|z|: the gates of test_pair_family_dist_logits_vs_reference
# (b): 4 x the largest deviation measured on an MI355X (module docstring, profiles/distogram.txt)
GATE_PAIR_NLL = 4 * 1.95e-6
GATE_NLL = 4 * 3.4e-7
GATE_NLL_NEAR = 4 * 4.2e-7
GATE_PCONTACT_REL = 4 * 7.95e-7
GATE_EDIST = 4 * 1.18e-5
GATE_EXP_CONTACTS_REL = 4 * 5.1e-8
BIN_MARGIN = 1e-5

_state = {}


def gpu_complex(case, blob_pair):
    from dfmdock_amd import engine
    if "model" not in _state:
        engine.set_device(0)
        _state["model"] = engine.Model(blob_pair, pair_hparams())
    key = next(k for k in ("7CEI", "syn_24_16", "syn_9_7", "syn_64_48") if k in case)
    if key not in _state:
        cx = complex_for(case)
        _state[key] = (engine.Complex(_state["model"], cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"]), cx)
    return _state[key]


def evaluated(case, prec, blob_pair):
    """One distogram call with every map, one score(dist=True) call and the float64 distances of `case` on engine `prec`: computed once."""
    from dfmdock_amd import distogram as DG
    if (case, prec) not in _state:
        gx, cx = gpu_complex(case, blob_pair)
        g = load_golden(case + ".npz")
        d = gx.distogram(g["lig_pos"], float(g["t"]), edges=g["edges"], maps=MAPS, **ENGINES[prec])
        z = gx.score(g["lig_pos"], float(g["t"]), edges=g["edges"], energy=True, dist=True, **ENGINES[prec])["dist_logits"][0]
        D = DG.ca_distances(cx["rec_pos"], g["lig_pos"])
        keep = np.abs((D ** 2)[..., None] / DG.BOUNDS ** 2 - 1).min(-1) > BIN_MARGIN
        assert (~keep).sum() <= 0.005 * keep.size, (case, int((~keep).sum()))
        _state[(case, prec)] = (d, z, D, keep)
    return _state[(case, prec)]


@pytest.mark.parametrize("prec", list(ENGINES))
@pytest.mark.parametrize("case,key,stride", [("fwd2_syn_24_16", "syn_24_16", 1), ("fwd2_7CEI_p1", "cei_p1_stride8", 8)])
def test_against_the_reference_logits(case, key, stride, prec, blob_pair):
    from dfmdock_amd import distogram as DG
    d, _, D, keep = evaluated(case, prec, blob_pair)
    zr = load_golden("fwd2_dist.npz")[key]
    eps = REF_EPS[prec] * float(np.abs(zr).max())
    sl = (slice(None, None, stride), slice(None, None, stride))
    e = DG.pose_scores(zr, D[sl], 7, pair_hparams().cut_off)
    k = keep[sl]
    dev = {"pair_nll": np.abs(d["pair_nll"][0][sl] - e["pair_nll"])[k].max(),
           "pcontact": (np.abs(d["pcontact"][0][sl] - e["pcontact"]) / e["pcontact"]).max(),
           "edist": np.abs(d["edist"][0][sl] - e["edist"]).max()}
    print(case, prec, "eps", eps, dev)
    assert dev["pair_nll"] <= 2 * eps
    assert dev["pcontact"] <= 2.1 * eps
    assert dev["edist"] <= 2.1 * eps * 51
    if stride == 1:      # the whole tensor is committed: the per-pose mean, every pair in
        print("nll", float(d["nll"][0]), e["nll"])
        assert abs(float(d["nll"][0]) - e["nll"]) <= 2 * eps


@pytest.mark.parametrize("prec", list(ENGINES))
@pytest.mark.parametrize("case", CASES)
def test_same_call_consistency(case, prec, blob_pair):
    from dfmdock_amd import distogram as DG
    d, z, D, keep = evaluated(case, prec, blob_pair)
    cut = pair_hparams().cut_off
    e = DG.pose_scores(z, D, 7, cut)
    dev = {"pair_nll": float(np.abs(d["pair_nll"][0] - e["pair_nll"])[keep].max()), "nll": abs(float(d["nll"][0]) - e["nll"]),
           "pcontact": float((np.abs(d["pcontact"][0] - e["pcontact"]) / e["pcontact"]).max()),
           "edist": float(np.abs(d["edist"][0] - e["edist"]).max()),
           "exp_contacts": abs(float(d["exp_contacts"][0]) - e["exp_contacts"]) / e["exp_contacts"]}
    print(case, prec, json.dumps(dev), "dropped", int((~keep).sum()), "of", keep.size)
    eps = REF_EPS[prec] * float(np.abs(z).max())      # never looser than (a)
    assert dev["pair_nll"] <= min(GATE_PAIR_NLL, 2 * eps)
    assert dev["nll"] <= min(GATE_NLL, 2 * eps)
    assert dev["pcontact"] <= min(GATE_PCONTACT_REL, 2.1 * eps)
    assert dev["edist"] <= min(GATE_EDIST, 2.1 * eps * 51)
    assert dev["exp_contacts"] <= min(GATE_EXP_CONTACTS_REL, 2.1 * eps)
    # the near set is decided by the fp32 D of the engine: exact wherever no pair sits on the cut-off itself
    edge = int((np.abs(D / cut - 1) <= 1e-6).sum())
    assert abs(int(d["n_near"][0]) - e["n_near"]) <= edge
    if edge == 0 and e["n_near"]:
        assert abs(float(d["nll_near"][0]) - e["nll_near"]) <= min(GATE_NLL_NEAR, 2 * eps)
    np.testing.assert_array_equal(d["pcontact_mean"], d["pcontact"][0])      # B = 1: the mean is the pose's map
    assert all(np.isfinite(d[k]).all() for k in MAPS + POSE_KEYS)


@pytest.mark.parametrize("case", ["fwd2_syn_9_7", "fwd2_7CEI_p1"])
def test_invariance_is_bitwise(case, blob_pair):
    gx, _ = gpu_complex(case, blob_pair)
    g = load_golden(case + ".npz")
    t, B = float(g["t"]), 5
    one, _, _, _ = evaluated(case, "fp32", blob_pair)
    rng = np.random.default_rng(1)
    poses = np.stack([g["lig_pos"]] + [g["lig_pos"] + rng.normal(0, 2.0, 3).astype(np.float32) for _ in range(B - 1)])
    poses[1] = g["lig_pos"]      # the same pose at positions 0 and 1
    ed = np.stack([g["edges"]] * B)
    five = gx.distogram(poses, t, edges=ed, maps=MAPS)
    bare = gx.distogram(poses, t, edges=ed)
    for k in POSE_KEYS + MAPS[:3]:
        np.testing.assert_array_equal(five[k][0], five[k][1], err_msg=k)      # position in the batch
        np.testing.assert_array_equal(five[k][0], one[k][0], err_msg=k)       # B = 5 against B = 1
    for k in POSE_KEYS:
        np.testing.assert_array_equal(five[k], bare[k], err_msg=k)            # with and without the optional maps
    assert sorted(bare) == sorted(POSE_KEYS)
    same = gx.distogram(np.stack([g["lig_pos"]] * 3), t, edges=ed[:3], maps=("pcontact", "pcontact_mean"))
    np.testing.assert_array_equal(same["pcontact_mean"], same["pcontact"][0])      # B copies of one pose
    from dfmdock_amd import distogram as DG
    np.testing.assert_allclose(five["pcontact_mean"], DG.pcontact_mean(five["pcontact"]), rtol=6e-8, atol=0)      # the double sum, rounded once


def test_arguments(blob_pair, blob):
    from dfmdock_amd import distogram as DG
    from dfmdock_amd import engine
    case = "fwd2_syn_24_16"
    gx, cx = gpu_complex(case, blob_pair)
    g = load_golden(case + ".npz")
    t = float(g["t"])
    gx0 = engine.Complex(engine.Model(blob), cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    with pytest.raises(ValueError, match="family-1"):
        gx0.distogram(g["lig_pos"], t)
    gx0.close()
    for bad in (0, 64, -3):
        with pytest.raises(ValueError, match="contact_bins"):
            gx.distogram(g["lig_pos"], t, edges=g["edges"], contact_bins=bad)
    with pytest.raises(ValueError):
        gx.distogram(g["lig_pos"], t, edges=g["edges"], maps=("logits",))
    # contact_bins = 63: everything but the last bin
    d, z, D, _ = evaluated(case, "fp32", blob_pair)
    r = gx.distogram(g["lig_pos"], t, edges=g["edges"], maps=("pcontact",), contact_bins=63)
    eps = REF_EPS["fp32"] * float(np.abs(z).max())
    last = np.exp(DG.log_softmax(z))[..., 63]
    assert np.abs((1.0 - r["pcontact"][0].astype(np.float64)) - last).max() <= 2.1 * eps * last.max()
    for k in ("nll", "nll_near", "n_near"):      # the contact threshold moves nothing else
        np.testing.assert_array_equal(r[k], d[k])
    # near_cutoff: explicit = the model's cut-off by default; a tiny one empties the near set
    np.testing.assert_array_equal(gx.distogram(g["lig_pos"], t, edges=g["edges"], near_cutoff=pair_hparams().cut_off)["nll_near"], d["nll_near"])
    r = gx.distogram(g["lig_pos"], t, edges=g["edges"], near_cutoff=0.5)
    assert int(r["n_near"][0]) == 0 and np.isnan(r["nll_near"][0]) and np.isfinite(r["nll"][0])
    # a NaN coordinate poisons its own trajectory only
    poses = np.stack([g["lig_pos"]] * 3)
    poses[1, 3, 1, 0] = np.nan
    r = gx.distogram(poses, t, edges=np.stack([g["edges"]] * 3), maps=("pcontact",))
    assert np.isnan(r["nll"][1]) and np.isnan(r["nll_near"][1]) and np.isnan(r["exp_contacts"][1])
    for b in (0, 2):
        for k in POSE_KEYS + ("pcontact",):
            np.testing.assert_array_equal(r[k][b], d[k][0], err_msg=k)


def test_reference_shaped_adapter(blob_pair):
    import torch
    from dfmdock_amd.score_model import DFMDock
    g = load_golden("fwd2_syn_24_16.npz")
    cx = complex_for("syn_24_16")
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cx.items()}
    batch["t"] = torch.tensor([float(g["t"])])
    out = DFMDock(blob_pair, precision="fp32", with_distogram=True)(batch)
    assert {"dist_nll", "dist_nll_near", "dist_n_near", "exp_contacts"} <= set(out) and "dist_nll" not in DFMDock(blob_pair, precision="fp32")(batch)
    assert abs(float(out["dist_nll"]) - 4.3629) < 0.05 and float(out["exp_contacts"]) > 0      # own graph draw: the golden's value up to sampling spread


ALLOC_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import alloc_recipe as ar
from dfmdock_amd import engine
from dfmdock_amd.weights import HParams, make_random_weights, pack_blob
hp = HParams(family=1, mask_dist=20.0)
engine.set_device(0)
model = engine.Model(pack_blob(make_random_weights(0, hp), hp), hp)
cx = ar.complex_7cei()
gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
res = ar.Results()
poses = ar.moved(cx["lig_pos"], 3, seed=4)
maps = ("pair_nll", "pcontact", "edist", "pcontact_mean")
res.put("first", gx.distogram(poses, 0.3, seed=2, maps=maps))
gx.distogram(ar.moved(cx["lig_pos"], 7, seed=5), 0.9, seed=3, mfma16=True, maps=maps[:1])      # grows and dirties the workspace
res.put("small", gx.distogram(poses[:1], 0.3, seed=2))
second = ar.Results(); second.put("first", gx.distogram(poses, 0.3, seed=2, maps=maps))
differs = ar.compare({k: v for k, v in res.items() if k.startswith("first")}, second)
gx.close(); model.close()
engine.trim_cache()      # every block released, both of its bands checked
diag = engine.alloc_diag()
np.savez(sys.argv[2], __pass2_differs=np.array(differs, dtype="U64"), __diag=np.array([diag[k] for k in ar.DIAG], np.int64), **res)
"""


def test_under_poison_fills_and_guard_bands(tmp_path):
    """The call once under the allocator regime of tests/alloc_recipe.py (DFM_ALLOC_GUARD=64 + DFM_ALLOC_POISON=90: exact-size blocks
    filled with 0x5A between checked bands) against a child under the default allocator, key by key and bit by bit."""
    script = tmp_path / "child.py"
    script.write_text(ALLOC_CHILD)
    got = {}
    for tag, extra in (("default", {}), ("guard", {"DFM_ALLOC_GUARD": "64", "DFM_ALLOC_POISON": "90"})):
        env = {k: v for k, v in os.environ.items() if not k.startswith("DFM_")}
        env.update(extra)
        out = str(tmp_path / f"{tag}.npz")
        p = subprocess.run([sys.executable, str(script), ROOT, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]
        got[tag] = dict(np.load(out, allow_pickle=False))
        assert got[tag]["__pass2_differs"].tolist() == []
    assert len([k for k in got["guard"] if not k.startswith("__")]) >= 12
    assert ar.compare(got["default"], got["guard"]) == []
    d = dict(zip(ar.DIAG, got["guard"]["__diag"].tolist()))
    assert d["poisoned_bytes"] > 0 and d["bands_checked"] > 0 and d["bands_damaged"] == 0, d


def test_cli_rank_distogram_end_to_end(tmp_path):
    """dock --top-k 3 --distogram --rank distogram --distogram-restraints: the JSON line is sorted by dist_nll, and the restraint file
    it wrote is accepted by a second, guided run."""
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    cx, rs, ls = golden_7cei()
    ckpt = str(tmp_path / "m.ckpt")
    write_ckpt(ckpt, pair_hparams())
    rec, lig, feat = write_pair(str(tmp_path), cx, rs, ls)

    def run(args):
        return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
                              env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    common = [rec, lig, "--ckpt", ckpt, "--features", feat, "--num-samples", "8", "--num-steps", "4", "--no-selfcheck", "--seed", "3"]
    p = run(["dock"] + common + ["--top-k", "3", "--cluster-radius", "1.0", "--distogram", "--rank", "distogram", "--distogram-restraints",
                                 "f.txt", "--restraint-top", "5", "--distogram-map", "m.npz"])
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["dist_rank"] == 1 and line["distogram_restraints_n"] == 5
    nll = [m["dist_nll"] for m in line["models"]]
    assert len(nll) >= 2 and nll == sorted(nll) and nll[0] == line["dist_nll"] and all("exp_contacts" in m and "dist_nll_near" in m for m in line["models"])
    m = np.load(str(tmp_path / "m.npz"))
    assert m["pcontact_mean"].shape == (len(rs), len(ls)) and m["edist"].shape[1:] == (len(rs), len(ls)) and (m["pcontact_mean"] > 0).all()
    assert float(line["dist_nll"]) == pytest.approx(float(m["nll"].min()))
    p2 = run(["dock"] + common + ["--restraints", str(tmp_path / "f.txt")])
    assert p2.returncode == 0, p2.stderr[-3000:]
    assert json.loads(p2.stdout.strip().splitlines()[-1])["restraints"] == 5
