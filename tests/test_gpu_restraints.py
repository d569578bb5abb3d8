"""Interface distance restraints on the GPU (DFM_F_RESTRAINTS, dfm_complex_set_restraints, dfm_restraint_eval) against the float64
numpy definition in dfmdock_amd/restraints.py, and what they do to a docking run.

Gates: satisfied counts exact, energy and step within the derived bound of tests/test_gpu_aux_kernels.py (one fp32 rounding plus a few
float64 roundings of the sums; the definition evaluated on the fp32 bounds, weights and parameters the kernel is given) (evaluation);
<= 1e-3 A per atom for a sampler step replayed on the host from the traced pose, scores and injected noise; bitwise for the flag without
a set, the captured graph and batch invariance.
"""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, complex_for, draw_blob, draw_hparams, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


def _complex(model, case):
    from dfmdock_amd import engine
    cx = complex_for(case)
    return engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"]), cx


def _random_groups(R, L, rng, G=48):
    """Groups of 1 ... 64 pairs: single pairs, ambiguous patches, exact ties (a pair listed twice), zero weights, groups every pose
    satisfies (u = 500 A) and groups large enough for the kernel's one-wave-per-group path (> 16 pairs)."""
    from dfmdock_amd.restraints import RestraintGroup
    out = []
    for g in range(G):
        n = [1, 1, 2, 5, 16, 17, 40, 64][g % 8]
        pairs = [(int(rng.integers(R)), int(rng.integers(L))) for _ in range(n)]
        if g % 5 == 1 and n > 1:
            pairs[-1] = pairs[0]                                  # exact tie: the first of the two is the arg-min
        upper = 500.0 if g % 7 == 3 else float(rng.uniform(4.0, 12.0))
        weight = 0.0 if g % 6 == 2 else float(rng.uniform(0.2, 3.0))
        out.append(RestraintGroup(tuple(pairs), upper, weight))
    return out


def _random_poses(lig, B, rng, spread=8.0):
    """B rigid moves of the native ligand: a random rotation about its CA centroid and an N(0, spread^2) shift."""
    from dfmdock_amd.restraints import axis_angle_to_matrix
    lig = np.asarray(lig, np.float64)
    c = lig[:, 1].mean(0)
    out = np.empty((B,) + lig.shape, np.float32)
    for b in range(B):
        aa = rng.standard_normal(3)
        aa *= rng.uniform(0, np.pi) / np.linalg.norm(aa)
        out[b] = (lig - c) @ axis_angle_to_matrix(aa).T + c + spread * rng.standard_normal(3)
    return out


def _check_eval(ev, groups, rec_pos, poses, params, all_atoms=0):
    """dfm_restraint_eval of every pose against restraints.evaluate on the kernel's own fp32 inputs, under aux_harness.restraint_ref's
    bound (it was 1e-5 relative on the energy and 1e-4 on the step).  Returns the clip decisions [B][2]."""
    import aux_harness as ah
    from dfmdock_amd.restraints import RestraintGroup
    f32 = np.float32
    g32 = [RestraintGroup(g.pairs, float(f32(g.upper)), float(f32(g.weight))) for g in groups]
    B = len(poses)
    rec = np.asarray(rec_pos, f32).reshape(-1, 9)
    c = dict(groups=g32, rec_pos=rec, lig=np.asarray(poses, f32).reshape(B, -1, 9), R=len(rec), L=np.asarray(poses).reshape(B, -1, 9).shape[1], B=B,
             all_atoms=all_atoms, params={k: float(f32(getattr(params, k))) for k in ("k_tr", "k_rot", "max_tr", "max_rot", "t_start")})
    c.update(ah.pack_groups(g32, c["R"], c["L"]))
    clipped = []
    for b in range(B):
        e = ah.restraint_ref(c, b)
        assert e["decided"].all(), (b, e["norm"], e["limit"])
        assert int(ev["n_satisfied"][b]) == e["n_satisfied"], b
        assert abs(float(ev["energy"][b]) - e["energy"]) <= e["b_energy"], (b, ev["energy"][b], e["energy"], e["b_energy"])
        assert (np.abs(ev["step"][b] - e["step"]) <= e["b_step"]).all(), (b, ev["step"][b], e["step"], e["b_step"])
        clipped.append(e["clipped"])
    return np.array(clipped)


def _native_groups(cx, k=5, seed=0):
    from dfmdock_amd.restraints import native_contact_groups
    return native_contact_groups(cx["rec_pos"], cx["lig_pos"], k, cutoff=8.0, seed=seed)


@pytest.mark.parametrize("case", ["rollout_7CEI", "c3_300_300"])
def test_restraint_eval_vs_numpy(case, model):
    from dfmdock_amd import restraints as RS
    gx, cx = _complex(model, case)
    rng = np.random.default_rng(3)
    groups = _random_groups(gx.R, gx.L, rng)
    poses = _random_poses(cx["lig_pos"], 64, rng)
    poses[0] = cx["lig_pos"]                                     # the native pose: many groups satisfied
    # the default parameters clip every step of these far-off poses; tiny gains clip none
    for params, clipped in ((RS.RestraintParams(), True), (RS.RestraintParams(k_tr=1e-5, k_rot=1e-7), False)):
        gx.set_restraints(groups, params)
        r = gx.restraint_eval(poses)
        assert (_check_eval(r, groups, cx["rec_pos"], poses, params)[:, 0] == clipped).all()
        assert 0 < r["n_satisfied"].min() < len(groups)
    # an empty set evaluates to zeros
    gx.set_restraints([])
    z = gx.restraint_eval(poses[:3])
    assert not z["energy"].any() and not z["n_satisfied"].any() and not z["step"].any()
    gx.close()


def test_set_restraints_validates(model):
    from dfmdock_amd import _lib as L
    from dfmdock_amd.restraints import RestraintGroup
    import ctypes as C
    gx, _ = _complex(model, "rollout_7CEI")
    for bad in ([RestraintGroup(((gx.R, 0),), 8.0)], [RestraintGroup(((0, gx.L),), 8.0)], [RestraintGroup(((0, 0),), 0.0)],
                [RestraintGroup(((0, 0),), 8.0, -1.0)], [RestraintGroup((), 8.0)]):
        with pytest.raises(ValueError):
            gx.set_restraints(bad)
    # the C entry point checks on its own (the Python packing above refuses first)
    gs, pairs, up, w = (np.array([0, 1], np.int32), np.array([[gx.R, 0]], np.int32), np.ones(1, np.float32) * 8, np.ones(1, np.float32))
    rc = L.lib().dfm_complex_set_restraints(gx._h, 1, gs.ctypes.data_as(L.I32P), pairs.ctypes.data_as(L.I32P), up.ctypes.data_as(L.F32P),
                                            w.ctypes.data_as(L.F32P), None)
    assert rc == -1 and b"outside" in L.lib().dfm_last_error()
    gs = np.array([0, 0], np.int32)
    rc = L.lib().dfm_complex_set_restraints(gx._h, 1, gs.ctypes.data_as(L.I32P), pairs.ctypes.data_as(L.I32P), up.ctypes.data_as(L.F32P),
                                            w.ctypes.data_as(L.F32P), None)
    assert rc == -1 and b"empty" in L.lib().dfm_last_error()
    # the documented limits are accepted: 4096 groups, 65536 pairs
    rng = np.random.default_rng(0)
    big = [RestraintGroup(tuple((int(rng.integers(gx.R)), int(rng.integers(gx.L))) for _ in range(16)), 8.0) for _ in range(4096)]
    gx.set_restraints(big)
    r = gx.restraint_eval(complex_for("rollout_7CEI")["lig_pos"])
    assert np.isfinite(r["energy"]).all()
    with pytest.raises(ValueError):
        gx.set_restraints(big + big[:1])
    gx.close()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "mfma16", "f16"])
def test_flag_without_set_is_bitwise_unflagged(prec, graph, model):
    from dfmdock_amd import engine
    gx, _ = _complex(model, "rollout_7CEI")
    kw = dict(B=4, num_steps=6, seed=3, graph=graph, **engine.precision_kwargs(prec))
    a = gx.sample(**kw)
    b = gx.sample(restraints=True, **kw)
    gx.set_restraints(_native_groups(complex_for("rollout_7CEI")))
    gx.set_restraints(None)                                        # cleared again
    c = gx.sample(restraints=True, **kw)
    for k in ("lig_pos", "rot_update", "tr_update", "energy", "num_clashes", "final_scores"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    gx.close()


def _em_host(pose, scores, z_rot, z_tr, t, dt, noise, hp=None):
    """The Euler-Maruyama step of inference_base.py:439-456 in float64 from the traced scores and the injected noise."""
    from dfmdock_amd import engine
    from dfmdock_amd.restraints import axis_angle_to_matrix
    g_r, _ = engine.diffusion_coef(1, t, hp)
    g_t, _ = engine.diffusion_coef(0, t, hp)
    rot = g_r ** 2 * scores[3:6] * dt + g_r * np.sqrt(dt) * (noise * z_rot)
    tr = g_t ** 2 * scores[0:3] * dt + g_t * np.sqrt(dt) * (noise * z_tr)
    pose = np.asarray(pose, np.float64)
    c = pose[:, 1].mean(0)
    return (pose - c) @ axis_angle_to_matrix(rot).T + c + tr


@pytest.mark.parametrize("prec", ["fp32", "mfma16"])
def test_step_replay_on_host(prec, model):
    from dfmdock_amd import engine
    from dfmdock_amd import restraints as RS
    g = load_golden("rollout_7CEI.npz")
    gx, cx = _complex(model, "rollout_7CEI")
    groups = _native_groups(cx)
    gx.set_restraints(groups)
    S = 6
    inj = dict(R0=g["R0"].astype(np.float32), tr_draw=g["tr_draw"], z_rot=g["z_rot"], z_tr=g["z_tr"], edges=g["edges"])
    r = gx.sample(B=1, num_steps=S, inject=inj, trace=True, restraints=True, **engine.precision_kwargs(prec))
    plain = gx.sample(B=1, num_steps=S, inject=inj, trace=True, **engine.precision_kwargs(prec))
    assert np.abs(plain["trace_pose"][0, 0] - r["trace_pose"][0, 0]).max() > 0.5      # the restraint step moved the first pose
    eps = 1e-3
    step = (eps - 1.0) / (S - 1)
    ts = np.array([np.float32(1.0 + np.float32(step) * np.float32(i)) if i < S // 2 else
                   np.float32(eps - np.float32(step) * np.float32(S - 1 - i)) for i in range(S)], np.float32)
    dt = float(np.float32(ts[0] - ts[1]))
    worst = 0.0
    for i in range(S):
        prev = r["init_pose"][0] if i == 0 else r["trace_pose"][0, i - 1]
        em = _em_host(prev, r["trace_scores"][0, i].astype(np.float64), g["z_rot"][i], g["z_tr"][i], float(ts[i]), dt,
                      0.0 if i == S - 1 else 0.5)
        st = RS.evaluate(groups, cx["rec_pos"], em)["step"]
        want, _, _ = RS.apply_step(em, st)
        worst = max(worst, float(np.abs(want - r["trace_pose"][0, i]).max()))
    assert worst <= 1e-3, worst
    np.testing.assert_array_equal(r["trace_pose"][0, -1], r["lig_pos"][0])
    # the bookkeeping still describes the final pose (dock_pair's output.pdb): the complex's start pose moved by (rot_update, tr_update)
    again = RS.replay_pose(cx["lig_pos"], r["rot_update"][0], r["tr_update"][0])
    assert np.abs(again - r["lig_pos"][0]).max() <= 1e-3
    gx.close()


def test_graph_with_restraints_is_bitwise_plain(model):
    from dfmdock_amd import restraints as RS
    gx, cx = _complex(model, "rollout_7CEI")
    kw = dict(B=6, num_steps=8, seed=11, mfma16=True)
    a_groups = _native_groups(cx, 5, seed=0)
    b_groups = _native_groups(cx, 3, seed=1) + _random_groups(gx.R, gx.L, np.random.default_rng(1), G=8)
    gx.set_restraints(a_groups)
    pa, ga = gx.sample(restraints=True, **kw), gx.sample(restraints=True, graph=True, **kw)
    ga2 = gx.sample(restraints=True, graph=True, **kw)                         # replayed graph
    gx.set_restraints(b_groups)
    gb = gx.sample(restraints=True, graph=True, **kw)                          # a new set between two graph calls
    pb = gx.sample(restraints=True, **kw)
    gx.set_restraints(b_groups, RS.RestraintParams(t_start=0.5))               # new parameters: the step from t <= 0.5 on only
    gc, pc = gx.sample(restraints=True, graph=True, **kw), gx.sample(restraints=True, **kw)
    none = gx.sample(**kw)
    for k in ("lig_pos", "rot_update", "tr_update", "energy"):
        np.testing.assert_array_equal(pa[k], ga[k], err_msg=k)
        np.testing.assert_array_equal(pa[k], ga2[k], err_msg=k)
        np.testing.assert_array_equal(pb[k], gb[k], err_msg=k)
        np.testing.assert_array_equal(pc[k], gc[k], err_msg=k)
    assert not np.array_equal(pa["lig_pos"], pb["lig_pos"]) and not np.array_equal(pb["lig_pos"], pc["lig_pos"])
    assert not np.array_equal(pc["lig_pos"], none["lig_pos"])
    gx.close()


def test_batch_invariance(model):
    gx, cx = _complex(model, "rollout_7CEI")
    gx.set_restraints(_native_groups(cx) + _random_groups(gx.R, gx.L, np.random.default_rng(5), G=16))
    B, S = 64, 8
    rng = np.random.default_rng(21)
    from dfmdock_amd.restraints import axis_angle_to_matrix
    c1, c2 = cx["rec_pos"][:, 1].mean(0), cx["lig_pos"][:, 1].mean(0)
    R0 = np.stack([axis_angle_to_matrix(0.5 * rng.standard_normal(3)) for _ in range(B)]).reshape(B, 9).astype(np.float32)
    inj = dict(R0=R0, tr_draw=((c2 - c1)[None] + 6.0 * rng.standard_normal((B, 3))).astype(np.float32),
               z_rot=rng.standard_normal((B, S, 3)).astype(np.float32), z_tr=rng.standard_normal((B, S, 3)).astype(np.float32))
    edges = np.empty((B, S + 1, gx.N, gx.K), np.int32)
    for s in range(S + 1):
        poses = (cx["lig_pos"][None] + rng.standard_normal((B, 1, 1, 3)).astype(np.float32)).astype(np.float32)
        edges[:, s] = gx.score(poses, 0.5, seed=900 + s, mfma16=True, energy=False, return_edges=True)["edges"]
    inj["edges"] = edges
    big = gx.sample(B=B, num_steps=S, inject=inj, restraints=True, mfma16=True)
    seven = {k: np.ascontiguousarray(v[30:37]) for k, v in inj.items()}
    mid = gx.sample(B=7, num_steps=S, inject=seven, restraints=True, mfma16=True)
    one = {k: np.ascontiguousarray(v[33:34]) for k, v in inj.items()}
    r1 = gx.sample(B=1, num_steps=S, inject=one, restraints=True, mfma16=True)
    for k in ("lig_pos", "energy", "tr_update", "rot_update"):
        np.testing.assert_array_equal(mid[k], big[k][30:37], err_msg=k)
        np.testing.assert_array_equal(r1[k][0], big[k][33], err_msg=k)
    gx.close()


def _lrmsd(poses, native):
    return np.sqrt(((poses[:, :, 1] - native[None, :, 1]) ** 2).sum(-1).mean(-1))


def test_restraints_steer_7cei_docking(model):
    """5 native CA-CA contacts (< 8 A) as single-pair groups, u = 8 A, default parameters, B = 128, 40 steps, seed 0, native RNG,
    against the same call without restraints."""
    gx, cx = _complex(model, "rollout_7CEI")
    groups = _native_groups(cx, 5, seed=0)
    assert len(groups) == 5
    gx.set_restraints(groups)
    free = gx.sample(B=128, num_steps=40, seed=0, mfma16=True)
    guided = gx.sample(B=128, num_steps=40, seed=0, mfma16=True, restraints=True)
    ev = gx.restraint_eval(guided["lig_pos"])
    ev0 = gx.restraint_eval(free["lig_pos"])
    all_sat = float((ev["n_satisfied"] == 5).mean())
    med_g, med_f = float(np.median(_lrmsd(guided["lig_pos"], cx["lig_pos"]))), float(np.median(_lrmsd(free["lig_pos"], cx["lig_pos"])))
    rec = {"all_satisfied_guided": all_sat, "all_satisfied_free": float((ev0["n_satisfied"] == 5).mean()),
           "median_lrmsd_guided": med_g, "median_lrmsd_free": med_f, "mean_satisfied_guided": float(ev["n_satisfied"].mean())}
    print("restraints 7CEI:", json.dumps(rec))
    assert np.isfinite(guided["lig_pos"]).all()
    # first GPU run at the shipped defaults: 73 % of the trajectories satisfy all five groups (0 % without restraints), median l-RMSD
    # 29.3 A against 71.4 A (the seeded weights push free ligands away from the receptor)
    assert all_sat >= 0.5, rec
    assert med_g < 0.6 * med_f, rec
    gx.close()


def test_second_family_restrained_sample():
    from dfmdock_amd import engine
    from dfmdock_amd import restraints as RS
    hp = draw_hparams(1)
    m = engine.Model(draw_blob(1, "s1"), hp)
    cx = complex_for("rollout_7CEI")
    gx = engine.Complex(m, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    groups = _native_groups(cx, 5) + _random_groups(gx.R, gx.L, np.random.default_rng(9), G=8)
    gx.set_restraints(groups)
    r = gx.sample(B=16, num_steps=12, seed=2, mfma16=True, restraints=True)
    assert np.isfinite(r["lig_pos"]).all() and np.isfinite(r["energy"]).all()
    ev = gx.restraint_eval(r["lig_pos"])
    _check_eval(ev, groups, cx["rec_pos"], r["lig_pos"], RS.RestraintParams(), all_atoms=1)
    # the bookkeeping of the second family (rotation about the all-atom centroid) still describes the final pose
    for b in range(4):
        again = RS.replay_pose(cx["lig_pos"], r["rot_update"][b], r["tr_update"][b], center="all_atoms")
        assert np.abs(again - r["lig_pos"][b]).max() <= 1e-3
    gx.close(); m.close()


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def test_cli_dock_and_sweep_with_restraints(tmp_path):
    from cli_fixtures import golden_7cei, write_ckpt, write_db5_pt, write_pair
    from dfmdock_amd import pdbio, restraints as RS
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    rec = pdbio.backbone_from_atoms(pdbio.read_pdb(rec_pdb))
    lig = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))
    name = lambda k: f"{k[0]}:{k[1]}{k[2].strip()}"
    lines = ["# native contacts of 7CEI"]
    for grp in RS.native_contact_groups(rec["bb_coords"], lig["bb_coords"], 4, seed=0):
        (i, j), = grp.pairs
        lines.append(f"{name(rec['residues'][i])}  {name(lig['residues'][j])}  8.0")
    k0 = lig["residues"][0]
    lines.append(f"{name(rec['residues'][0])},{name(rec['residues'][1])}  {name(k0)}-{name(lig['residues'][5])}  10.0 0.5   # ambiguous")
    (tmp_path / "r.txt").write_text("\n".join(lines) + "\n")
    p = _run(["dock", rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--num-samples", "12", "--max-batch", "6", "--seed", "5",
              "--restraints", str(tmp_path / "r.txt"), "--json", str(tmp_path / "res.json")], cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert (tmp_path / "output.pdb").exists()
    assert line["restraints"] == 5 and 0 <= line["restraints_satisfied"] <= 5 and line["restraint_rank"] == "satisfied"
    tr = json.load(open(tmp_path / "res.json"))["trajectories"]
    assert len(tr["energy"]) == 12
    assert line["index"] == RS.rank_key(np.float32(tr["energy"]), np.int32(tr["restraints_satisfied"]))
    assert line["restraints_satisfied"] == max(tr["restraints_satisfied"])
    assert line["energy"] == pytest.approx(tr["energy"][line["index"]], abs=1e-6)
    # sweep with native restraints: the extra CSV columns
    d = tmp_path / "db5"
    d.mkdir()
    write_db5_pt(str(d / "7CEI.pt"), "7CEI", cx, rs, ls)
    write_db5_pt(str(d / "SYN1.pt"), "SYN1", complex_for("fwd_syn_24_16"), "A" * 24, "G" * 16)
    (d / "test.txt").write_text("7CEI\nSYN1\n")
    q = _run(["sweep", "--db5", str(d), "--ckpt", ck, "--num-samples", "4", "--num-steps", "8", "--out-csv", str(tmp_path / "r.csv"),
              "--native-restraints", "3", "--limit", "2", "--summary", str(tmp_path / "s.json")], cwd=str(tmp_path))
    assert q.returncode == 0, q.stdout + q.stderr
    rows = list(csv.DictReader(open(tmp_path / "r.csv")))
    assert len(rows) == 8 and "restraints_satisfied" in rows[0] and "restraint_energy" in rows[0]
    assert all(0 <= int(r["restraints_satisfied"]) <= 3 for r in rows)
    summ = json.load(open(tmp_path / "s.json"))["restraints"]
    assert summ["7CEI"]["groups"] == 3
