"""Cn symmetric docking on the GPU (DFM_F_SYMMETRY, dfm_complex_set_symmetry, dfm_symmetry_eval; kernels_symmetry.hip: k_symmetry)
against the float64 numpy definition in dfmdock_amd/symmetry.py, and what the symmetry step does to a docking run.

Homodimers are built here: the receptor of an existing case with its features on both sides, the ligand started as the receptor turned
about an axis a few Angstrom outside the chain.

Gates of the evaluation (the definition evaluated on the kernel's own fp32 coordinates and fp32 parameters): order_m exact; theta within
1e-11 rad, axis within 1e-10, screw / axis_point / fit_rmsd / sym_rmsd within 1e-8 A.  Basis: two independent float64 algorithms (SVD
Kabsch, an eigen-solver on Horn's matrix) agree over 3000 such cases within 6e-15 rad, 5e-14, 3e-12 A and 1e-12 A; the gates leave three
to four orders above that for the device's summation order and Jacobi sweeps.  Each component of `step` lies within 2 fp32 ulp, taken at
that 3-vector's largest component, of the step recomputed in float64 from the device's OWN float64 outputs - gain_rot (theta* - theta) u
and -gain_tr s u with the device's theta, axis, screw and order_m, then the clip (symmetry_fixtures.check_eval).  theta, axis and screw
are gated against the definition separately, so this gate is on the step's own arithmetic - gains, clip, the conversion to fp32 - at
every size of step, the rounding-noise step of an exactly symmetric pose included, and every step counts in the recorded worst ulp.
(Against the definition's own step, 2 ulp of a near-zero float64 DIFFERENCE theta* - theta would be no statement at all.)
Sampler: <= 1e-3 A per atom for a step replayed on the host; closure <= 1e-3 A and |theta - theta*| <= 1e-5 rad for final poses; bitwise
for the flag without a stored symmetry, the captured graph and batch invariance.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, complex_for, draw_blob, draw_hparams, load_golden
from symmetry_fixtures import check_eval as _check_eval, closure as _closure, homodimer as _homodimer, poses as _poses

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


@pytest.fixture(scope="module")
def handles(model):
    """One homodimer handle per chain length, shared by the evaluation tests."""
    hs = {}
    yield lambda size: hs.setdefault(size, _homodimer(model, size))
    for gx, _, _ in hs.values():
        gx.close()


@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("size", [9, 24, "7CEI", 300])
def test_symmetry_eval_vs_numpy(size, n, handles):
    from dfmdock_amd import symmetry as SY
    gx, y, _ = handles(size)
    if size == "7CEI":
        assert 3 * len(y) > 256 and (3 * len(y)) % 64
    B = 64
    poses = _poses(y, n, B, np.random.default_rng(100 * n + len(y)))
    params = SY.SymmetryParams()
    gx.set_symmetry(n, params)
    ev = gx.symmetry_eval(poses)
    worst, clipped = _check_eval(ev, y, poses, n, params)
    print("symmetry eval:", json.dumps(dict(worst, M=len(y), n=n)))
    assert clipped[2].any() and not clipped[3].any()
    # the exactly symmetric poses: a step of the coordinates' fp32 rounding only
    sym = [0, 1] if n == 2 else [0]
    assert np.abs(ev["step"][sym]).max() < 1e-4 and ev["sym_rmsd"][sym].max() < 1e-4 and (ev["order_m"][sym] == 1).all()
    assert abs(ev["theta"][1] - np.pi) < 1e-5
    assert np.abs(poses[4] - y).max() > 0
    # the pure translation has no axis: m = 0, theta = 0, a zero step, fit_rmsd as fitted, NaN elsewhere
    assert ev["order_m"][4] == 0 and ev["theta"][4] == 0.0 and not ev["step"][4].any() and 0 <= ev["fit_rmsd"][4] < 1e-5
    assert all(np.isnan(ev[k][4]).all() for k in ("screw", "axis", "axis_point", "sym_rmsd"))
    # the NaN pose is alone: every other pose keeps its bits with a finite pose in its place
    other = poses.copy()
    other[5] = poses[6]
    ev2 = gx.symmetry_eval(other)
    keep = np.arange(B) != 5
    for k in ev:
        np.testing.assert_array_equal(ev[k][keep], ev2[k][keep], err_msg=k)
    # nothing stored: zeros
    gx.set_symmetry(0)
    z = gx.symmetry_eval(poses[:3])
    assert not any(np.asarray(v).any() for v in z.values())


def test_set_symmetry_validates(model):
    import ctypes as C
    from dfmdock_amd import _lib as L, engine
    from dfmdock_amd import symmetry as SY
    gx, y, _ = _homodimer(model, 24)
    gx.set_symmetry(3)
    want = gx.symmetry_eval(gx.lig_pos0)
    for n in (1, -2, 25):
        with pytest.raises(ValueError):
            gx.set_symmetry(n)
    for bad in (dict(gain_rot=0.0), dict(gain_tr=1.5), dict(max_rot=0.0), dict(max_tr=-1.0), dict(gain_rot=float("nan")),
                dict(max_tr=float("inf")), dict(t_start=float("nan"))):
        par = L.SymmetryParamsC(*[bad.get(k, d) for k, d in (("gain_rot", 0.5), ("gain_tr", 0.5), ("max_rot", 0.3), ("max_tr", 10.0),
                                                              ("t_start", 1.0))], 1)
        assert L.lib().dfm_complex_set_symmetry(gx._h, 3, C.byref(par)) == -1, bad
        assert b"symmetry" in L.lib().dfm_last_error()
    got = gx.symmetry_eval(gx.lig_pos0)      # every refused call kept the stored state
    for k in want:
        np.testing.assert_array_equal(want[k], got[k], err_msg=k)
    assert L.lib().dfm_complex_set_symmetry(gx._h, 0, C.byref(par)) == 0      # a clear ignores the parameters, invalid ones too
    assert not gx.symmetry_eval(gx.lig_pos0)["theta"].any()
    gx.set_symmetry(24)
    gx.close()
    cx = complex_for("fwd_syn_24_16")        # R != L
    g2 = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    with pytest.raises(ValueError, match="same chain"):
        g2.set_symmetry(2)
    g2.set_symmetry(0)
    g2.close()


KEYS = ("lig_pos", "rot_update", "tr_update", "energy", "num_clashes", "final_scores")


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "mfma16", "f16"])
def test_flag_without_symmetry_is_bitwise_unflagged(prec, graph, model):
    from dfmdock_amd import engine
    gx, _, _ = _homodimer(model, 24)
    kw = dict(B=4, num_steps=6, seed=3, graph=graph, **engine.precision_kwargs(prec))
    a = gx.sample(**kw)
    b = gx.sample(symmetry=True, **kw)
    gx.set_symmetry(3)
    d = gx.sample(symmetry=True, **kw)
    gx.set_symmetry(0)                                             # cleared again
    c = gx.sample(symmetry=True, **kw)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    assert not np.array_equal(a["lig_pos"], d["lig_pos"])
    gx.close()


def _em_host(pose, scores, z_rot, z_tr, t, dt, noise, center="ca", hp=None):
    """The Euler-Maruyama step of inference_base.py:439-456 in float64 from the traced scores and the injected noise."""
    from dfmdock_amd import engine
    from dfmdock_amd.restraints import _centroid, axis_angle_to_matrix
    g_r, _ = engine.diffusion_coef(1, t, hp)
    g_t, _ = engine.diffusion_coef(0, t, hp)
    rot = g_r ** 2 * scores[3:6] * dt + g_r * np.sqrt(dt) * (noise * z_rot)
    tr = g_t ** 2 * scores[0:3] * dt + g_t * np.sqrt(dt) * (noise * z_tr)
    pose = np.asarray(pose, np.float64)
    c = _centroid(pose, center)
    return (pose - c) @ axis_angle_to_matrix(rot).T + c + tr


def _time_grid(S, eps=1e-3):
    step = (eps - 1.0) / (S - 1)
    ts = np.array([F32(1.0 + F32(step) * F32(i)) if i < S // 2 else F32(eps - F32(step) * F32(S - 1 - i)) for i in range(S)], F32)
    return ts, float(F32(ts[0] - ts[1]))


def _injection(gx, y, lig0, B, S, rng, prec_kw):
    """Injected draws of B trajectories that start near the stored pose, and edges through score(return_edges=True)."""
    from dfmdock_amd.restraints import axis_angle_to_matrix
    c1, c2 = y[:, 1].mean(0), lig0[:, 1].mean(0)
    R0 = np.stack([axis_angle_to_matrix(0.3 * rng.standard_normal(3)) for _ in range(B)]).reshape(B, 9).astype(F32)
    inj = dict(R0=R0, tr_draw=((c2 - c1)[None] + 2.0 * rng.standard_normal((B, 3))).astype(F32),
               z_rot=rng.standard_normal((B, S, 3)).astype(F32), z_tr=rng.standard_normal((B, S, 3)).astype(F32))
    edges = np.empty((B, S + 1, gx.N, gx.K), np.int32)
    for s in range(S + 1):
        poses = (lig0[None] + rng.standard_normal((B, 1, 1, 3)).astype(F32)).astype(F32)
        edges[:, s] = gx.score(poses, 0.5, seed=900 + s, energy=False, return_edges=True, **prec_kw)["edges"]
    inj["edges"] = edges
    return inj


def _replay(r, inj, y, n, params, S, groups=None, center="ca", hp=None):
    """Worst per-atom deviation of the traced poses from the float64 replay: Euler-Maruyama step, restraint step (groups), symmetry
    step (the last one with last=True)."""
    from dfmdock_amd import restraints as RS, symmetry as SY
    ts, dt = _time_grid(S)
    worst = 0.0
    for b in range(len(r["lig_pos"])):
        for i in range(S):
            prev = r["init_pose"][b] if i == 0 else r["trace_pose"][b, i - 1]
            x = _em_host(prev, r["trace_scores"][b, i].astype(np.float64), inj["z_rot"][b, i], inj["z_tr"][b, i], float(ts[i]), dt,
                         0.0 if i == S - 1 else 0.5, center, hp)
            if groups:
                x, _, _ = RS.apply_step(x, RS.evaluate(groups, y, x, center=center)["step"], center=center)
            if ts[i] <= params.t_start:
                x, _, _ = SY.apply_step(x, SY.evaluate(y, x, n, params, center, last=i == S - 1), center=center)
            worst = max(worst, float(np.abs(x - r["trace_pose"][b, i]).max()))
    return worst


@pytest.mark.parametrize("prec", ["fp32", "mfma16"])
def test_step_replay_on_host(prec, model):
    from dfmdock_amd import engine
    from dfmdock_amd import restraints as RS, symmetry as SY
    n, B, S = 3, 2, 6
    gx, y, lig0 = _homodimer(model, "7CEI", n)
    kw = engine.precision_kwargs(prec)
    inj = _injection(gx, y, lig0, B, S, np.random.default_rng(4), kw)
    params = SY.SymmetryParams()
    gx.set_symmetry(n, params)
    r = gx.sample(B=B, num_steps=S, inject=inj, trace=True, symmetry=True, **kw)
    plain = gx.sample(B=B, num_steps=S, inject=inj, trace=True, **kw)
    assert np.abs(plain["trace_pose"][:, 0] - r["trace_pose"][:, 0]).max() > 0.05      # the symmetry step moved the first pose
    worst = _replay(r, inj, y, n, params, S)
    assert worst <= 1e-3, worst
    np.testing.assert_array_equal(r["trace_pose"][:, -1], r["lig_pos"])
    for b in range(B):
        cl, dth, s = _closure(y, r["lig_pos"][b], n)
        assert cl <= 1e-3 and dth <= 1e-5, (b, cl, dth, s)
        again = RS.replay_pose(lig0, r["rot_update"][b], r["tr_update"][b])      # the bookkeeping still describes the final pose
        assert np.abs(again - r["lig_pos"][b]).max() <= 1e-3
    # with a restraint set stored as well: restraint step first
    groups = RS.native_contact_groups(y, lig0, 5, cutoff=12.0, seed=0)
    assert groups
    gx.set_restraints(groups)
    rr = gx.sample(B=B, num_steps=S, inject=inj, trace=True, symmetry=True, restraints=True, **kw)
    assert _replay(rr, inj, y, n, params, S, groups) <= 1e-3
    assert not np.array_equal(rr["lig_pos"], r["lig_pos"])
    for b in range(B):
        cl, dth, _ = _closure(y, rr["lig_pos"][b], n)
        assert cl <= 1e-3 and dth <= 1e-5, (b, cl, dth)
    gx.set_restraints(None)
    # snap_last = 0: the last step follows the gains; and a late t_start leaves the early steps alone
    for params in (SY.SymmetryParams(snap_last=0), SY.SymmetryParams(t_start=0.5, gain_rot=1.0, gain_tr=0.25, max_rot=0.1)):
        gx.set_symmetry(n, params)
        rs = gx.sample(B=B, num_steps=S, inject=inj, trace=True, symmetry=True, **kw)
        assert _replay(rs, inj, y, n, params, S) <= 1e-3
    gx.set_symmetry(n, SY.SymmetryParams(snap_last=0))
    rs = gx.sample(B=B, num_steps=S, inject=inj, trace=True, symmetry=True, **kw)
    assert max(_closure(y, rs["lig_pos"][b], n)[0] for b in range(B)) > 1e-3      # (half of the last error is left)
    gx.close()


def test_clash_force_then_symmetry_stays_closed(model):
    n = 3
    gx, y, _ = _homodimer(model, "7CEI", n)
    gx.set_symmetry(n)
    r = gx.sample(B=8, num_steps=8, seed=2, mfma16=True, symmetry=True, use_clash_force=True)
    f = gx.sample(B=8, num_steps=8, seed=2, mfma16=True, use_clash_force=True)
    assert not np.array_equal(r["lig_pos"], f["lig_pos"])
    for b in range(8):
        cl, dth, _ = _closure(y, r["lig_pos"][b], n)
        assert cl <= 1e-3 and dth <= 1e-5, (b, cl, dth)
    g = gx.sample(B=8, num_steps=8, seed=2, mfma16=True, symmetry=True, use_clash_force=True, graph=True)
    for k in KEYS:
        np.testing.assert_array_equal(r[k], g[k], err_msg=k)
    gx.close()


def test_graph_with_symmetry_is_bitwise_plain(model):
    from dfmdock_amd import symmetry as SY
    gx, _, _ = _homodimer(model, "7CEI")
    kw = dict(B=6, num_steps=8, seed=11, mfma16=True, symmetry=True)
    gx.set_symmetry(3)
    pa, ga = gx.sample(**kw), gx.sample(graph=True, **kw)
    ga2 = gx.sample(graph=True, **kw)                                          # replayed graph
    gx.set_symmetry(5, SY.SymmetryParams(gain_rot=0.25, gain_tr=1.0, t_start=0.5, snap_last=0))      # another order and other parameters
    gb = gx.sample(graph=True, **kw)                                           # ... between two graph calls
    pb = gx.sample(**kw)
    gc = gx.sample(graph=True, **dict(kw, num_steps=5))                        # another step count: the last step is read from the device
    pc = gx.sample(**dict(kw, num_steps=5))
    gx.set_symmetry(5)
    gd, pd = gx.sample(graph=True, **dict(kw, num_steps=5)), gx.sample(**dict(kw, num_steps=5))
    for k in KEYS:
        np.testing.assert_array_equal(pa[k], ga[k], err_msg=k)
        np.testing.assert_array_equal(pa[k], ga2[k], err_msg=k)
        np.testing.assert_array_equal(pb[k], gb[k], err_msg=k)
        np.testing.assert_array_equal(pc[k], gc[k], err_msg=k)
        np.testing.assert_array_equal(pd[k], gd[k], err_msg=k)
    assert not np.array_equal(pa["lig_pos"], pb["lig_pos"]) and not np.array_equal(pc["lig_pos"], pd["lig_pos"])
    gx.close()


def test_batch_invariance(model):
    gx, y, lig0 = _homodimer(model, "7CEI")
    gx.set_symmetry(3)
    B, S = 64, 8
    inj = _injection(gx, y, lig0, B, S, np.random.default_rng(21), dict(mfma16=True))
    big = gx.sample(B=B, num_steps=S, inject=inj, symmetry=True, mfma16=True)
    seven = {k: np.ascontiguousarray(v[30:37]) for k, v in inj.items()}
    mid = gx.sample(B=7, num_steps=S, inject=seven, symmetry=True, mfma16=True)
    one = {k: np.ascontiguousarray(v[33:34]) for k, v in inj.items()}
    r1 = gx.sample(B=1, num_steps=S, inject=one, symmetry=True, mfma16=True)
    for k in ("lig_pos", "energy", "tr_update", "rot_update"):
        np.testing.assert_array_equal(mid[k], big[k][30:37], err_msg=k)
        np.testing.assert_array_equal(r1[k][0], big[k][33], err_msg=k)
    ev, ev7 = gx.symmetry_eval(big["lig_pos"]), gx.symmetry_eval(big["lig_pos"][30:37])
    for k in ev:
        np.testing.assert_array_equal(ev7[k], ev[k][30:37], err_msg=k)
    gx.close()


def test_second_family():
    from dfmdock_amd import engine
    from dfmdock_amd import restraints as RS, symmetry as SY
    hp = draw_hparams(1)
    m = engine.Model(draw_blob(1, "s1"), hp)
    n = 3
    gx, y, lig0 = _homodimer(m, "7CEI", n)
    params = SY.SymmetryParams()
    gx.set_symmetry(n, params)
    poses = _poses(y, n, 16, np.random.default_rng(8))
    worst, _ = _check_eval(gx.symmetry_eval(poses), y, poses, n, params, center="all_atoms")
    print("symmetry eval family 1:", json.dumps(worst))
    r = gx.sample(B=8, num_steps=8, seed=2, mfma16=True, symmetry=True)
    assert np.isfinite(r["lig_pos"]).all() and np.isfinite(r["energy"]).all()
    for b in range(8):
        cl, dth, _ = _closure(y, r["lig_pos"][b], n, center="all_atoms")
        assert cl <= 1e-3 and dth <= 1e-5, (b, cl, dth)
        again = RS.replay_pose(lig0, r["rot_update"][b], r["tr_update"][b], center="all_atoms")
        assert np.abs(again - r["lig_pos"][b]).max() <= 1e-3
    gx.close(); m.close()


def test_symmetry_closes_7cei_homotrimer(model):
    """7CEI-receptor homodimer, n = 3, B = 64, 40 steps, seed 0, native RNG, against the same call without the flag."""
    n = 3
    gx, y, _ = _homodimer(model, "7CEI", n)
    gx.set_symmetry(n)
    on = gx.sample(B=64, num_steps=40, seed=0, mfma16=True, symmetry=True)
    off = gx.sample(B=64, num_steps=40, seed=0, mfma16=True)
    c_on = np.array([_closure(y, p, n) for p in on["lig_pos"]])
    c_off = np.array([_closure(y, p, n) for p in off["lig_pos"]])
    q = lambda a: [float(v) for v in np.quantile(a, [0.0, 0.5, 1.0])]
    print("symmetry 7CEI C3:", json.dumps({"closure_on": q(c_on[:, 0]), "closure_off": q(c_off[:, 0]), "dtheta_on": q(c_on[:, 1]),
                                           "dtheta_off": q(c_off[:, 1]), "screw_on": q(c_on[:, 2]), "screw_off": q(c_off[:, 2])}))
    assert np.isfinite(on["lig_pos"]).all()
    assert c_on[:, 0].max() <= 1e-3, c_on[:, 0].max()
    assert not ((c_off[:, 1] < 1e-3) & (c_off[:, 2] < 1e-3)).any()
    gx.close()


def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def _chains(path):
    from dfmdock_amd import pdbio
    out = {}
    for a in pdbio.read_pdb(path):
        out.setdefault(a["chain"], []).append(a["coord"])
    return {k: np.asarray(v) for k, v in out.items()}


def test_cli_dock_with_symmetry(tmp_path):
    from cli_fixtures import write_ckpt
    from symmetry_fixtures import write_homodimer
    from dfmdock_amd.metrics import find_rigid_alignment
    a, a2, feat, other = write_homodimer(str(tmp_path))
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    common = ["--ckpt", ck, "--features", feat, "--num-samples", "8", "--num-steps", "8", "--top-k", "2"]
    p = _run(["dock", a, a2, "--symmetry", "C3", "--json", str(tmp_path / "res.json")] + common, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["symmetry"]["n"] == 3 and line["symmetry"]["m"] == 1 and line["symmetry"]["closure"] <= 1e-3
    assert "ring_clashes" not in line["symmetry"] and all(m["symmetry"]["n"] == 3 for m in line["models"])
    data = json.load(open(tmp_path / "res.json"))["symmetry_data"]
    assert len(data["closure"]) == 8 and max(data["closure"]) <= 1e-3
    for f in ["output.pdb"] + [os.path.basename(m["path"]) for m in line["models"]]:
        ch = _chains(str(tmp_path / f))
        assert list(ch) == ["A", "B", "C"] and len({len(v) for v in ch.values()}) == 1, (f, {k: len(v) for k, v in ch.items()})
        Q, t = find_rigid_alignment(ch["A"], ch["B"])
        for k, k1 in (("A", "B"), ("B", "C")):      # chain k + 1 is chain k under ONE rigid transform (the file's three decimals)
            assert np.sqrt((((ch[k] @ Q.T + t) - ch[k1]) ** 2).sum(-1)).max() <= 2e-3, (f, k)
    p4 = _run(["dock", a, a2, "--symmetry", "4", "--out", "c4.pdb"] + common, cwd=str(tmp_path))
    assert p4.returncode == 0, p4.stdout + p4.stderr
    l4 = json.loads(p4.stdout.strip().splitlines()[-1])
    assert l4["symmetry"]["n"] == 4 and isinstance(l4["symmetry"]["ring_clashes"], int) and len(_chains(str(tmp_path / "c4.pdb"))) == 4
    bad = _run(["dock", a, other, "--symmetry", "C3"] + common, cwd=str(tmp_path))
    assert bad.returncode != 0 and "sequences differ" in bad.stdout + bad.stderr


def test_cli_dock_with_symmetry_and_refinement(tmp_path):
    """--symmetry with --refine-t: the refinement samples with the symmetry step as well, every model gains the record of its refined
    pose, and the model files - which hold the refined poses - are closed trimers."""
    from cli_fixtures import write_ckpt
    from symmetry_fixtures import write_homodimer
    from dfmdock_amd.metrics import find_rigid_alignment
    a, a2, feat, _ = write_homodimer(str(tmp_path))
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    p = _run(["dock", a, a2, "--symmetry", "C3", "--ckpt", ck, "--features", feat, "--num-samples", "8", "--num-steps", "8", "--top-k", "2",
              "--refine-t", "0.2", "--refine-samples", "2"], cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["models"]
    for m in line["models"]:
        rs = m["refined_symmetry"]
        assert rs["n"] == 3 and rs["m"] == 1 and rs["closure"] <= 1e-3 and abs(rs["screw"]) <= 1e-3, rs
        assert m["symmetry"]["closure"] <= 1e-3 and "refined_energy" in m
        ch = _chains(m["path"])
        assert list(ch) == ["A", "B", "C"]
        Q, t = find_rigid_alignment(ch["A"], ch["B"])
        for k, k1 in (("A", "B"), ("B", "C")):
            assert np.sqrt((((ch[k] @ Q.T + t) - ch[k1]) ** 2).sum(-1)).max() <= 2e-3, (m["rank"], k)
