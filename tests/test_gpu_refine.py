"""Local refinement on the GPU (dfm_refine / dfm_forward_marginal / dfm_igso3_table; kernels k_igso3_cdf, k_start_pose) against the
reference's recorded forward process (tests/golden/igso3_ref.npz, make_golden_igso3.py), the float64 mirror dfmdock_amd/refine.py and
the CPU oracle.  Every test prints the figure it asserts on."""
import numpy as np
import pytest

import aux_harness as ah
from conftest import complex_for, load_golden, pair_hparams
from refine_replay import CONTACT_CUTOFF, oracle_refine_replay

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "mfma16", "f16"]
T_BEGIN_7CEI, SEED_7CEI = 0.1, 3      # chosen with the oracle alone: >= 18 CA contacts within 8 A at every one of the 40 steps


def kw(prec):
    return dict(mfma16=prec == "mfma16", f16=prec == "f16")


def rel_inf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def model(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob)
    yield m
    m.close()


@pytest.fixture(scope="module")
def model_pair(blob_pair):
    from dfmdock_amd import engine
    engine.set_device(0)
    m = engine.Model(blob_pair, pair_hparams())
    yield m
    m.close()


@pytest.fixture(scope="module")
def ref():
    return load_golden("igso3_ref.npz")


def _complex(model, case):
    from dfmdock_amd import engine
    cx = complex_for(case)
    return engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"]), cx


def test_igso3_table_vs_reference(model, ref):
    """Item 6.  Index and sigma exact, cdf within 1e-10 absolute.  The bound comes from the consumer: the angle is stored as float32
    (half an ulp at pi is 1.2e-7); an error d of the cdf moves the looked-up angle by d / pdf, and the fixture's uniforms sit where
    pdf >= 1e-3 (asserted by make_golden_igso3.py), so 1e-10 keeps the shift below 1e-7.  Measured on MI355X: see profiles/refine.txt."""
    worst = 0.0
    for n, t in enumerate(ref["t"]):
        r = model.igso3_table(float(t))
        dev = float(np.abs(r["cdf"] - ref[f"t{n}/cdf"]).max())
        print(f"igso3 t={t}: idx {r['sigma_idx']} sigma {r['sigma']!r} max |cdf - reference| {dev:.3e}")
        assert r["sigma_idx"] == int(ref[f"t{n}/sigma_idx"])
        assert r["sigma"] == float(ref[f"t{n}/sigma"])
        worst = max(worst, dev)
        assert dev < 1e-10, (t, dev)
        # the derived gate of k_igso3_cdf (tests/test_gpu_aux_kernels.py; 1.5e-13 .. 2e-11, entry by entry) against the table in extended
        # precision, and twice it against the recorded float64 table, which the same count of roundings bounds
        ext, gate = ah.igso3_ref(r["sigma"])
        assert (np.abs(r["cdf"] - ext) <= gate).all(), (t, float((np.abs(r["cdf"] - ext) / gate).max()))
        assert (np.abs(r["cdf"] - ref[f"t{n}/cdf"]) <= 2 * gate).all(), (t, float((np.abs(r["cdf"] - ref[f"t{n}/cdf"]) / gate).max()))
    print(f"igso3 max cdf deviation over the 8 t: {worst:.3e}")
    again = model.igso3_table(0.1)      # cached: the same bits
    np.testing.assert_array_equal(again["cdf"], model.igso3_table(0.1)["cdf"])


@pytest.mark.parametrize("prec", PRECS)
def test_injected_start_vs_reference_and_oracle(prec, model, ref):
    """Item 7: the start of dfm_refine with u_angle / axis_draw / tr_draw injected against oracle.modify_coords of the mirror's draws and
    against the pose the reference's own noising recorded (atol 3e-5 A, the gate of randomize_pose); the rotation vector / translation
    the call starts from against the mirror (2e-4 rad / 2e-3 A, the gates of test_sampler_injected_rollout for the updates)."""
    from dfmdock_amd import refine as RF
    from oracle import oracle as ora
    gx, cx = _complex(model, "fwd_syn_24_16")
    np.testing.assert_array_equal(cx["lig_pos"], ref["lig_pos"])
    for n, t in enumerate(ref["t"]):
        if t <= 1e-3:      # t_begin must exceed eps
            continue
        rinj = dict(u_angle=[ref[f"t{n}/fm_u"]], axis_draw=ref[f"t{n}/fm_axis"], tr_draw=ref[f"t{n}/fm_z"])
        r = gx.refine(B=1, t_begin=float(t), num_steps=2, refine_inject=rinj, trace=True, **kw(prec))
        rot, tr = RF.forward_marginal(np.float32(t), rinj["u_angle"], rinj["axis_draw"], rinj["tr_draw"])
        want = ora.modify_coords(cx["lig_pos"], rot[0], tr[0])
        fm = gx.forward_marginal(1, float(t), refine_inject=rinj)
        d = (np.abs(r["init_pose"][0] - want).max(), np.abs(r["init_pose"][0] - ref[f"t{n}/fm_pose"]).max(),
             np.abs(fm["rot"][0] - rot[0]).max(), np.abs(fm["tr"][0] - tr[0]).max(), np.abs(fm["rot"][0] - ref[f"t{n}/fm_rot"]).max())
        print(f"start {prec} t={t}: pose vs oracle {d[0]:.2e} vs reference {d[1]:.2e} A; rot vs mirror {d[2]:.2e} (vs reference {d[4]:.2e}) rad, tr {d[3]:.2e} A")
        np.testing.assert_allclose(r["init_pose"][0], want, atol=3e-5)
        np.testing.assert_allclose(r["init_pose"][0], ref[f"t{n}/fm_pose"], atol=3e-5)
        np.testing.assert_allclose(fm["rot"][0], rot[0], atol=2e-4)
        np.testing.assert_allclose(fm["tr"][0], tr[0], atol=2e-3)
        # the updates are ONE fp32 rounding of float64 values a few roundings from the mirror's (tests/test_gpu_aux_kernels.py): an fp32
        # ulp, 2 u |x|, where the float64 difference crosses a rounding boundary; the angle also moves by (table difference) / pdf, the
        # tables within twice the gate of k_igso3_cdf and pdf >= 1e-3 at the fixture's uniforms (make_golden_igso3.py).  The mirror
        # takes the draws as the kernel receives them: rounded to fp32
        rot32, tr32 = RF.forward_marginal(np.float32(t), *(np.asarray(rinj[k], np.float32) for k in ("u_angle", "axis_draw", "tr_draw")))
        dang = 2 * float(ah.igso3_ref(RF.sigma_index(np.float32(t))[1])[1].max()) / 1e-3
        assert (np.abs(fm["rot"][0] - rot32[0]) <= 2 * ah.U * np.abs(rot32[0]) + dang).all(), (t, fm["rot"][0], rot32[0])
        assert (np.abs(fm["tr"][0] - tr32[0]) <= 2 * ah.U * np.abs(tr32[0]) + 1e-12).all(), (t, fm["tr"][0], tr32[0])
    gx.close()


def test_injected_start_second_family(model_pair, ref):
    """Item 7, second family once: rotation about the centroid of all backbone atoms (oracle.modify_coords_all_atom)."""
    from dfmdock_amd import refine as RF
    from oracle import oracle as ora
    gx, cx = _complex(model_pair, "fwd2_syn_24_16")
    n, t = 3, 0.1
    rinj = dict(u_angle=[ref[f"t{n}/fm_u"]], axis_draw=ref[f"t{n}/fm_axis"], tr_draw=ref[f"t{n}/fm_z"])
    r = gx.refine(B=1, t_begin=t, num_steps=2, refine_inject=rinj, trace=True)
    rot, tr = RF.forward_marginal(np.float32(t), rinj["u_angle"], rinj["axis_draw"], rinj["tr_draw"], hp=pair_hparams())
    want = ora.modify_coords_all_atom(cx["lig_pos"], rot[0], tr[0])
    d = np.abs(r["init_pose"][0] - want).max()
    print(f"start family 1: pose vs oracle {d:.2e} A; vs the mirror {np.abs(r['init_pose'][0] - RF.noise_pose(cx['lig_pos'], rot[0], tr[0], 1)).max():.2e}")
    np.testing.assert_allclose(r["init_pose"][0], want, atol=3e-5)
    assert np.abs(r["init_pose"][0] - ora.modify_coords(cx["lig_pos"], rot[0], tr[0])).max() > 1e-4      # not the CA centroid
    gx.close()


@pytest.fixture(scope="module")
def replay_7cei(blob):
    return oracle_refine_replay(blob, complex_for("fwd_7CEI_p0"), T_BEGIN_7CEI, steps=40, seed=SEED_7CEI)


@pytest.mark.parametrize("prec", PRECS)
def test_interface_trajectory_vs_oracle(prec, model, replay_7cei):
    """Item 8: 40 steps of 7CEI from its native pose at t_begin = 0.1, everything injected (start draws, z_rot, z_tr, the edge lists
    oracle.knn_sample drew on the oracle's own poses), against the host replay Oracle.score -> torch_reverse -> modify_coords.  Gates:
    those of test_sampler_injected_rollout, unchanged - CA-RMSD of the first 5 steps < 0.05 A (fp32) / 0.5 A (16-bit), all steps
    < 0.5 A, first evaluation's scores within 1e-4 / 1e-2.  Condition, on the ORACLE's poses: at least 10 receptor-ligand CA pairs
    within 8 A at every step (measured: 18 at the least).  Per-step RMSD on MI355X: profiles/refine.txt."""
    g = replay_7cei
    print(f"oracle contacts (< {CONTACT_CUTOFF} A) per step: min {g['contacts'].min()} {g['contacts'].tolist()}")
    assert g["contacts"].min() >= 10
    gx, cx = _complex(model, "fwd_7CEI_p0")
    r = gx.refine(B=1, t_begin=T_BEGIN_7CEI, num_steps=40, trace=True, inject=dict(z_rot=g["z_rot"], z_tr=g["z_tr"], edges=g["edges"]),
                  refine_inject=dict(u_angle=g["u_angle"], axis_draw=g["axis_draw"], tr_draw=g["tr_draw"]), **kw(prec))
    np.testing.assert_allclose(r["init_pose"][0], g["init_pose"], atol=3e-5)
    ca, want = r["trace_pose"][0][:, :, 1, :], g["poses"][:, :, 1, :]
    rmsd = np.sqrt(((ca - want) ** 2).sum(-1).mean(-1))
    s_tr, s_rot = rel_inf(r["trace_scores"][0][0, 0:3], g["scores"][0, :3]), rel_inf(r["trace_scores"][0][0, 3:6], g["scores"][0, 3:])
    print(f"interface {prec}: first-evaluation scores rel {s_tr:.2e} / {s_rot:.2e}; CA-RMSD per step max {rmsd.max():.3e} first5 {rmsd[:5].max():.3e}")
    print(f"interface {prec} per-step CA-RMSD: " + " ".join(f"{x:.2e}" for x in rmsd))
    sixteen = prec != "fp32"
    assert rmsd[:5].max() < (0.5 if sixteen else 0.05), rmsd[:5]
    assert rmsd.max() < 0.5, rmsd.max()
    tol = 1e-2 if sixteen else 1e-4
    assert s_tr < tol and s_rot < tol, (s_tr, s_rot)
    if not sixteen and rmsd.max() < 1e-3:
        np.testing.assert_allclose(r["tr_update"][0], g["tr_update"], atol=2e-3)
        np.testing.assert_allclose(r["rot_update"][0], g["rot_update"], atol=2e-4)
    gx.close()


def _ks(x, cdf_fn):
    x = np.sort(np.asarray(x, np.float64))
    n = x.size
    c = cdf_fn(x)
    return float(max((np.arange(1, n + 1) / n - c).max(), (c - np.arange(n) / n).max()))


def test_native_draw_distributions(model, ref):
    """Item 9: dfm_forward_marginal with Philox draws, B = 65536, three t: one-sample Kolmogorov-Smirnov distance of the angles against
    the fixture's cdf (piecewise linear through (0, 0) and the table, the distribution np.interp samples), of tr / sigma_r3(t) per
    component against N(0, 1) and of the axis' z-component against U(-1, 1); each below 1.95 / sqrt(B), the alpha = 0.001 point of the
    Kolmogorov distribution.  Fixed seed: deterministic.  Measured D on MI355X: profiles/refine.txt."""
    from math import erf
    from dfmdock_amd import refine as RF
    gx, _ = _complex(model, "fwd_syn_24_16")
    B = 65536
    bound = 1.95 / np.sqrt(B)
    ncdf = np.vectorize(lambda v: 0.5 * (1.0 + erf(v / np.sqrt(2.0))))
    for n in (3, 5, 7):      # t = 0.1, 0.3, 1.0
        t = float(ref["t"][n])
        fm = gx.forward_marginal(B, t, seed=11 + n)
        ang = np.linalg.norm(fm["rot"].astype(np.float64), axis=-1)
        grid_w, grid_c = np.concatenate([[0.0], ref["omega"]]), np.concatenate([[0.0], ref[f"t{n}/cdf"]])
        d_ang = _ks(ang, lambda x: np.interp(x, grid_w, grid_c))
        d_tr = [_ks(fm["tr"][:, k] / RF.r3_sigma(np.float32(t)), ncdf) for k in range(3)]
        d_ax = _ks(fm["rot"][:, 2] / ang, lambda x: (x + 1.0) / 2.0)
        print(f"KS t={t}: angle D {d_ang:.4e}  tr D {d_tr[0]:.4e} {d_tr[1]:.4e} {d_tr[2]:.4e}  axis-z D {d_ax:.4e}  (bound {bound:.4e}; mean angle {ang.mean():.4f} rad)")
        assert d_ang < bound and max(d_tr) < bound and d_ax < bound
    gx.close()


@pytest.mark.parametrize("prec", ["fp32", "mfma16"])
def test_bitwise_properties(prec, model):
    """Item 10."""
    gx, cx = _complex(model, "fwd_syn_64_48_p0")
    keys = ("lig_pos", "rot_update", "tr_update", "energy")
    a = gx.refine(B=6, t_begin=0.2, num_steps=8, seed=4, **kw(prec))
    g = gx.refine(B=6, t_begin=0.2, num_steps=8, seed=4, graph=True, **kw(prec))
    one = gx.refine(B=1, t_begin=0.2, num_steps=8, seed=4, **kw(prec))
    sp = gx.refine(B=6, t_begin=0.2, num_steps=8, seed=4, start_pos=np.repeat(cx["lig_pos"][None], 6, 0), **kw(prec))
    fl = gx.refine(B=6, t_begin=0.2, num_steps=8, seed=4, restraints=True, **kw(prec))      # no set stored
    for k in keys:
        np.testing.assert_array_equal(a[k], g[k], err_msg=f"graph replay {k}")
        np.testing.assert_array_equal(a[k][0], one[k][0], err_msg=f"batch invariance {k}")
        np.testing.assert_array_equal(a[k], sp[k], err_msg=f"start_pos = the stored pose {k}")
        np.testing.assert_array_equal(a[k], fl[k], err_msg=f"DFM_F_RESTRAINTS without a set {k}")
    assert (a["lig_pos"][0] != a["lig_pos"][1]).any()
    rng = np.random.default_rng(0)
    poses = cx["lig_pos"][None] + rng.normal(0, 3.0, size=(3, 1, 1, 3)).astype(np.float32)
    n = gx.refine(B=3, t_begin=0.2, num_steps=4, start_pos=poses, perturb=False, trace=True, **kw(prec))
    np.testing.assert_array_equal(n["init_pose"], poses)
    # t_begin = 1 runs dfm_sample's time grid: the same start pose gives the same trajectory bits through both calls
    # (layer 0 direct in both: a message table is built on the stored pose's geometry, and set_pose rebuilds it)
    s = gx.sample(B=2, num_steps=6, seed=9, trace=True, step_energy=False, l0_table=False, **kw(prec))
    gx.set_pose(lig_pos=s["init_pose"][0])
    z = gx.refine(B=1, t_begin=1.0, num_steps=6, seed=9, perturb=False, l0_table=False, **kw(prec))
    np.testing.assert_array_equal(z["lig_pos"][0], s["lig_pos"][0])
    gx.close()


def test_rigidly_moved_start_hits_the_l0_table(model):
    """Item 11: start_pos = a rigid motion of the stored ligand: layer-0 table on against DFM_F_NO_L0_TABLE within the 1e-3 of
    test_gpu_l0_table.py, and the profile shows intra-chain hits (the rows the edge model evaluated are not all the edges)."""
    from oracle import oracle as ora
    gx, cx = _complex(model, "fwd_syn_64_48_p0")
    moved = ora.modify_coords(cx["lig_pos"], [0.3, -0.5, 0.2], [2.0, -1.0, 0.5])
    e = np.stack([ora.knn_sample(np.concatenate([cx["rec_pos"][:, 1], moved[:, 1]], 0), seed=s) for s in range(3)])[None]
    args = dict(B=1, t_begin=0.05, num_steps=2, start_pos=moved[None], perturb=False, inject=dict(edges=e), mfma16=True, trace=True)
    on = gx.refine(profile=True, **args)
    p = gx.profile()
    off = gx.refine(l0_table=False, **args)
    for k in (slice(0, 3), slice(3, 6)):
        d = rel_inf(on["trace_scores"][0][0, k], off["trace_scores"][0][0, k])
        print(f"l0 table on vs off, first evaluation: {d:.2e}; evals {p['l0_evals']} edges {p['l0_edges']} miss rows {p['l0_miss_rows']}")
        assert d < 1e-3
    assert p["l0_evals"] == 3 and 0 < p["l0_miss_rows"] < p["l0_edges"]
    intra = sum(int(((np.arange(112)[:, None] < 64) == (ee < 64)).sum()) for ee in e[0])
    assert p["l0_miss_rows"] < p["l0_edges"] - intra // 2      # at least half of the intra-chain edges were table hits
    gx.close()


def test_argument_validation(model):
    """Item 12a: each case DFM_E_INVALID (ValueError), the handle usable afterwards."""
    import ctypes as C
    from dfmdock_amd import _lib as L
    gx, cx = _complex(model, "fwd_syn_24_16")
    for bad in (dict(t_begin=float("nan")), dict(t_begin=1e-3), dict(t_begin=5e-4), dict(t_begin=1.5), dict(t_begin=0.1, num_steps=1),
                dict(t_begin=0.1, inject=dict(R0=np.eye(3, dtype=np.float32).reshape(1, 9))), dict(t_begin=0.1, inject=dict(tr_draw=np.zeros((1, 3))))):
        with pytest.raises(ValueError):
            gx.refine(B=1, **bad)
    out = L.TrajOutC()
    assert L.lib().dfm_refine(gx._h, 1, 4, 1e-3, 0.5, 0.5, 0, 0, None, None, None, C.byref(out)) == -1      # NULL params
    with pytest.raises(ValueError):
        gx.forward_marginal(1, 1.5)
    with pytest.raises(ValueError):
        model.igso3_table(-0.1)
    r = gx.refine(B=2, t_begin=0.1, num_steps=4)
    assert np.isfinite(r["energy"]).all()
    gx.close()


def _run(args, cwd):
    import os
    import subprocess
    import sys
    from conftest import ROOT
    return subprocess.run([sys.executable, "-m", "dfmdock_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))


def test_cli_refine_and_dock_refine(tmp_path):
    """Item 12b: `refine` writes output.pdb; `dock --top-k 3 --refine-t 0.1` writes three models whose refined energies are on the
    result line; `dock --top-k 3` without the option is unchanged by it (same bytes as the run before, and as a second plain run)."""
    import json
    from cli_fixtures import golden_7cei, write_ckpt, write_pair
    from dfmdock_amd import pdbio
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    ck = str(tmp_path / "model_0.ckpt")
    write_ckpt(ck, seed=0)
    rd = tmp_path / "refine"
    rd.mkdir()
    p = _run(["refine", rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--t-begin", "0.1", "--num-samples", "6", "--seed", "2"], cwd=str(rd))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert (rd / "output.pdb").exists() and line["t_begin"] == pytest.approx(0.1) and np.isfinite(line["energy"])
    lig = pdbio.backbone_from_atoms(pdbio.read_pdb(lig_pdb))
    n_rec = len(pdbio.read_pdb(rec_pdb))
    moved = np.array([a["coord"] for a in pdbio.read_pdb(str(rd / "output.pdb"))[n_rec:]])
    shift = np.sqrt(((moved - lig["aa_coords"]) ** 2).sum(-1).mean())
    print(f"cli refine: energy {line['energy']:.4f}, all-atom RMSD to the input pose {shift:.3f} A")
    assert 0 < shift < 15.0      # a local move: the global sampler's start is N(0, 30 A) away
    common = ["dock", rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--num-samples", "16", "--max-batch", "8", "--seed", "5", "--top-k", "3",
              "--cluster-radius", "0.5"]
    outs = {}
    for name, extra in (("plain", []), ("refined", ["--refine-t", "0.1", "--refine-samples", "3"])):
        d = tmp_path / name
        d.mkdir()
        q = _run(common + extra, cwd=str(d))
        assert q.returncode == 0, q.stdout + q.stderr
        outs[name] = (d, json.loads(q.stdout.strip().splitlines()[-1]))
    (dp, lp), (dr, lr) = outs["plain"], outs["refined"]
    assert "refine_t" not in lp and all("refined_energy" not in m for m in lp["models"])
    assert lr["refine_t"] == pytest.approx(0.1) and len(lr["models"]) == len(lp["models"]) == 3
    assert (dp / "output.pdb").read_bytes() == (dr / "output.pdb").read_bytes()
    for mp, mr in zip(lp["models"], lr["models"]):
        assert mp["index"] == mr["index"] and mp["energy"] == mr["energy"] and np.isfinite(mr["refined_energy"])
        assert (dr / f"output_{mr['rank']}.pdb").exists()
        assert (dp / f"output_{mp['rank']}.pdb").read_bytes() != (dr / f"output_{mr['rank']}.pdb").read_bytes()
    bad = _run(["dock", rec_pdb, lig_pdb, "--ckpt", ck, "--features", feat, "--refine-t", "0.1"], cwd=str(tmp_path))
    assert bad.returncode == 2 and "--top-k" in bad.stderr
