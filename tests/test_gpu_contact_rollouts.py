"""40-step sampler rollouts that STAY IN CONTACT, on the GPU against the reference (tests/golden/contact*_*.npz, written by
tests/golden/make_golden_contact.py on the weight draw dfmdock_amd.weights.make_contact_weights; tests/contact_cases.py has the case
table and what each fixture guarantees for the reference alone).

The seed-0 rollouts leave the 20 A cut-off within a few steps, so their steps 6 to 40 and their final energy / clash count / tr_update
compare zeros.  Here every one of the 41 evaluations has live inter-chain edges, a non-zero energy and (on the larger complexes)
clashes, and a 2 % error in one message weight moves f by >= 1e-3 at every evaluation - ten times the fp32 forward gate.  Three views
of each run, on the fp32, mfma16 and f16 engines, none of them behind an `if` on a measured value:

  free injected rollout      all 40 poses at the rollout gates (fp32 0.05 A, 16-bit 0.5 A); fp32 also within a third of what the
                             reference's own 2 % defect twin moves the pose; final energy, tr_update, rot_update, clash count
  teacher forcing            the 41 reference poses through one batched score() per engine, with and without the layer-0 table
  restarts                   refine() from the reference's pose before step i over the rest of the same time grid; with the clash
                             force on, one step after the restart only (the repulsion amplifies a 0.02 A deviation to Angstroms)

Every test prints the figures it asserts on.
"""
import numpy as np
import pytest

import contact_cases as cc
from conftest import complex_for, load_golden

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "mfma16", "f16"]
ROLL_GATE = {"fp32": 0.05, "mfma16": 0.5, "f16": 0.5}          # CA RMSD of an injected rollout (A), all 40 steps
FWD_GATE = {"fp32": 1e-4, "mfma16": 1e-2, "f16": 1e-2}          # f, tr_score, rot_score of one evaluation (rel. inf-norm)
S = cc.NUM_STEPS


def kw(prec):
    return dict(mfma16=prec == "mfma16", f16=prec == "f16")


def energy_gate(prec, E):
    return 1e-4 if prec == "fp32" else 3e-2 * max(1.0, abs(float(E)))


_models, _complexes, _goldens = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _resident():
    from dfmdock_amd import engine
    engine.set_device(0)
    yield
    for gx in _complexes.values():
        gx.close()
    for m in _models.values():
        m.close()
    _complexes.clear()
    _models.clear()


def setup(case):
    """(fixture, resident complex, frame shift) of a case; one model per family and one complex per (family, complex)."""
    from dfmdock_amd import engine
    c = cc.CASES[case]
    fam = c["family"]
    if fam not in _models:
        _models[fam] = engine.Model(cc.contact_blob(fam), cc.hparams(fam))
    if (fam, c["cx"]) not in _complexes:
        cx = complex_for(c["cx"])
        _complexes[(fam, c["cx"])] = engine.Complex(_models[fam], cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    if case not in _goldens:
        g = load_golden(case + ".npz")
        g["edges"] = g["edges"].astype(np.int32)
        _goldens[case] = g
    g = _goldens[case]
    # inference_mlsb's sampler (the ODE case) works in the receptor-centred frame: its poses are this engine's minus c1
    return g, _complexes[(fam, c["cx"])], (g["c1"].astype(np.float32) if "c1" in g else np.zeros(3, np.float32))


def flags(case):
    c = cc.CASES[case]
    return dict(noise_annealing=c["kind"] == "anneal", ode=c["kind"] == "ode", use_clash_force=c["clash"])


def inject(g, case, lo=0, B=1, start=True):
    """Draws and edge lists of steps lo.. for B identical trajectories (R0 / tr_draw only for a run from the start)."""
    def tile(a):
        return np.repeat(np.ascontiguousarray(a)[None], B, 0)
    inj = dict(edges=tile(g["edges"][lo:]))
    if start:
        inj.update(R0=tile(g["R0"].astype(np.float32).reshape(9)), tr_draw=tile(g["tr_draw"].reshape(3)))
    if cc.CASES[case]["kind"] != "ode":
        inj.update(z_rot=tile(g["z_rot"][lo:]), z_tr=tile(g["z_tr"][lo:]))
    return inj


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.FREE_CASES)
def test_free_injected_rollout(case, prec):
    """Measured on MI355X, max CA RMSD over the 40 steps (A), fp32 / mfma16 / f16; in brackets the reference's own twins that back the
    gates (max of the 2 % defect twin, max of the fp16 twin):
      contact_syn_24_16      3.2e-5 / 2.5e-3 / 1.3e-3   (1.6e-2, 2.0e-2)
      contact_syn_64_48      5.0e-5 / 2.7e-3 / 2.2e-3   (1.1e-2, 1.9e-2)
      contact_7CEI           2.7e-4 / 1.3e-2 / 1.1e-2   (4.6e-2, 2.3e-2)
      contact_anneal_7CEI    2.7e-4 / 8.5e-3 / 1.1e-2   (3.0e-2, 2.0e-2)
      contact_ode_syn_24_16  1.1e-4 / 1.5e-2 / 6.2e-3   (7.8e-2, 4.5e-2)
      contact2_syn_24_16     1.3e-5 / 5.9e-4 / 3.3e-4   (2.9e-2, 1.9e-2)
    fp32 stays below 2.2 % of the defect twin at every step (gate: a third).  The 16-bit engines reach 72 % of it: their own
    rounding (f to 4e-3 teacher-forced) is as large as what a 2 % weight error moves, so their gates pin larger defects only.
    Final energy within 8e-5 (fp32) / 3.3e-4 (16-bit), every final clash count equal to the reference's (2 to 48 clashes)."""
    g, gx, shift = setup(case)
    r = gx.sample(B=1, num_steps=S, inject=inject(g, case), trace=True, **flags(case), **kw(prec))
    rmsd = cc.ca_rmsd(r["trace_pose"][0] - shift, g["poses"])
    E, Eref = float(r["energy"][0]), float(g["final_energy"])
    rec = g["rec_centered"] if "rec_centered" in g else complex_for(cc.CASES[case]["cx"])["rec_pos"]
    cap = cc.clash_margin_pairs(rec, g["poses"][-1], float(rmsd[-1]))
    dn = abs(int(r["num_clashes"][0]) - int(g["final_num_clashes"]))
    big = g["defect_rmsd"] > 3e-3
    ratio = float((rmsd[big] / g["defect_rmsd"][big]).max())
    print(f"{case} {prec}: rmsd max {rmsd.max():.3e} final {rmsd[-1]:.3e} | defect twin max {g['defect_rmsd'].max():.3e} rmsd/defect max "
          f"{ratio:.3f} on {int(big.sum())} steps | dE {abs(E - Eref):.2e} (E {Eref:.4f}) clashes {int(r['num_clashes'][0])} vs "
          f"{int(g['final_num_clashes'])} cap {cap}")
    np.testing.assert_allclose(r["init_pose"][0] - shift, g["init_pose"], atol=1e-4 if shift.any() else 3e-5)
    assert rmsd.max() < ROLL_GATE[prec], rmsd
    if prec == "fp32":
        # the fp32 gate alone (0.05 A) is above what a 2 % weight error moves the pose: hold fp32 to a third of the defect twin
        assert (rmsd[big] <= g["defect_rmsd"][big] / 3).all(), (rmsd[big] / g["defect_rmsd"][big])
        assert abs(E - Eref) < 1e-3
        if "tr_update" in g:      # (inference_mlsb's sampler returns neither)
            np.testing.assert_allclose(r["tr_update"][0], g["tr_update"].reshape(3), atol=2e-3)
            np.testing.assert_allclose(r["rot_update"][0], g["rot_update"].reshape(3), atol=2e-4)
    else:
        assert abs(E - Eref) < 3e-2 * max(1.0, abs(Eref))
    assert cap <= 2 and dn <= cap, (dn, cap)


FLIP_F_GATE = 2e-3      # one edge with a neighbouring feature bin swaps one embedding row: ~1e-3 on that node's force (test_oracle_golden.py)
# the layer-0 message table exists for the fp32 and the mfma16 engine (dfm_score refuses DFM_F_L0_TABLE | DFM_F_F16)
TF_ENGINES = [("fp32", True), ("fp32", False), ("mfma16", True), ("mfma16", False), ("f16", False)]


@pytest.mark.parametrize("prec,l0_table", TF_ENGINES)
@pytest.mark.parametrize("case", list(cc.CASES))
def test_teacher_forced_evaluations(case, prec, l0_table):
    """All 41 evaluations of the reference run in one batched score(): its poses, time steps and edge lists in, f / scores / energy /
    clash count out.  The evaluation index of a miss says where along the run a kernel goes wrong.

    Feature bins: torch, libm and the GPU differ in the last bit of atan2 / acos, so about one edge in 10^6 lands in the neighbouring
    bin (test_oracle_golden.py: test_score_matches_reference_real_esm).  The fixture's bins_rowsum tells such an evaluation from an
    arithmetic error: at most two of the 41 evaluations may have one, their f / scores are then held to FLIP_F_GATE, every other
    evaluation to the forward gates.  tr_score / rot_score: the flat gates, except for the ODE run, which follows a force balance
    (cancellation ratio up to 1772, where the CPU oracle is at 3e-4 too): there the flat gate or, where larger, what the evaluation's
    own f error allows through |d unit(m)| <= 2 |dm| / |m| (contact_cases.score_gate).

    Measured on MI355X, worst f error over the 41 evaluations, fp32 / mfma16 / f16 (table on or off alike), and what the 2 % defect
    moves f by at least:
      contact_syn_24_16 5.6e-6 / 5.7e-4 / 3.2e-4 (2.7e-3)      contact_syn_64_48 7.1e-6 / 4.5e-4 / 3.4e-4 (1.2e-3)
      contact_7CEI 9.0e-6 / 3.9e-3 / 2.1e-3 (1.5e-3)           contact_anneal_7CEI 9.3e-6 / 3.4e-3 / 1.5e-3 (1.7e-3)
      contact_ode_syn_24_16 3.3e-6 / 5.3e-4 / 2.8e-4 (3.4e-3)  contact2_syn_24_16 8.6e-7 / 2.4e-4 / 1.3e-4 (1.7e-3)
      contact_clash_syn_24_16 5.3e-6 / 5.3e-4 / 2.4e-4 (2.7e-3) contact_clash_syn_64_48 6.9e-6 / 4.5e-4 / 2.7e-4 (1.5e-3)
    Energy within 9e-5 (fp32) / 2.3e-4 (16-bit).  One flipped evaluation each in contact_7CEI (36: f 2.3e-4, on the CPU oracle too) and
    contact_clash_syn_24_16 (18: f 6.7e-4, GPU only), one node each.  ODE tr_score at its force balance: 5.4e-4 / 8.4e-2 / 9.3e-2."""
    g, gx, shift = setup(case)
    poses = cc.eval_poses(g) + shift
    r = gx.score(poses, g["t_eval"], edges=g["edges"], energy=True, l0_table=l0_table, debug=True, **kw(prec))
    np.testing.assert_array_equal(r["edges"], g["edges"])
    flipped = np.array([(cc.bins_rowsum(r["bins"][i]) != g["bins_rowsum"][i]).sum() for i in range(S + 1)])
    ef = np.array([cc.rel_inf(r["f"][i], g["f"][i]) for i in range(S + 1)])
    et = np.array([cc.rel_inf(r["tr_score"][i], g["tr_score"][i]) for i in range(S + 1)])
    er = np.array([cc.rel_inf(r["rot_score"][i], g["rot_score"][i]) for i in range(S + 1)])
    ee = np.abs(r["energy"].astype(np.float64) - g["energy"])
    ctr, crot = cc.cancellation(g)
    tol = np.where(flipped > 0, max(FWD_GATE[prec], FLIP_F_GATE), FWD_GATE[prec])
    ok = flipped == 0
    print(f"{case} {prec} l0_table={l0_table}: f {ef[ok].max():.2e} (eval {ef.argmax()}) tr {et[ok].max():.2e} rot {er[ok].max():.2e} energy "
          f"{ee.max():.2e} | bin flips at evals {np.flatnonzero(flipped)} (nodes {flipped[flipped > 0]}, f {ef[~ok]}) | tr/gate "
          f"{(et / cc.score_gate(case, tol, ctr, ef)).max():.2f} rot/gate {(er / cc.score_gate(case, tol, crot, ef)).max():.2f} | defect moves f by >= "
          f"{g['defect_f_rel'].min():.2e}")
    assert (flipped > 0).sum() <= 2 and flipped.max() <= 2, flipped      # (one flipped edge touches one node, or two in a symmetric pair)
    assert (ef < tol).all(), (ef.argmax(), ef.max())
    assert (et < cc.score_gate(case, tol, ctr, ef)).all(), (et.argmax(), et.max(), ctr[et.argmax()])
    assert (er < cc.score_gate(case, tol, crot, ef)).all(), (er.argmax(), er.max(), crot[er.argmax()])
    gate = np.array([energy_gate(prec, e) for e in g["energy"]])
    assert (ee < gate).all(), (ee.argmax(), ee.max())
    np.testing.assert_array_equal(r["num_clashes"], g["num_clashes"])      # the pose is the reference's


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.FREE_CASES)
def test_restart_reproduces_the_tail(case, prec):
    """refine(perturb=False) from the reference's pose before step i, over linspace(t_i, eps, 40 - i): the same spacing as the full
    grid, so steps i..39 must land on the reference's poses - each restart drops the deviation accumulated so far.
    Measured on MI355X, worst tail RMSD over i = 8, 16, 24, 32 (A), fp32 / mfma16 / f16: syn_24_16 6.0e-5 / 8.6e-4 / 4.5e-4, syn_64_48
    1.6e-5 / 5.1e-4 / 2.8e-4, 7CEI 2.3e-4 / 1.1e-3 / 1.1e-3, anneal_7CEI 4.8e-5 / 2.1e-3 / 2.0e-3, ode_syn_24_16 1.3e-4 / 1.6e-2 /
    7.8e-3, contact2_syn_24_16 4.5e-6 / 3.8e-4 / 2.7e-4."""
    g, gx, shift = setup(case)
    ev = cc.eval_poses(g)
    worst = {}
    for i in cc.RESTARTS:
        r = gx.refine(B=1, t_begin=float(g["t_eval"][i]), start_pos=ev[i] + shift, perturb=False, num_steps=S - i,
                      inject=inject(g, case, lo=i, start=False), trace=True, **flags(case), **kw(prec))
        rmsd = cc.ca_rmsd(r["trace_pose"][0] - shift, g["poses"][i:])
        E, Eref = float(r["energy"][0]), float(g["final_energy"])
        worst[i] = (float(rmsd.max()), abs(E - Eref))
        assert rmsd.shape == (S - i,) and rmsd.max() < ROLL_GATE[prec], (i, rmsd)
        if prec == "fp32":
            big = g["defect_rmsd"][i:] > 3e-3
            assert (rmsd[big] <= g["defect_rmsd"][i:][big] / 3).all(), (i, rmsd[big] / g["defect_rmsd"][i:][big])
        assert abs(E - Eref) < (1e-3 if prec == "fp32" else 3e-2 * max(1.0, abs(Eref))), i
    print(f"{case} {prec}: " + "  ".join(f"i={i}: rmsd {a:.2e} dE {b:.1e}" for i, (a, b) in worst.items()))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.CLASH_CASES)
def test_clash_force_one_step_after_restart(case, prec):
    """use_clash_force=True inside the step loop (inference_base.py:458-461).  Free runs under the repulsion diverge (the fixture's
    twin16_rmsd: Angstroms), so only the first step after each restart is compared: the pose after the clash force, and the step's
    translation tau + clash force - what the step adds to tr_update; a rotation about the CA centroid leaves the centroid in place,
    so it is the shift of the CA centroid.  tr_update itself is returned for the whole run only: it must take the start pose onto
    the run's own final pose, which it cannot do if any step's clash force were left out of it.
    Measured on MI355X, worst one-step RMSD (A), fp32 / mfma16 / f16: syn_24_16 2.8e-5 / 2.6e-3 / 6.5e-4, syn_64_48 1.1e-5 / 9.8e-4 /
    1.5e-3 (the fixture's one-step fp16 twin: 1.9e-2); clash shifts of 0.5 to 3.8 A on the compared steps; bookkeeping <= 4e-5 A."""
    from oracle import oracle as ora
    g, gx, _ = setup(case)
    ev = cc.eval_poses(g)
    out = []
    for i in cc.CLASH_RESTARTS:
        r = gx.refine(B=1, t_begin=float(g["t_eval"][i]), start_pos=ev[i], perturb=False, num_steps=S - i,
                      inject=inject(g, case, lo=i, start=False), trace=True, **flags(case), **kw(prec))
        first = r["trace_pose"][0][0]
        rmsd = float(cc.ca_rmsd(first, g["poses_clash"][i]))
        tr_ref = g["step_tr"][i].astype(np.float64) + (g["poses_clash"][i] - g["poses"][i])[0, 0]
        tr_gpu = first[:, 1].astype(np.float64).mean(0) - ev[i][:, 1].astype(np.float64).mean(0)
        dtr = float(np.abs(tr_gpu - tr_ref).max())
        book = float(np.abs(ora.modify_coords(ev[i], r["rot_update"][0], r["tr_update"][0]) - r["lig_pos"][0]).max())
        out.append(f"i={i}: rmsd {rmsd:.2e} dtr {dtr:.2e} book {book:.1e} shift {g['clash_shift'][i]:.2f}")
        assert rmsd < ROLL_GATE[prec], (i, rmsd)
        assert dtr < ROLL_GATE[prec], (i, dtr)
        assert book < 2e-3, (i, book)
        # (the fixture itself: the reference's recorded step takes its pose before step i onto its pose after the clash force)
        assert cc.ca_rmsd(ora.modify_coords(ev[i], g["step_rot"][i], tr_ref.astype(np.float32)), g["poses_clash"][i]) < 1e-4
    assert sum(g["clash_shift"][i] > 0 for i in cc.CLASH_RESTARTS) >= 3      # the repulsion acts on the compared steps
    print(f"{case} {prec}: " + "  ".join(out))


def _rows_equal(a, b, keys=("lig_pos", "energy", "tr_update", "rot_update", "num_clashes")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_variants_bitwise_on_contact_7CEI():
    """mfma16 on the DB5 pair, in contact throughout: the captured-graph replay, the untraced run (ligand-only last layer on the 40
    step evaluations) and a batch of three identical trajectories all give bitwise the eager traced run's result."""
    case = "contact_7CEI"
    g, gx, _ = setup(case)
    args = dict(num_steps=S, mfma16=True)
    traced = gx.sample(B=1, inject=inject(g, case), trace=True, **args)
    rmsd = cc.ca_rmsd(traced["trace_pose"][0], g["poses"])
    print(f"{case} mfma16: rmsd max {rmsd.max():.3e}, energy {float(traced['energy'][0]):.5f} (reference {float(g['final_energy']):.5f})")
    assert rmsd.max() < ROLL_GATE["mfma16"]
    eager = gx.sample(B=1, inject=inject(g, case), trace=False, **args)
    _rows_equal(eager, traced)
    _rows_equal(gx.sample(B=1, inject=inject(g, case), trace=False, graph=True, **args), eager)
    three = gx.sample(B=3, inject=inject(g, case, B=3), trace=False, **args)
    for b in range(3):
        _rows_equal({k: v[b:b + 1] for k, v in three.items()}, traced)
