"""The in-contact rollout fixtures (tests/golden/make_golden_contact.py) on the CPU: the conditions that make them worth having,
re-asserted from the stored arrays, and the plain-C oracle's injected 40-step rollouts against them at the oracle's gates
(tests/test_oracle_golden.py: CA RMSD <= 0.05 A over the first five steps, <= 0.5 A over the run).  CPU only."""
import numpy as np
import pytest

import contact_cases as cc
from conftest import complex_for, load_golden
from oracle import oracle as ora


def _rec_of(g, cx):
    return g["rec_centered"] if "rec_centered" in g else cx["rec_pos"]


@pytest.mark.parametrize("case", list(cc.CASES))
def test_fixture_conditions(case):
    """Every evaluation in contact and with a live energy head, the coordinate head inside its clamp, the 2 % defect visible on f at
    every evaluation, the fp16 twin a quarter of the 16-bit gate away at most - for the reference alone."""
    g = load_golden(case + ".npz")
    c = cc.CASES[case]
    cc.check_conditions(case, g, _rec_of(g, complex_for(c["cx"])))
    assert g["edges"].dtype == np.int16 and g["edges"].shape[0] == cc.NUM_STEPS + 1
    assert abs(float(np.linalg.norm(g["tr_draw"])) - c["norm"]) < 1e-5
    np.testing.assert_allclose(g["t_eval"][:-1], np.linspace(1.0, 1e-3, cc.NUM_STEPS), atol=1e-6)
    assert g["t_eval"][-1] == g["t_eval"][-2]
    assert float(g["energy"][-1]) == float(g["final_energy"]) and int(g["num_clashes"][-1]) == int(g["final_num_clashes"])
    if c["clash"]:      # the pose after the clash force is the pose before it shifted rigidly by the recorded amount
        d = g["poses_clash"] - g["poses"]
        np.testing.assert_allclose(np.linalg.norm(d[:, 0, 0], axis=-1), g["clash_shift"], atol=1e-4)
        assert np.abs(d - d[:, :1, :1]).max() < 1e-4


def _oracle_run(case):
    g = load_golden(case + ".npz")
    c = cc.CASES[case]
    o = ora.Oracle(cc.contact_blob(c["family"]), complex_for(c["cx"]), cc.hparams(c["family"]))
    inj = dict(R0=g["R0"], tr_draw=g["tr_draw"], edges=g["edges"].astype(np.int32))
    if c["kind"] != "ode":
        inj.update(z_rot=g["z_rot"], z_tr=g["z_tr"])
    r = o.sample(num_steps=cc.NUM_STEPS, inject=inj, trace=True, noise_annealing=c["kind"] == "anneal", ode=c["kind"] == "ode",
                 use_clash_force=c["clash"])
    assert r["forwards"] == cc.NUM_STEPS + 1
    shift = g["c1"] if "c1" in g else 0.0      # inference_mlsb's sampler works in the receptor-centred frame
    return g, r, shift


@pytest.mark.parametrize("case", cc.FREE_CASES)
def test_oracle_contact_rollout(case):
    g, r, shift = _oracle_run(case)
    np.testing.assert_allclose(r["init_pose"] - shift, g["init_pose"], atol=5e-5)
    rmsd = cc.ca_rmsd(r["trace_pose"] - shift, g["poses"])
    print(f"{case}: oracle rmsd max {rmsd.max():.2e} (defect twin {g['defect_rmsd'].max():.2e})")
    assert rmsd[:5].max() < 0.05 and rmsd.max() < 0.5, rmsd
    # fp32 against fp32: a third of what the reference's own 2 % defect twin moves the pose, wherever that is measurable
    big = g["defect_rmsd"] > 3e-3
    assert (rmsd[big] <= g["defect_rmsd"][big] / 3).all(), (rmsd[big], g["defect_rmsd"][big])
    sc = r["trace_scores"]
    assert cc.rel_inf(sc[0, 0:3], g["tr_score"][0]) < 1e-4 and cc.rel_inf(sc[0, 3:6], g["rot_score"][0]) < 1e-4
    E = float(g["final_energy"])
    assert abs(float(r["energy"]) - E) < 1e-3 * max(1.0, abs(E))
    if "tr_update" in g:
        np.testing.assert_allclose(r["tr_update"].reshape(-1), g["tr_update"].reshape(-1), atol=2e-3)
        np.testing.assert_allclose(r["rot_update"].reshape(-1), g["rot_update"].reshape(-1), atol=2e-4)
    cap = cc.clash_margin_pairs(_rec_of(g, complex_for(cc.CASES[case]["cx"])), g["poses"][-1], float(rmsd[-1]))
    assert cap <= 2 and abs(int(r["num_clashes"]) - int(g["final_num_clashes"])) <= cap


@pytest.mark.parametrize("case", cc.CLASH_CASES)
def test_oracle_contact_rollout_with_clash_force(case):
    """use_clash_force=True inside the step loop (inference_base.py:458-461): the trace holds the pose after the repulsion, and
    tr_update carries it."""
    g, r, _ = _oracle_run(case)
    rmsd = cc.ca_rmsd(r["trace_pose"], g["poses_clash"])
    print(f"{case}: oracle rmsd max {rmsd.max():.2e}")
    assert rmsd[:5].max() < 0.05 and rmsd.max() < 0.5, rmsd
    np.testing.assert_allclose(r["tr_update"].reshape(-1), g["tr_update"].reshape(-1), atol=2e-3 + 2 * rmsd.max())
