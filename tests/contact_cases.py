"""The in-contact rollout fixtures (tests/golden/contact*_*.npz, written by tests/golden/make_golden_contact.py): case table, blobs
and the conditions every fixture has to meet FOR THE REFERENCE ALONE.  Pure numpy: the generator asserts `check_conditions` before
it saves, tests/test_contact_golden.py re-asserts it from the stored arrays, the GPU tests take the cases and gates from here.

The weight draw is dfmdock_amd.weights.make_contact_weights: the chains stay within the 20 A cut-off over all 40 steps and the force
head follows the network, so a defect in a message or node kernel that only shows with live inter-chain edges moves f, and through f
the pose, by more than the gates below.  Each fixture carries the evidence, measured on the reference with the same draws and edge lists
replayed:
  twin16_rmsd[40]    pose deviation of a run with the weights and every nn.Linear input rounded to fp16  (what 16 bits may cost)
  defect_rmsd[40]    pose deviation of a run with EGNN_2.edge_mlp.0.weight * 1.02                          (what a defect moves)
  defect_f_rel[41]   rel. inf-norm change of f by that defect, teacher-forced on the clean poses
"""
import numpy as np

NUM_STEPS = 40
# kind: plain = inference_base.Euler_Maruyama_sampler, anneal = the same with noise_annealing, ode = inference_mlsb's sampler with
# ode=True (centred frame, `c1`), pair = src/inference.py driving DFMDock.forward (second family).  norm: length of the start draw
# that takes the place of randomize_pose's N(0, 30^2) draw (A); seed: of R0, the draw's direction, z and the sampled edges.
CASES = {
    "contact_syn_24_16": dict(cx="syn_24_16", family=0, kind="plain", clash=False, norm=5.0, seed=401),
    "contact_syn_64_48": dict(cx="syn_64_48", family=0, kind="plain", clash=False, norm=8.0, seed=402),
    "contact_7CEI": dict(cx="7CEI", family=0, kind="plain", clash=False, norm=8.0, seed=403),
    "contact_anneal_7CEI": dict(cx="7CEI", family=0, kind="anneal", clash=False, norm=8.0, seed=444),
    "contact_ode_syn_24_16": dict(cx="syn_24_16", family=0, kind="ode", clash=False, norm=5.0, seed=415),
    "contact2_syn_24_16": dict(cx="syn_24_16", family=1, kind="pair", clash=False, norm=5.0, seed=406),
    "contact_clash_syn_24_16": dict(cx="syn_24_16", family=0, kind="plain", clash=True, norm=5.0, seed=417),
    "contact_clash_syn_64_48": dict(cx="syn_64_48", family=0, kind="plain", clash=True, norm=8.0, seed=408),
}
FREE_CASES = [c for c, v in CASES.items() if not v["clash"]]
CLASH_CASES = [c for c, v in CASES.items() if v["clash"]]
RESTARTS = (8, 16, 24, 32)              # free cases: refine from the reference's pose before step i, compare the whole tail
CLASH_RESTARTS = (0, 8, 16, 24, 32)     # clash cases: one step after the restart only (the repulsion amplifies any deviation)

CLASH_DIST = 3.0                        # get_clashes: CA-CA distance <= 3 A
TWIN_GATE = 0.125                       # a quarter of the 0.5 A 16-bit rollout gate
DEFECT_F_GATE = 1e-3                    # ten times the fp32 forward gate
SAT_GATE = 0.10
# tr_score = unit(mean_j f_j) * scale, rot_score = unit(mean_j r_j x f_j) * scale: where the ligand sits near a force (torque) balance
# the mean m is a small difference of large terms.  |unit(m + dm) - unit(m)| <= 2 |dm| / |m| and |dm| <= max_j |df_j|, so an error
# ef = max|df| / max|f| on f allows up to 2 * ef * ratio on the direction, ratio = max|f| / |m|.  Every fixture but one keeps both
# ratios below CANCEL_GATE (check_conditions) and is held to the flat score gates (1e-4 fp32, 1e-2 16-bit).  The noise-free ODE run
# follows a force balance for half of its 41 evaluations whatever the seed (worst ratio 1700 to 8600 over six seeds tried; 1772 in the
# fixture): there the CPU oracle itself is at 3e-4 on tr_score with f at 1.6e-6, and the mfma16 engine at 8e-2 with f at 5e-4, a
# twentieth of its gate.  For that fixture the score gate of an evaluation is the flat gate or, where larger, what the inequality
# allows for the evaluation's own f error (which is held to the f gate): `score_gate`.
CANCEL_GATE = 250.0


def score_gate(name, gate, ratio, ef):
    """Per-evaluation gate of tr_score / rot_score of fixture `name` from the flat `gate`, the fixture's cancellation ratios and
    the evaluations' f errors."""
    gate = np.broadcast_to(np.asarray(gate, np.float64), np.shape(ratio))
    if CASES[name]["kind"] != "ode":
        return gate
    return np.maximum(gate, 2.0 * np.asarray(ef, np.float64) * np.asarray(ratio, np.float64))


def hparams(family):
    from dfmdock_amd.weights import HParams
    return HParams(family=1, mask_dist=20.0) if family else HParams()


_blobs = {}


def contact_blob(family):
    from dfmdock_amd.weights import make_contact_weights, pack_blob
    if family not in _blobs:
        hp = hparams(family)
        _blobs[family] = pack_blob(make_contact_weights(hp=hp), hp)
    return _blobs[family]


def ca_rmsd(a, b):
    """CA RMSD per pose of two [..., L, 3, 3] stacks."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a[..., 1, :] - b[..., 1, :]) ** 2).sum(-1).mean(-1))


def rel_inf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def eval_poses(g):
    """The 41 poses the reference evaluated the network on: the start pose and the pose after every complete step (after the clash
    force where it is on)."""
    after = g["poses_clash"] if "poses_clash" in g else g["poses"]
    return np.concatenate([g["init_pose"][None], after], 0)


def clash_margin_pairs(rec_pos, lig_pos, dev):
    """CA pairs whose distance lies within 2 * dev of the clash threshold: by how many the clash count of a pose that deviates by
    `dev` may differ."""
    d = np.linalg.norm(np.asarray(rec_pos, np.float64)[:, None, 1, :] - np.asarray(lig_pos, np.float64)[None, :, 1, :], axis=-1)
    return int((np.abs(d - CLASH_DIST) <= 2.0 * dev).sum())


def bins_rowsum(bins):
    """Checksum per node of the feature bins [N,K,4] of its K edges (slot- and channel-weighted, so that swapped bins show)."""
    b = np.asarray(bins).astype(np.int64)
    K = b.shape[1]
    w = (np.arange(K)[:, None] * 4 + np.arange(4)[None, :] + 1)
    return (b * w).sum((1, 2)).astype(np.int32)


def cancellation(g):
    """(max|f| / |mean f|, max|r x f| / |mean r x f|) per evaluation, r about the ligand's CA centroid."""
    f, ev = g["f"].astype(np.float64), eval_poses(g).astype(np.float64)
    r = ev[:, :, 1] - ev[:, :, 1].mean(1, keepdims=True)
    x = np.cross(r, f)
    return (np.abs(f).max((1, 2)) / np.linalg.norm(f.mean(1), axis=-1), np.abs(x).max((1, 2)) / np.linalg.norm(x.mean(1), axis=-1))


def check_conditions(name, g, rec_pos):
    """What makes a fixture worth having, for the reference alone (never loosened to fit an engine: choose another seed instead)."""
    c = CASES[name]
    n = NUM_STEPS + 1
    assert g["energy"].shape == (n,) and g["f"].shape[0] == n and g["num_clashes"].shape == (n,)
    assert (g["energy"] != 0).all(), f"{name}: energy == 0 at evaluations {np.flatnonzero(g['energy'] == 0)}"
    assert (g["pairs_in_cutoff"] > 0).all()
    assert g["sat_share"].max() <= SAT_GATE, f"{name}: clamp-saturated share {g['sat_share'].max()}"
    if c["cx"] in ("syn_64_48", "7CEI"):
        assert (g["num_clashes"] > 0).sum() * 2 >= n, f"{name}: clashes on {(g['num_clashes'] > 0).sum()} of {n} evaluations"
    assert g["defect_f_rel"].min() >= DEFECT_F_GATE, f"{name}: defect moves f by {g['defect_f_rel'].min()} only"
    ctr, crot = cancellation(g)
    if c["kind"] != "ode":      # (the ODE run follows the balance for 18 of its 41 evaluations)
        assert ctr.max() <= CANCEL_GATE and crot.max() <= CANCEL_GATE, f"{name}: cancellation {ctr.max():.0f} (tr) {crot.max():.0f} (rot)"
    assert g["bins_rowsum"].shape == (n, g["f"].shape[1] + int(g["R"]))
    if c["clash"]:      # free runs under the clash force diverge (the stored twin16_rmsd shows by how much): one-step comparisons only
        assert (g["clash_shift"] > 0).sum() >= 10, f"{name}: clash force on {(g['clash_shift'] > 0).sum()} steps"
        assert g["twin16_step_rmsd"].shape == (len(CLASH_RESTARTS),)
        assert g["twin16_step_rmsd"].max() <= TWIN_GATE, f"{name}: one-step fp16 twin {g['twin16_step_rmsd']}"
    else:
        assert g["twin16_rmsd"].max() <= TWIN_GATE, f"{name}: fp16 twin {g['twin16_rmsd'].max()} A"
        cap = clash_margin_pairs(rec_pos, g["poses"][-1], float(g["twin16_rmsd"][-1]))
        assert cap <= 2, f"{name}: {cap} CA pairs within 2 x {g['twin16_rmsd'][-1]} A of the clash threshold"
