"""The kernel harness of the pair heads and score heads without a GPU (tests/heads_harness.py, tests/kernels/heads_harness.hip): it
builds and links against the library, its float64 references agree with torch's float64 modules, the bound of k_pair_head_m in
tests/test_gpu_head_kernels.py holds for an fp32 restatement of the kernel and is missed by five subtly wrong ones, no input of a GPU
test sits within rounding of a threshold, and the LayerNorm conditioning kappa of the committed golden cases is where the moment form
of the variance is harmless."""
import os

import numpy as np
import pytest

import heads_harness as hh
import kernel_harness as kh
from conftest import complex_for, load_golden, pair_hparams

H = hh.H


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return hh.compile_shim(tmp_path_factory.mktemp("heads_harness"))


def test_library_exports_the_launchers():
    """The harness links against the launchers by name: a build with hidden visibility would break it silently."""
    out = kh.exported_symbols(hh.LIBDIR + "/libdfmdock_amd.so", True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in hh.LAUNCHERS:
        assert s in syms, s


def test_shim_links(shim):
    out = kh.exported_symbols(shim, False)
    for s in hh.LAUNCHERS:
        assert s in out, s
    h = hh.Harness(shim)      # also checks that the ctypes call record has the shim's size
    assert h.guard >= 1024


# ---- the float64 references against torch's float64 modules -------------------------------------------------------------------------
def test_pair_references_agree_with_torch():
    """Linear(513 -> 256) on cat[h_r, h_l, D] -> LayerNorm -> SiLU -> Linear(256 -> 1 / 64), F.normalize(vec) s pooled, masked energy,
    confidence, clashes: torch float64 modules on the concatenated input against the split form of the references."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    B, R, L = 2, 5, 4
    N = R + L
    h = rng.standard_normal((B, N, H))
    W = rng.standard_normal((H, 2 * H + 1)) / np.sqrt(2 * H)
    W[:, 2 * H] = rng.standard_normal(H) * 2e-2
    ln_w, ln_b = 1 + 0.1 * rng.standard_normal(H), 0.1 * rng.standard_normal(H)
    w3, w3d = rng.standard_normal(H) / 16, rng.standard_normal((64, H)) / 16
    ca = hh.lattice_coords(rng, B, N).astype(np.float64)
    ca[0, R, :3] = ca[0, 0, :3]                                     # a coincident pair: F.normalize's eps
    P, Q = h @ W[:, :H].T, h @ W[:, H:2 * H].T
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    x = t(ca[..., :3])
    vec = x[:, :R, None, :] - x[:, None, R:, :]
    D = vec.norm(dim=-1)
    inp = torch.cat([t(h)[:, :R, None, :].expand(B, R, L, H), t(h)[:, None, R:, :].expand(B, R, L, H), D[..., None]], -1)
    ln = torch.nn.LayerNorm(H, eps=1e-5).double()
    with torch.no_grad():
        ln.weight.copy_(t(ln_w)); ln.bias.copy_(t(ln_b))
        act = torch.nn.SiLU()(ln(inp @ t(W).T))
        s_t = act @ t(w3)
        d_t = act @ t(w3d).T
        f_t = (F.normalize(vec, dim=-1) * s_t[..., None]).sum(1) / R
        mask = (D < hh.CUT_OFF).double()
    s, _, _, Dn = hh.pair_head_exact_ref(P, Q, ca, R, W[:, 2 * H], ln_w, ln_b, w3)
    assert np.abs(s - s_t.numpy()).max() < 1e-12
    sm = hh.pair_head_m_ref(P, Q, ca, R, W[:, 2 * H], ln_w, ln_b, w3)[0]
    assert np.abs(sm - s_t.numpy()).max() < 1e-12
    dist = hh.pair_head_exact_ref(P, Q, ca, R, W[:, 2 * H], ln_w, ln_b, w3d.T)[0]
    assert np.abs(dist - d_t.numpy()).max() < 1e-12
    fin = hh.finish64(s, ca, R, hh.CUT_OFF, 1.0 / R)
    assert np.abs(fin["fvec"] - f_t.numpy()).max() < 1e-12
    assert np.isfinite(fin["fvec"]).all()
    assert np.abs(fin["esum"] - (s_t * mask).sum((1, 2)).numpy()).max() < 1e-12
    assert (fin["count"] == mask.sum((1, 2)).numpy()).all() and (fin["clash"] == (D <= 3.0).sum((1, 2)).numpy()).all()
    assert np.abs(fin["conf"] - s_t.mean((1, 2)).numpy()).max() < 1e-12


def test_head_references_agree_with_torch():
    """The time embedding (sin / cos -> Linear -> Sigmoid) and the two scale MLPs (Linear(129 -> 128) on cat[norm, t_embed] -> LayerNorm
    -> SiLU -> Linear -> Softplus) against torch float64, on both sides of the Softplus threshold."""
    import torch
    rng = np.random.default_rng(1)
    B, R, L = 3, 5, 7
    tt = np.array([0.0, 0.3, 1.0], np.float32)
    for sat in (None, (25.0, -60.0)):
        w = hh.heads_weights(1, sat)
        base, _ = hh.time_embed64(tt, w)
        t = lambda x: torch.tensor(np.asarray(x, np.float64))
        xp = t(tt)[:, None] * t(w["t_W"])[None] * 2 * np.pi
        temb = torch.sigmoid(torch.cat([xp.sin(), xp.cos()], -1) @ t(w["t_lin"]).T)
        fvec = rng.standard_normal((B, L, 3)).astype(np.float32)
        ca = hh.lattice_coords(rng, B, R + L)
        sc, _, pre = hh.heads64(fvec, ca, R, w, base, float(L))
        tr = t(fvec).mean(1)
        rot = torch.cross(t(ca[:, R:, :3]), t(fvec), dim=-1).mean(1)
        for g, (pred, n) in enumerate(((tr, "trs"), (rot, "rots"))):
            ln = torch.nn.LayerNorm(hh.HI, eps=1e-5).double()
            with torch.no_grad():
                ln.weight.copy_(t(w[n + "_ln_w"])); ln.bias.copy_(t(w[n + "_ln_b"]))
                nrm = pred.norm(dim=-1, keepdim=True)
                o = torch.nn.SiLU()(ln(torch.cat([nrm, temb], -1) @ t(w[n + "0"]).T)) @ t(w[n + "4"]).reshape(-1, 1)
                want = pred / (nrm + 1e-6) * torch.nn.Softplus()(o)
            # (the fp32 Fourier argument of time_embed64 against the float64 one here: |t W 2 pi| <= 20, 3 roundings)
            assert np.abs(sc[:, g * 3:g * 3 + 3] - want.numpy()).max() < 1e-4 * max(1.0, float(want.abs().max()))
            assert np.abs(pre[:, g] - o.numpy()[:, 0]).max() < 1e-4 * max(1.0, float(o.abs().max()))
        if sat:
            assert (pre[:, 0] > 20).all() and (pre[:, 1] < -50).all()


def test_update_reference_agrees_with_the_oracle():
    """update64 against the oracle's fp32 modify_coords / rot_compose / torch_reverse (inference_base.py), CA and all-atom centre."""
    from oracle import oracle as ora
    rng = np.random.default_rng(2)
    L = 9
    lig = (rng.standard_normal((1, L, 9)) * 5 + 3).astype(np.float32)
    scores = np.zeros((1, 8))
    scores[0, :6] = rng.standard_normal(6) * 0.3
    ru, tu = np.array([[0.3, -0.2, 0.5]], np.float32), np.array([[1.0, 2.0, -3.0]], np.float32)
    z_rot, z_tr = rng.standard_normal((1, 3)).astype(np.float32), rng.standard_normal((1, 3)).astype(np.float32)
    g_r, g_t, dt, ns = 1.3, 2.1, 0.025, 0.5
    for ode in (0, 1):
        sp = dict(g2_r=g_r * g_r, g_r=g_r, hg2_r=0.5 * g_r * g_r, g2_t=g_t * g_t, g_t=g_t, hg2_t=0.5 * g_t * g_t, dt=dt, sqrt_dt=np.sqrt(dt),
                  rot_noise=ns, tr_noise=ns)
        for all_atoms in (0, 1):
            nl, nt, nr, rot, tr = hh.update64(scores, lig, ru, tu, sp, z_rot, z_tr, ode, all_atoms)
            rot_o = ora.torch_reverse(g_r, scores[0, 3:6].astype(np.float32), dt, ns, z_rot[0], ode=bool(ode))
            tr_o = ora.torch_reverse(g_t, scores[0, :3].astype(np.float32), dt, ns, z_tr[0], ode=bool(ode))
            assert np.abs(rot[0] - rot_o).max() < 1e-6 and np.abs(tr[0] - tr_o).max() < 1e-6
            mc = ora.modify_coords_all_atom if all_atoms else ora.modify_coords
            assert np.abs(nl[0].reshape(L, 3, 3) - mc(lig[0].reshape(L, 3, 3), rot_o, tr_o)).max() < 1e-4
            assert np.abs(nr[0] - ora.rot_compose(ru[0], rot_o)[0]).max() < 1e-5
            assert np.abs(nt[0] - (tu[0] + tr_o)).max() < 1e-5


# ---- the bound of k_pair_head_m has power ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def m_cases():
    out = {}
    for name, c in hh.pair_m_cases().items():
        args = (c["P"], c["Q"], c["ca4"], c["R"], c["w_d"], c["ln_w"], c["ln_b"], c["w3"])
        s, bound, scale, _, kappa, er = hh.pair_head_m_ref(*args)
        out[name] = dict(args=args, s=s, bound=bound, scale=scale, kappa=kappa, er=er)
    return out


def test_the_restatement_stays_under_the_bound(m_cases):
    """The fp32 restatement of k_pair_head_m (moments, ez2 - mean^2, exp2 / rcp SiLU) on every input of the GPU tests."""
    for name, c in m_cases.items():
        got = hh.pair_head_m_fp32(*c["args"])
        assert np.isfinite(got).all(), name
        ratio = np.abs(got - c["s"]) / c["bound"]
        assert ratio.max() <= 1.0, (name, float(ratio.max()))
        assert float(c["er"].max()) < 0.1, "the bound linearises in the relative error of rstd"


@pytest.mark.parametrize("mutant", hh.MUTANTS)
def test_the_bound_catches_a_subtly_wrong_kernel(m_cases, mutant):
    """Each mutant of the restatement misses the bound by at least 4 x on the GPU tests' inputs: at every size at which it can show at all
    (rows 8..15 of a wave exist from 33 ligand residues of a chunk on; the LayerNorm eps shows at the LOW input scales, where it is 0.5 % of the variance)."""
    shows = {"swap_rows": lambda R, L: L >= 33, "no_eps": lambda R, L: False}.get(mutant, lambda R, L: True)
    worst = {}
    for name, c in m_cases.items():
        got = hh.pair_head_m_fp32(*c["args"], mutant=mutant)
        with np.errstate(invalid="ignore"):
            worst[name] = float(np.nanmax(np.abs(got - c["s"]) / c["bound"]))
        R, L = c["args"][0].shape[1] - c["s"].shape[2], c["s"].shape[2]
        if name.startswith("size_") and shows(R, L):
            assert worst[name] >= 4.0, (mutant, name, worst[name])
    assert max(worst.values()) >= 4.0, (mutant, worst)
    if mutant == "no_eps":
        low = [worst[f"size_{R}_{L}"] for i, (R, L) in enumerate(hh.PAIR_M_SIZES) if i % 2]
        assert min(low) >= 4.0, (mutant, worst)


def test_kappa_of_the_sweep_cases(m_cases):
    for k in hh.KAPPAS:
        got = float(np.median(m_cases[f"kappa_{k:g}"]["kappa"]))
        assert 0.6 * k < got < 1.6 * k, (k, got)


# ---- the bound of k_pair_head<1> has power, and is the tighter one ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def x_cases():
    out = {}
    for name, c in hh.pair_x_cases().items():
        args = (c["P"], c["Q"], c["ca4"], c["R"], c["w_d"], c["ln_w"], c["ln_b"], c["w3"])
        s, bound, scale, _ = hh.pair_head_x_ref(*args)
        out[name] = dict(args=args, s=s, bound=bound, scale=scale, bound_m=hh.pair_head_m_ref(*args)[1], low=name.startswith("size_") and
                         [f"size_{R}_{L}" for R, L in hh.PAIR_X_SIZES].index(name) % 2 == 1)
    return out


def test_the_exact_bound_is_the_tighter_one(x_cases):
    """On every input k_pair_head<1> is tested with its bound is below k_pair_head_m's, pair by pair, and an fp32 restatement of the
    kernel's three sequential loops stays under it."""
    for name, c in x_cases.items():
        assert (c["bound"] < c["bound_m"]).all(), name
        ratio = np.abs(hh.pair_head_x_fp32(*c["args"]) - c["s"]) / c["bound"]
        assert ratio.max() <= 1.0, (name, float(ratio.max()))


@pytest.mark.parametrize("mutant", hh.MUTANTS)
def test_the_exact_bound_catches_a_subtly_wrong_kernel(x_cases, mutant):
    """The five wrong kernels (mutants of the moment / exp2 / rcp restatement) miss k_pair_head<1>'s bound by at least 4 x at every size
    (the LayerNorm eps: at the sizes with the LOW input scales, where it shows)."""
    for name, c in x_cases.items():
        if not name.startswith("size_") or (mutant == "no_eps" and not c["low"]):
            continue
        got = hh.pair_head_m_fp32(*c["args"], mutant=mutant)
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got - c["s"]) / c["bound"]))
        assert worst >= 4.0, (mutant, name, worst)


# ---- threshold safety -----------------------------------------------------------------------------------------------------------
def test_no_input_sits_within_rounding_of_a_threshold():
    """For every GPU case: no pair has |D - cut_off| or |D - 3| in the open interval (0, 1e-3), with D as the kernels form it in fp32 and
    in float64, and the two agree on which side every pair is.  The cases place pairs ON both thresholds (D exact in fp32)."""
    on_cut = on_clash = 0
    for name, ca, R in hh.all_coordinate_sets():
        _, D = hh.pair_dist64(ca, R)
        v = ca[:, :R, None, :3] - ca[:, None, R:, :3]
        D32 = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        assert D32.dtype == np.float32
        for thr in (hh.CUT_OFF, 3.0):
            for d in (D, D32.astype(np.float64)):
                gap = np.abs(d - thr)
                assert not ((gap > 0) & (gap < 1e-3)).any(), (name, thr)
            assert ((D < thr) == (D32 < np.float32(thr))).all() and ((D <= thr) == (D32 <= np.float32(thr))).all(), (name, thr)
        on_cut += int((D32 == np.float32(hh.CUT_OFF)).sum())
        on_clash += int((D32 == np.float32(3.0)).sum())
    assert on_cut > 0 and on_clash > 0
    for R, L in hh.ENERGY_SIZES:
        c = hh.energy_case(R, L)
        _, D = hh.pair_dist64(c["ca4"], R)
        assert (D[:, 0, 0] == hh.CUT_OFF).all() and (L == 1 or (D[:, 0, 1] == 3.0).all())


# ---- where the committed features sit on the kappa curve ------------------------------------------------------------------------------
GOLDEN_CASES = ("fwd2_syn_9_7", "fwd2_syn_24_16", "fwd2_syn_64_48_p0", "fwd2_syn_64_48_p1", "fwd2_syn_64_48_p2", "fwd2_7CEI_p0",
                "fwd2_7CEI_p1", "fwd2_7CEI_p2")


DRAW_CASES = ("fwd2_syn_24_16", "fwd2_syn_64_48_p0")      # the further weight draws: h_last from the oracle on the golden pose and graph


def golden_kappa(blob_pair):
    """kappa = E[z^2] / (Var[z] + eps) over all pairs of the committed fwd2_* cases: the oracle's h_last (the golden files) and the
    pair weights of the seed-0 draw; for the draws s1, s2, x3 (trunk weights x 3) the oracle's h_last on two of the cases.
    Rows: (case, head, median, max, max relative bound of rstd)."""
    from conftest import draw_blob
    from dfmdock_amd.weights import unpack_blob
    from oracle import oracle as ora
    todo = [(case, "s0", blob_pair) for case in GOLDEN_CASES] + [(case, d, draw_blob(1, d)) for d in ("s1", "s2", "x3") for case in DRAW_CASES]
    rows = []
    for case, draw, blob in todo:
        w = unpack_blob(blob, pair_hparams())
        g = load_golden(case + ".npz")
        cx = complex_for(case)
        R = cx["rec_pos"].shape[0]
        pos = np.concatenate([cx["rec_pos"], g["lig_pos"]], 0)[None, :, 1, :].astype(np.float32)
        ca = pos - pos[:, R:].mean(1, keepdims=True)
        if draw == "s0":
            h = g["h_last"].astype(np.float64)[None]
        else:
            r = ora.Oracle(blob, cx, pair_hparams()).score(g["lig_pos"], float(g["t"]), edges=g["edges"])
            h = np.asarray(r["h_layers"][-1], np.float64)[None]
            case = f"{case}[{draw}]"
        for head in ("to_force", "to_energy", "to_confidence"):
            W = w[head + ".0.weight"].astype(np.float64)
            P, Q = (h @ W[:, :H].T).astype(np.float32), (h @ W[:, H:2 * H].T).astype(np.float32)
            _, _, _, _, kappa, er = hh.pair_head_m_ref(P, Q, ca, R, W[:, 2 * H], w[head + ".1.weight"], w[head + ".1.bias"],
                                                        w[head + ".3.weight"].reshape(-1))
            rows.append((case, head, float(np.median(kappa)), float(kappa.max()), float(er.max())))
    return rows


def test_golden_features_sit_low_on_the_kappa_curve(blob_pair):
    """The moment form ez2 - mean^2 loses accuracy in proportion to kappa.  On every pair of the committed golden cases, with the seed-0
    weights and with the three further committed draws, the bound of the relative error of rstd (24 kappa u and the dot-product term)
    stays under 1e-3, one tenth of the 16-bit engines' 1e-2 gate: the variance needs no per-row shift for these features.  All four
    draws are zero-mean random weights, for which kappa ~ 1 is expected; trained weights are not in the tree and are not covered.  (DFM_HEAD_PROFILE=<dir>: the table goes to <dir>/head_kernels_kappa.txt.)"""
    rows = golden_kappa(blob_pair)
    lines = ["case head kappa_median kappa_max rstd_rel_bound_max"] + [f"{c} {h} {m:.3f} {x:.3f} {e:.3e}" for c, h, m, x, e in rows]
    print("\n".join(lines))
    out = os.environ.get("DFM_HEAD_PROFILE")
    if out:
        with open(os.path.join(out, "head_kernels_kappa.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert max(r[4] for r in rows) < 1e-3
