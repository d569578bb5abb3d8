"""Kernel-level harness of the pair heads and score heads (tests/kernels/heads_harness.hip): everything downstream of the trunk.

The shim drives the shipped launchers of dfmdock_amd/libdfmdock_amd.so (dfm::launch_pair_head, launch_pair_head_m,
launch_pair_finish_s, launch_pair_finish, launch_pair_dist, launch_energy_pairs, launch_time_embed, launch_heads, launch_prep_pose)
under the guard-band protocol of tests/kernel_harness.py.  This module binds it and holds
  * float64 numpy references of each operation, written from the model definition (egnn_net.py:329-358, :413-470; score_net_mlsb.py
    :162-172, :386-411; inference_base.py:342-352, :439-456), not from the kernels;
  * the error bounds of each kernel relative to those references (derivations: the docstring of tests/test_gpu_head_kernels.py);
  * numpy fp32 restatements of k_pair_head_m's arithmetic (row moments, ez2 - mean^2, exp2 / rcp SiLU; five mutants of it) and of
    k_pair_head<1>'s (three sequential loops), with which tests/test_heads_harness_cpu.py shows that the two bounds have power;
  * the inputs of the GPU tests, so that the CPU tests can check conditions on them (threshold safety, the restatement under the bound).
"""
import ctypes as C
import functools

import numpy as np

import kernel_harness as kh
from kernel_harness import HIP_SUCCESS, LIBDIR, ROOT, Out, guards_intact, is_sentinel      # noqa: F401 (re-exported)

LAUNCHERS = ("_ZN3dfm16launch_pair_headERKNS_8PairArgsEP12ihipStream_t",
             "_ZN3dfm18launch_pair_head_mERKNS_8PairArgsEP12ihipStream_t",
             "_ZN3dfm20launch_pair_finish_sERKNS_8PairArgsEifPfS3_P12ihipStream_t",
             "_ZN3dfm18launch_pair_finishEPKfiiifPfS1_S2_P12ihipStream_t",
             "_ZN3dfm16launch_pair_distEPKfS1_PK15HIP_vector_typeIfLj4EEiiiS1_S1_S1_S1_PfP12ihipStream_t",
             "_ZN3dfm19launch_energy_pairsEPKfS1_PK15HIP_vector_typeIfLj4EEiiifPKNS_8HeadsDevEiPfPiP12ihipStream_t",
             "_ZN3dfm17launch_time_embedEPKfiPKNS_8HeadsDevEPfP12ihipStream_t",
             "_ZN3dfm12launch_headsERKNS_8HeadArgsEP12ihipStream_t",
             "_ZN3dfm16launch_prep_poseEPKfS1_iiiiP15HIP_vector_typeIfLj4EES4_S4_P12ihipStream_t")
H, HI = 256, 128
U = 2.0 ** -24                    # unit roundoff of fp32
LN_EPS = 1e-5
SILU_S = np.float32(-1.44269504088896340736)
PM_RT, PM_LC = 32, 64             # k_pair_head_m: receptor x ligand residues of a workgroup

SLOTS = ("P", "Q", "ca4", "w_d", "ln_w", "ln_b", "w3", "S", "fpart", "spart", "clash", "fvec", "conf", "dist",
         "enA", "enB", "en_ln_w", "en_ln_b", "en_w3",
         "t", "t_W", "t_lin", "trs0", "trs_ln_w", "trs_ln_b", "trs4", "rots0", "rots_ln_w", "rots_ln_b", "rots4", "base",
         "scores", "z_rot", "z_tr", "lig", "tr_upd", "rot_upd", "trace_pose", "trace_scores", "step_params", "ctl",
         "rec_pos", "prep_pos", "prep_ca4", "prep_cb4")
LONGS = ("hid_bstride", "z_bstride", "trace_bstride", "trace_s_bstride")
FLOATS = ("cut_off", "inv_pool", "pool_div", "g2_r", "g_r", "hg2_r", "g2_t", "g_t", "hg2_t", "dt", "sqrt_dt", "rot_noise", "tr_noise")
INTS = ("B", "R", "L", "Rp", "mode", "n_part", "want_energy", "en_mode", "do_update", "ode", "all_atoms", "prep_next", "step", "n_times")
OPS = ("pair_head", "pair_head_m", "pair_finish_s", "pair_finish", "pair_dist", "energy_pairs", "time_embed", "heads", "prep_pose")
STEP_FIELDS = ("g2_r", "g_r", "hg2_r", "g2_t", "g_t", "hg2_t", "dt", "sqrt_dt", "rot_noise", "tr_noise")
HEAD_W = ("t_W", "t_lin", "trs0", "trs_ln_w", "trs_ln_b", "trs4", "rots0", "rots_ln_w", "rots_ln_b", "rots4")


class Call(C.Structure):
    _fields_ = ([("buf", kh.Buf * len(SLOTS))] + [(n, C.c_longlong) for n in LONGS] + [("seed", C.c_ulonglong)]
                + [(n, C.c_float) for n in FLOATS] + [(n, C.c_int) for n in INTS])


compile_shim = functools.partial(kh.compile_shim, "heads")


class Harness(kh.KernelHarness):
    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)
        self.lib.hh_step_params_bytes.restype = C.c_longlong
        assert int(self.lib.hh_step_params_bytes()) == 48


def step_params(entries):
    """dfm::StepParams records (ten floats, step, pad) from dicts of STEP_FIELDS + 'step'."""
    out = np.zeros((len(entries), 12), np.float32)
    for i, e in enumerate(entries):
        out[i, :10] = [e[k] for k in STEP_FIELDS]
        out[i, 10:] = np.array([e["step"], 0], np.uint32).view(np.float32)
    return out


# ---- float64 references -------------------------------------------------------------------------------------------------------
def f64(x):
    return np.asarray(x, np.float64)


def silu64(y):
    return y / (1.0 + np.exp(-y))


def layernorm64(z, w, b):
    """Three-pass LayerNorm over the last axis, eps 1e-5.  Returns (y, d = z - mean, var)."""
    mean = z.mean(-1, keepdims=True)
    d = z - mean
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + LN_EPS) * f64(w) + f64(b), d, var


def softplus64(o):
    """torch.nn.Softplus(beta = 1, threshold = 20)."""
    o = f64(o)
    return np.where(o > 20.0, o, np.log1p(np.exp(np.minimum(o, 20.0))))


def pair_dist64(ca, R):
    """vec[b][r][l] = x_r - x_l and D = |vec| from the fp32 coordinates ca [B][N][>=3]."""
    ca = f64(ca)[..., :3]
    vec = ca[:, :R, None, :] - ca[:, None, R:, :]
    return vec, np.sqrt((vec * vec).sum(-1))


def pair_z64(P, Q, ca, R, w_d):
    """Linear(513 -> 256, no bias)(cat[h_r, h_l, D]) split as P_r + Q_l + w_d D: z [B][R][L][256], zabs = |P| + |Q| + |w_d| D."""
    _, D = pair_dist64(ca, R)
    Pr, Ql = f64(P)[:, :R, None, :], f64(Q)[:, None, R:, :]
    wd = f64(w_d)
    return Pr + Ql + wd * D[..., None], np.abs(Pr) + np.abs(Ql) + np.abs(wd) * D[..., None], D


def ln_silu_bound(z, dz, ln_w, ln_b, ns, k_silu=5.0):
    """a = SiLU(LayerNorm(z)) in float64 and the bound da of an fp32 kernel that forms it in three passes from inputs carrying |error|
    <= dz, its two reductions rounding at most `ns` times each (the derivation: tests/test_gpu_head_kernels.py)."""
    y, d, var = layernorm64(z, ln_w, ln_b)
    w = np.abs(f64(ln_w))
    dmean = dz.mean(-1, keepdims=True) + (ns + 1) * U * np.abs(z).mean(-1, keepdims=True)
    dd = dz + dmean + U * np.abs(d)
    dvar = 2 * (np.abs(d) * dd).mean(-1, keepdims=True) + (ns + 2) * U * var
    er = 0.5 * dvar / (var + LN_EPS) + 3 * U
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    dy = w * rstd * (dd + np.abs(d) * (er + 3 * U)) + U * np.abs(y)
    a = silu64(y)
    return a, 1.1 * dy + k_silu * U * np.abs(a)


def dot_bound(a, da, w3, nacc):
    """o = a . w3 over the last axis (w3 [C] or [C][K]) with the bound of an fp32 accumulation of at most `nacc` roundings."""
    w3 = f64(w3)
    return a @ w3, (da + U * np.abs(a)) @ np.abs(w3) + nacc * U * (np.abs(a) @ np.abs(w3)), np.abs(a) @ np.abs(w3)


def pair_head_exact_ref(P, Q, ca, R, w_d, ln_w, ln_b, w3, ns=256, nacc=256):
    """s(r, l) [B][R][L] (or [B][R][L][K] for w3 [C][K]) in float64, the bound of a tree-reduced three-pass kernel such as k_pair_dist
    (IEEE expf and division; ns / nacc roundings in the statistics / in the output dot), and the natural scale sum_c |SiLU(y_c) w3_c|."""
    z, zabs, D = pair_z64(P, Q, ca, R, w_d)
    a, da = ln_silu_bound(z, 6 * U * zabs, ln_w, ln_b, ns)
    return dot_bound(a, da, w3, nacc) + (D,)


def seq_err(terms):
    """u * sum_k |s_k| over the running partial sums s_k of a sequential fp32 accumulation of `terms` along the last axis, in the kernel's
    order (channel 0 first): the first-order bound of that loop's rounding error (each addition rounds its own partial sum once)."""
    return U * np.abs(np.cumsum(terms, -1)).sum(-1, keepdims=True)


def pair_head_x_ref(P, Q, ca, R, w_d, ln_w, ln_b, w3):
    """s(r, l) [B][R][L] in float64 and the bound of k_pair_head<1>, from that kernel's own order of operations: three sequential loops
    over the channels (sum z, sum (z - mean)^2, sum SiLU(y) w3), each charged u times its running partial sums (seq_err), IEEE sqrtf /
    division, expf within 1 ulp.  Derivation: tests/test_gpu_head_kernels.py.  Returns (s, bound, scale, D)."""
    z, zabs, D = pair_z64(P, Q, ca, R, w_d)
    lw, lb = f64(ln_w), f64(ln_b)
    PQ = f64(P)[:, :R, None, :] + f64(Q)[:, None, R:, :]
    wdD = np.abs(f64(w_d)) * D[..., None]
    dz = U * (np.abs(PQ) + 4 * wdD + np.abs(z))                      # P + Q | w_d D (product, D's 3 u) | the second add
    y, d, var = layernorm64(z, lw, lb)
    mean = z.mean(-1, keepdims=True)
    dmean = (seq_err(z) + dz.sum(-1, keepdims=True)) / H + U * np.abs(mean)
    dd = dz + dmean + U * np.abs(d)
    dsq = 2 * np.abs(d) * dd + U * d * d
    dvar = (seq_err(d * d) + dsq.sum(-1, keepdims=True)) / H + U * var
    er = 0.5 * dvar / (var + LN_EPS) + 3 * U
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    dy = np.abs(lw) * rstd * (dd + np.abs(d) * (er + 2 * U)) + U * np.abs(y)
    a = silu64(y)
    da = 1.1 * dy + 4 * U * np.abs(a)
    t = a * f64(w3)
    scale = np.abs(t).sum(-1)
    bound = (np.abs(f64(w3)) * da + U * np.abs(t)).sum(-1) + seq_err(t)[..., 0]
    return t.sum(-1), bound, scale, D


def pair_head_x_fp32(P, Q, ca, R, w_d, ln_w, ln_b, w3):
    """k_pair_head<1>'s arithmetic in numpy float32, its three channel loops accumulated sequentially (np.cumsum adds in order)."""
    f = np.float32
    P, Q, ca = np.asarray(P, f), np.asarray(Q, f), np.asarray(ca, f)
    w_d, ln_w, ln_b, w3 = (np.asarray(x, f) for x in (w_d, ln_w, ln_b, w3))
    vec = ca[:, :R, None, :3] - ca[:, None, R:, :3]
    D = np.sqrt((vec[..., 0] * vec[..., 0] + vec[..., 1] * vec[..., 1]) + vec[..., 2] * vec[..., 2]).astype(f)
    z = (P[:, :R, None, :] + Q[:, None, R:, :]) + w_d * D[..., None]
    seq = lambda x: np.cumsum(x, -1, dtype=f)[..., -1:]
    mean = seq(z) * f(1.0 / H)
    d = z - mean
    rstd = f(1) / np.sqrt(seq(d * d) * f(1.0 / H) + f(LN_EPS))
    y = d * rstd * ln_w + ln_b
    a = y / (f(1) + np.exp(-y))
    return seq(a * w3)[..., 0]


def pair_head_m_ref(P, Q, ca, R, w_d, ln_w, ln_b, w3):
    """s(r, l) [B][R][L] in float64 and the bound of k_pair_head_m (LayerNorm statistics from row moments: the kappa u term).
    Returns (s, bound, scale, D, kappa, er) with kappa = E[z^2] / (Var[z] + eps) and er the relative bound of rstd, per pair."""
    z, zabs, D = pair_z64(P, Q, ca, R, w_d)
    lw, lb = f64(ln_w), f64(ln_b)
    y, d, var = layernorm64(z, lw, lb)
    mean = z.mean(-1, keepdims=True)
    pq = (np.abs(f64(P))[:, :R, None, :] * np.abs(f64(Q))[:, None, R:, :]).mean(-1, keepdims=True)
    ez2 = (z * z).mean(-1, keepdims=True)
    dmean = 24 * U * zabs.mean(-1, keepdims=True)
    dez2 = U * (24 * (zabs * zabs).mean(-1, keepdims=True) + 512 * pq)
    dvar = dez2 + 2 * np.abs(mean) * dmean + 2 * U * mean * mean
    er = 0.5 * dvar / (var + LN_EPS) + 3 * U
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    T = rstd * np.abs(lw) * (zabs + np.abs(mean)) + np.abs(lb)
    dy = np.abs(lw) * rstd * (np.abs(d) * er + dmean) + 12 * U * T
    a = silu64(y)
    da = 1.1 * dy + 6 * U * np.abs(a)
    w = np.abs(f64(w3))
    scale = np.abs(a) @ w
    return a @ f64(w3), (da + 3 * U * np.abs(a)) @ w + 130 * U * scale, scale, D, (ez2 / (var + LN_EPS))[..., 0], er[..., 0]


def finish64(s, ca, R, cut_off, inv_pool):
    """The reductions over the receptor residues of s [B][R][L] (egnn_net.py:430-470): force pooled with inv_pool, clash count
    D <= 3, masked energy (sum, count) over D < cut_off, confidence mean.  `fabs` = sum_r |unit vec * s| * inv_pool (the force's scale)."""
    vec, D = pair_dist64(ca, R)
    unit = vec / np.maximum(D, 1e-12)[..., None]          # F.normalize(vec, eps = 1e-12)
    s = f64(s)
    mask = D < cut_off
    return dict(fvec=(unit * s[..., None]).sum(1) * inv_pool, fabs=np.abs(unit * s[..., None]).sum(1) * inv_pool,
                clash=(D <= 3.0).sum((1, 2)), esum=np.where(mask, s, 0.0).sum((1, 2)), eabs=np.where(mask, np.abs(s), 0.0).sum((1, 2)),
                count=mask.sum((1, 2)), conf=s.mean((1, 2)), cabs=np.abs(s).mean((1, 2)), D=D)


def time_embed64(t, w):
    """Gaussian-Fourier -> Linear -> Sigmoid -> the t_embed columns of the two scale nets' first Linear: base [n][2][128].
    The Fourier argument is formed with the kernel's three fp32 multiplies, as the fp32 model forms it; the rest is float64."""
    t32 = np.asarray(t, np.float32)[:, None]
    xp = ((t32 * np.asarray(w["t_W"], np.float32)[None]) * np.float32(2.0)) * np.float32(3.14159265358979323846)
    xp = f64(xp)
    four = np.concatenate([np.sin(xp), np.cos(xp)], -1)
    pre = four @ f64(w["t_lin"]).T
    temb = 1.0 / (1.0 + np.exp(-pre))
    base = np.stack([temb @ f64(w["trs0"])[:, 1:].T, temb @ f64(w["rots0"])[:, 1:].T], 1)
    babs = np.stack([temb @ np.abs(f64(w["trs0"]))[:, 1:].T, temb @ np.abs(f64(w["rots0"]))[:, 1:].T], 1)
    # sinf / cosf 2 ulp of values <= 1; Linear: 8 roundings (fma pair + butterfly); sigmoid <= 1/4 slope, 4 ulp; second Linear likewise
    dpre = (3 * U + 8 * U) * (np.abs(four) @ np.abs(f64(w["t_lin"])).T)
    dtemb = 0.25 * dpre + 4 * U * temb
    dbase = np.stack([dtemb @ np.abs(f64(w["trs0"]))[:, 1:].T, dtemb @ np.abs(f64(w["rots0"]))[:, 1:].T], 1) + 8 * U * babs
    return base, dbase


def aa_to_mat64(aa):
    """Rodrigues: rotation matrix of an axis-angle vector."""
    aa = f64(aa)
    th = np.linalg.norm(aa)
    K = np.array([[0, -aa[2], aa[1]], [aa[2], 0, -aa[0]], [-aa[1], aa[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def mat_to_aa64(Rm):
    """Axis-angle of a rotation by an angle in (0, pi) (the tests stay well inside)."""
    th = np.arccos(np.clip((np.trace(Rm) - 1) / 2, -1, 1))
    ax = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]]) / (2 * np.sin(th))
    return ax * th


def heads64(fvec, ca, R, w, base, pool_div, en_part=None, clash_part=None, en_mode=0):
    """k_heads' scores in float64 (score_net_mlsb.py:396-411): pooled force / torque, the two scale MLPs with Softplus(threshold 20),
    energy and clash totals.  base [B][2][128].  Returns (scores [B][8], bound [B][8], pre-activations [B][2])."""
    fvec, ca = f64(fvec), f64(ca)[:, R:, :3]
    B, L = fvec.shape[:2]
    tr = fvec.sum(1) / pool_div
    tq = np.cross(ca, fvec)
    rot = tq.sum(1) / pool_div
    # double sums of fp32 terms (the torque's terms: two products and a difference in fp32), one rounding to fp32 after the division
    tqabs = np.abs(ca[..., (1, 2, 0)] * fvec[..., (2, 0, 1)]) + np.abs(ca[..., (2, 0, 1)] * fvec[..., (1, 2, 0)])
    dpred = [2 * U * np.abs(fvec).sum(1) / pool_div, 4 * U * tqabs.sum(1) / pool_div]
    scores, bound, pre = np.zeros((B, 8)), np.zeros((B, 8)), np.zeros((B, 2))
    for g, (pred, name) in enumerate(((tr, "trs"), (rot, "rots"))):
        w0 = f64(w[name + "0"])
        nrm = np.linalg.norm(pred, axis=-1, keepdims=True)
        dn = np.linalg.norm(dpred[g], axis=-1, keepdims=True) + 4 * U * nrm
        hid = w0[:, 0][None] * nrm + f64(base)[:, g]
        dhid = np.abs(w0[:, 0])[None] * dn + 2 * U * (np.abs(w0[:, 0])[None] * nrm + np.abs(f64(base)[:, g]))
        a, da = ln_silu_bound(hid, dhid, w[name + "_ln_w"], w[name + "_ln_b"], ns=7)
        o, do, _ = dot_bound(a, da, f64(w[name + "4"]).reshape(-1), 8)
        sp = softplus64(o)
        dsp = np.where(o > 20, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(o, 20)))) * do + 6 * U * sp
        unit = pred / (nrm + 1e-6)
        scores[:, g * 3:g * 3 + 3] = unit * sp[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            du = np.where(nrm > 0, (dpred[g] + np.abs(unit) * dn) / (nrm + 1e-6), 0.0)
        bound[:, g * 3:g * 3 + 3] = du * sp[:, None] + np.abs(unit) * dsp[:, None] + 4 * U * np.abs(unit * sp[:, None])
        pre[:, g] = o
    if en_part is not None:
        es, ec, cl = f64(en_part)[..., 0].sum(1), f64(en_part)[..., 1].sum(1), f64(clash_part).sum(1)
        scores[:, 6] = es / (ec + 1e-6) if en_mode == 0 else (es / np.maximum(ec, 1.0) if en_mode == 1 else es)
        bound[:, 6] = 4 * U * np.abs(scores[:, 6])
        scores[:, 7] = cl
    return scores, bound + 1e-37, pre


def update64(scores, lig, rot_upd, tr_upd, sp, z_rot, z_tr, ode, all_atoms):
    """The Euler-Maruyama step and modify_coords in float64 (inference_base.py:439-456, :342-352; r3_diffuser.py:40-55): rotation about the
    CA (all_atoms: all-backbone-atom) centroid, then the translation; tr_update += tr; rot_update = axis_angle(R(rot) R(rot_update)).
    sp: the step's scalars (STEP_FIELDS).  Returns (lig, tr_update, rot_update, rot, tr)."""
    scores, lig = f64(scores), f64(lig)
    B = lig.shape[0]
    s = {k: float(np.float32(sp[k])) for k in STEP_FIELDS}
    out_l, out_t, out_r, rots, trs = np.zeros_like(lig), np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, 3))
    for b in range(B):
        if ode:
            rot, tr = s["hg2_r"] * scores[b, 3:6] * s["dt"], s["hg2_t"] * scores[b, :3] * s["dt"]
        else:
            rot = s["g2_r"] * scores[b, 3:6] * s["dt"] + s["g_r"] * s["sqrt_dt"] * (s["rot_noise"] * f64(z_rot)[b])
            tr = s["g2_t"] * scores[b, :3] * s["dt"] + s["g_t"] * s["sqrt_dt"] * (s["tr_noise"] * f64(z_tr)[b])
        x = lig[b].reshape(-1, 3, 3)
        c = x.reshape(-1, 3).mean(0) if all_atoms else x[:, 1].mean(0)
        Rm = aa_to_mat64(rot)
        out_l[b] = ((x - c) @ Rm.T + c + tr).reshape(lig[b].shape)
        out_t[b] = f64(tr_upd)[b] + tr
        out_r[b] = mat_to_aa64(Rm @ aa_to_mat64(f64(rot_upd)[b]))
        rots[b], trs[b] = rot, tr
    return out_l, out_t, out_r, rots, trs


# ---- the fp32 restatement of k_pair_head_m and its mutants ----------------------------------------------------------------------
MUTANTS = ("drop_sum_w2", "ln_w_block", "swap_rows", "w3_unscaled", "no_eps")


def pair_head_m_fp32(P, Q, ca, R, w_d, ln_w, ln_b, w3, mutant=None):
    """k_pair_head_m's arithmetic in numpy float32 (the same formulas; sums in numpy's order): row moments and the dot product P_r . Q_l
    -> mean, ez2 - mean^2 -> rstd; S y as the five-term sum the MFMA phase forms; SiLU as y' rcp(1 + exp2(y')); w3 / S.
    mutant: None or one of MUTANTS -
      drop_sum_w2  the D^2 sum_w2 term of ez2 left out;
      ln_w_block   channels 96..127 (block 3) take ln_w from block 4;
      swap_rows    a wave's dot products of its ligand rows 8..15 swapped with rows 0..7 (an idle row's product is 0);
      w3_unscaled  w3 not divided by SILU_S;
      no_eps       rstd = 1 / sqrt(var)."""
    f = np.float32
    P, Q, ca = np.asarray(P, f), np.asarray(Q, f), np.asarray(ca, f)
    w_d, ln_w, ln_b, w3 = (np.asarray(x, f) for x in (w_d, ln_w, ln_b, w3))
    B, N = P.shape[:2]
    L = N - R
    Pr, Ql = P[:, :R], Q[:, R:]
    if mutant == "ln_w_block":
        ln_w = ln_w.copy()
        ln_w[96:128] = ln_w[128:160]
    vec = ca[:, :R, None, :3] - ca[:, None, R:, :3]
    D = np.sqrt((vec[..., 0] * vec[..., 0] + vec[..., 1] * vec[..., 1]) + vec[..., 2] * vec[..., 2]).astype(f)
    mP, mP2, mPw = Pr.sum(-1, dtype=f), (Pr * Pr).sum(-1, dtype=f), (Pr * w_d).sum(-1, dtype=f)
    sQ, sQ2, sQw = Ql.sum(-1, dtype=f), (Ql * Ql).sum(-1, dtype=f), (Ql * w_d).sum(-1, dtype=f)
    sum_w, sum_w2 = w_d.sum(dtype=f), (w_d * w_d).sum(dtype=f)
    dot = np.einsum("brc,blc->brl", Pr, Ql).astype(f)
    if mutant == "swap_rows":
        l = np.arange(L)
        li = l % PM_LC
        partner = (l - li) + (li % 4) + 4 * ((li // 4) ^ 8)
        ok = partner < np.minimum(L, (l - li) + PM_LC)
        dot = np.where(ok[None, None, :], dot[:, :, np.where(ok, partner, 0)], f(0))
    if mutant == "drop_sum_w2":
        sum_w2 = f(0)
    inv = f(1.0 / H)
    mean = ((mP[:, :, None] + sQ[:, None, :]) + D * sum_w) * inv
    ez2 = (((mP2[:, :, None] + sQ2[:, None, :]) + f(2) * dot) + D * (f(2) * (mPw[:, :, None] + sQw[:, None, :]) + D * sum_w2)) * inv
    var = np.maximum(ez2 - mean * mean, f(0)) + (f(0) if mutant == "no_eps" else f(LN_EPS))
    rstd = (f(1) / np.sqrt(var)).astype(f)
    lw = SILU_S * ln_w
    P2 = Pr * lw                                        # the tile, scaled in place
    y = (rstd[..., None] * P2[:, :, None, :] + (rstd * D)[..., None] * (lw * w_d)) + (rstd[..., None] * (Ql * lw)[:, None, :, :])
    y = (y + (-mean * rstd)[..., None] * lw) + SILU_S * ln_b
    with np.errstate(over="ignore"):                    # exp2 -> inf -> rcp 0, as on the device
        a = y * (f(1) / (f(1) + np.exp2(y)))
    w3s = w3 if mutant == "w3_unscaled" else w3 * f(1.0 / SILU_S)
    return (a * w3s).sum(-1, dtype=f)


# ---- inputs of the GPU tests ------------------------------------------------------------------------------------------------------
CUT_OFF = 5.0      # on the lattice below D^2 is an integer: D = 5 (3-4-5) and D = 3 (1-2-2) are exact in fp32, every other D at least
                   # 5 - sqrt(24) > 0.1 from the cut-off and 3 - sqrt(8) > 0.17 from the clash distance

PAIR_M_SIZES = ((1, 1), (31, 3), (32, 64), (33, 65), (65, 130), (577, 33))
PAIR_X_SIZES = ((1, 1), (63, 5), (64, 4), (65, 7), (130, 9))
KAPPAS = (1.0, 50.0, 5000.0)


def lattice_coords(rng, B, N, span=6):
    """Centred CA as ca4 [B][N][4] on the integer lattice [-span, span]^3 (w = 0): every squared distance is an integer <= 3 (2 span)^2,
    exact in fp32, so D is the correctly rounded square root and the threshold decisions cannot depend on rounding."""
    ca = np.zeros((B, N, 4), np.float32)
    ca[..., :3] = rng.integers(-span, span + 1, (B, N, 3))
    return ca


def head_weights(rng, wd_scale=2e-2):
    """(w_d, ln_w, ln_b, w3) of one pair head at the generator's scales (dfmdock_amd/weights.py)."""
    return ((rng.standard_normal(H) * wd_scale).astype(np.float32), (1 + 0.1 * rng.standard_normal(H)).astype(np.float32),
            (0.1 * rng.standard_normal(H)).astype(np.float32), (rng.standard_normal(H) / 16).astype(np.float32))


LOW = dict(scale=0.03, wd_scale=2e-3)      # features and distance column small: Var[z] ~ 2e-3, so the LayerNorm eps is 0.5 % of it


def pair_case(R, L, B=2, scale=1.0, kappa=1.0, seed=0, poison=True, wd_scale=2e-2):
    """Inputs of one pair-head launch: P / Q = scale N(0, 1) + a common channel offset chosen for E[z^2] / Var[z] ~ kappa; with `poison`
    the rows the kernel must not read (ligand rows of P, receptor rows of Q) are NaN."""
    rng = np.random.default_rng([seed, R, L])
    N = R + L
    off = np.float32(0.5 * scale * np.sqrt(2.0 * (kappa - 1.0)))
    P = (scale * rng.standard_normal((B, N, H)) + off).astype(np.float32)
    Q = (scale * rng.standard_normal((B, N, H)) + off).astype(np.float32)
    if poison:
        P[:, R:] = np.nan
        Q[:, :R] = np.nan
    w_d, ln_w, ln_b, w3 = head_weights(rng, wd_scale)
    return dict(P=P, Q=Q, ca4=lattice_coords(rng, B, N), w_d=w_d, ln_w=ln_w, ln_b=ln_b, w3=w3, R=R, L=L, B=B)


def pair_m_cases():
    """name -> inputs of every k_pair_head_m launch the GPU tests compare with float64: the six sizes, every second one at the LOW scales
    (the variance is small enough for the LayerNorm eps to matter), and the kappa sweep."""
    out = {}
    for i, (R, L) in enumerate(PAIR_M_SIZES):
        out[f"size_{R}_{L}"] = pair_case(R, L, seed=1, **(LOW if i % 2 else {}))
    for k in KAPPAS:
        out[f"kappa_{k:g}"] = pair_case(33, 65, kappa=k, seed=2)
    return out


def pair_x_cases():
    """name -> inputs of every k_pair_head<1> launch: the five sizes (every second one at the LOW scales) and two with a channel offset."""
    out = {f"size_{R}_{L}": pair_case(R, L, seed=3, **(LOW if i % 2 else {})) for i, (R, L) in enumerate(PAIR_X_SIZES)}
    for k in KAPPAS[1:]:
        out[f"kappa_{k:g}"] = pair_case(65, 7, kappa=k, seed=6)
    return out


def nan_isolation_case():
    return pair_case(33, 65, seed=4)


def nan_cut_off_case():
    return finish_case(70, 40, 8, seed=1)


def energy_case(R, L, B=2, seed=0):
    """k_energy_pairs: enA / enB [B][N][256] (the rows it must not read NaN), lattice coordinates with one pair placed at exactly
    D = cut_off (3-4-5) and one at exactly D = 3 (1-2-2) when there is room."""
    rng = np.random.default_rng([seed, R, L, 7])
    N = R + L
    enA = rng.standard_normal((B, N, H)).astype(np.float32)
    enB = rng.standard_normal((B, N, H)).astype(np.float32)
    enA[:, R:] = np.nan
    enB[:, :R] = np.nan
    ca = lattice_coords(rng, B, N)
    ca[:, R, :3] = ca[:, 0, :3] + np.array([3, 4, 0], np.float32)               # pair (0, 0): D = 5 = cut_off exactly
    if L > 1:
        ca[:, R + 1, :3] = ca[:, 0, :3] + np.array([1, 2, 2], np.float32)       # pair (0, 1): D = 3 exactly
    return dict(enA=enA, enB=enB, ca4=ca, en_ln_w=(1 + 0.1 * rng.standard_normal(H)).astype(np.float32),
                en_ln_b=(0.1 * rng.standard_normal(H)).astype(np.float32), en_w3=(rng.standard_normal(H) / 16).astype(np.float32),
                R=R, L=L, B=B)


ENERGY_SIZES = tuple((R, L) for R in (1, 5) for L in (1, 3, 4, 5, 9))


def all_coordinate_sets():
    """(name, ca4, R) of every GPU case that takes a threshold decision, for the threshold-safety check."""
    out = [("pair_m/" + k, c["ca4"], c["R"]) for k, c in pair_m_cases().items()]
    out += [("pair_x/" + k, c["ca4"], c["R"]) for k, c in pair_x_cases().items()]
    out += [(f"energy/{R}_{L}", energy_case(R, L)["ca4"], R) for R, L in ENERGY_SIZES]
    out += [(f"finish/{R}_{L}", finish_case(R, L, n)["ca4"], R) for R, L, n in FINISH_SIZES]
    out += [("nan_isolation", nan_isolation_case()["ca4"], 33), ("nan_cut_off", nan_cut_off_case()["ca4"], 70)]
    return out


FINISH_SIZES = ((130, 9, 12), (5, 3, 40), (5, 1, 300), (70, 40, 8))      # (R, L, n_part): ls = 2 after the 4 ls > L cut, 1, 1, 2


def finish_case(R, L, n_part, B=2, seed=0):
    """k_pair_finish_s on a synthetic S [B][L][Rp] (pad columns NaN)."""
    rng = np.random.default_rng([seed, R, L, 11])
    Rp = 32 * ((R + 31) // 32)
    S = np.full((B, L, Rp), np.nan, np.float32)
    S[:, :, :R] = rng.standard_normal((B, L, R))
    return dict(S=S, ca4=lattice_coords(rng, B, R + L), R=R, L=L, B=B, Rp=Rp, n_part=n_part)


def heads_weights(seed=0, sat=None):
    """The weights of k_time_embed / k_heads at the generator's scales.  sat = (tr, rot): the last Linear of each scale net replaced
    so that the Softplus pre-activation lands near the given value (LayerNorm weight 0, bias 1 -> SiLU(1) in every channel)."""
    rng = np.random.default_rng([seed, 13])
    w = {"t_W": rng.standard_normal(HI // 2), "t_lin": rng.standard_normal((HI, HI)) / np.sqrt(HI)}
    for n in ("trs", "rots"):
        w[n + "0"] = rng.standard_normal((HI, HI + 1)) / np.sqrt(HI + 1)
        w[n + "_ln_w"] = 1 + 0.1 * rng.standard_normal(HI)
        w[n + "_ln_b"] = 0.1 * rng.standard_normal(HI)
        w[n + "4"] = -0.15 + 0.02 * rng.standard_normal(HI)
    if sat is not None:
        silu1 = 1.0 / (1.0 + np.exp(-1.0))
        for n, target in zip(("trs", "rots"), sat):
            w[n + "_ln_w"] = np.zeros(HI)
            w[n + "_ln_b"] = np.ones(HI)
            w[n + "4"] = np.full(HI, target / (HI * silu1))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in w.items()}
