"""The pair heads (k_pair_head<1>, k_pair_head_m, k_pair_finish_s, k_pair_finish, k_pair_dist) and the score heads (k_energy_pairs,
k_time_embed, k_heads), launch by launch against float64 computed from the same fp32 inputs, through the host shim of
tests/heads_harness.py.  Every bound is relative to the natural scale of its output and is compared with the float64 reference, never
with another run of the kernel.  u = 2^-24.

k_pair_head<1> (heads_harness.pair_head_x_ref): the bound follows the kernel's own order of operations.  A sequential fp32 loop
  s_k = s_(k-1) + t_k rounds each partial sum once: its error is at most u sum_k |s_k| =: seq(t), the partial sums taken in float64 in
  channel order.
    dz    = u (|P + Q| + 4 |w_d| D + |z|)            (the add, the product with D's own 3 u, the second add)
    dmean = (seq(z) + sum dz) / H + u |mean|          d = z - mean: dd = dz + dmean + u |d|
    dvar  = (seq(d^2) + sum (2 |d| dd + u d^2)) / H + u var             rstd: er = dvar / (2 (var + eps)) + 3 u   (add eps, sqrtf, division)
    dy    = |ln_w| rstd (dd + |d| (er + 2 u)) + u |y|
    da    = 1.1 dy + 4 u |a|                          (|SiLU'| <= 1.1; expf 1 ulp, add, IEEE division)
    do    = sum_c (|w3_c| da_c + u |a_c w3_c|) + seq(a w3)
  seq(d^2) is a sum of positive terms: up to 128 u var, so er ~ 64 u - the largest term, and what a sequential loop can really lose.  seq(z)
  grows with |mean| / std = sqrt(kappa - 1), where k_pair_head_m's variance term grows with kappa itself.  On every input used here the
  bound is below k_pair_head_m's, pair by pair; an fp32 restatement of the kernel's loops stays under it, and the five wrong kernels of
  tests/test_heads_harness_cpu.py miss it by 4 x or more (tests/test_heads_harness_cpu.py).  It cannot reject the UNMUTATED moment / exp2 /
  rcp arithmetic at kappa ~ 1, whose error (1.3e-7 of the scale, two roundings) is below what one rounding per channel operation allows.
Tree-reduced three-pass heads (k_pair_dist, k_energy_pairs, the scale MLPs of k_heads): heads_harness.ln_silu_bound / dot_bound.
  With |dz_c| the error of the pre-activation and ns the roundings of one reduction (9 for a 4-term tree or the thread's own value + the
  64-lane butterfly + the four wave sums, 7 for the 128-thread group sum):
    dmean = mean(dz) + (ns + 1) u mean|z|            d = z - mean: dd = dz + dmean + u |d|
    dvar  = 2 mean(|d| dd) + (ns + 2) u var           rstd: er = dvar / (2 (var + eps)) + 3 u
    dy    = |ln_w| rstd (dd + |d| (er + 3 u)) + u |y|
    da    = 1.1 dy + 5 u |a|
    do    = sum_c |w3_c| (da_c + u |a_c|) + nacc u sum_c |a_c w3_c|       (nacc roundings of the output dot: 67 / 9 / 8)
k_pair_head_m (heads_harness.pair_head_m_ref): LayerNorm statistics from row moments.
    dmean = 24 u mean(zabs)                           (moments: 3 + 8 + 8 roundings, the three-term mean, 1 / H, D)
    dez2  = u (24 mean(zabs^2) + 512 mean|P Q|)       (the same sums of squares; P.Q on the fp32 matrix pipe: 128 steps of two products)
    dvar  = dez2 + 2 |mean| dmean + 2 u mean^2        -> er = dvar / (2 (var + eps)) + 3 u: the explicit kappa u term, since
                                                         mean(zabs^2) / (var + eps) >= kappa; rsq 1 ulp
    dy    = |ln_w| rstd (|d| er + dmean) + 12 u T,    T = rstd |ln_w| (zabs + |mean|) + |ln_b|: S y is the sum of five products of rounded
                                                         factors (P'' = S ln_w P, rstd D, ...) accumulated by two MFMAs and an fma
    da    = 1.1 dy + 6 u |a|                          (exp2 1 ulp, add, rcp 1 ulp, product)
    do    = sum_c |w3_c| (da_c + 3 u |a_c|) + 130 u sum_c |a_c w3_c|      (w3 / S; two fma chains of 128 and their sum)
  The bound is linear in er, checked to stay below 0.1.  Tight: tests/test_heads_harness_cpu.py - an fp32 restatement of the kernel stays
  under it on every input used here, five subtly wrong ones miss it by 4 x or more.
Reductions (k_pair_finish_s, k_pair_finish, the partial sums of k_heads): float64 accumulation of fp32 terms, one rounding to fp32 per
  stored partial: 2 u of the sum of |terms|; fp32 force sums of k_pair_finish_s: (R / 64 + 16) u sum_r |unit s| (five roundings per term, the
  lane's running fma, the butterfly, inv_pool).  Counts and clash counts are exact.
k_time_embed: heads_harness.time_embed64 (sinf / cosf 2 ulp, 8 roundings per Linear, sigmoid slope 1 / 4).
The update of k_heads: rot / tr = two or five fp32 operations on the scores (6 u of the sum of |terms|, plus g^2 dt dscore); the pose
  x' = R (x - c) + c + tr with |dR| <= |drot| + 32 u: 2 |x - c|_max (|drot| + 32 u) + |dtr| + 8 u (|x|_max + |c| + |tr|); the composed rotation
  2 |drot| + 256 u (angles stay below 2.5, where the axis-angle of a matrix is well conditioned).

The largest measured |error| / bound of every test goes to $DFM_HEAD_PROFILE/head_kernels_gpu.txt when that variable names a directory
(profiles/head_kernels.txt holds the MI355X figures).
"""
import os

import numpy as np
import pytest

import heads_harness as hh
from heads_harness import Out

pytestmark = pytest.mark.gpu

U = hh.U
H = hh.H
RATIOS = {}


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    harness = hh.Harness(hh.compile_shim(tmp_path_factory.mktemp("heads_harness_gpu")))
    yield harness
    out = os.environ.get("DFM_HEAD_PROFILE")
    if out:
        with open(os.path.join(out, "head_kernels_gpu.txt"), "w") as f:
            f.write("test max_error_over_bound\n" + "".join(f"{k} {v:.4g}\n" for k, v in sorted(RATIOS.items())))


@pytest.fixture(scope="module")
def m_cases():
    return hh.pair_m_cases()


def run(h, op, bufs, **scalars):
    r = h.run(op, bufs, **scalars)
    assert r["err"] == hh.HIP_SUCCESS, f"{op}: hipError {r['err']}"
    for k, v in bufs.items():
        if isinstance(v, Out):
            assert hh.guards_intact(r, k), f"{op}: bytes outside the {k} block changed"
    return r


def check(name, got, ref, bound, key=None):
    """Every element within its bound (NaN fails); records the largest |error| / bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ratio = np.abs(got - ref) / np.broadcast_to(bound, ref.shape)
    worst = float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if ratio.size else 0.0
    k = key or name
    RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
    print(f"{name}: max |err| / bound = {worst:.3g}")
    assert worst <= 1.0, f"{name}: worst |err| / bound = {worst:.3g} at {np.argwhere(~(ratio <= 1.0))[:3].tolist()}"


def head_bufs(c):
    return {k: c[k] for k in ("P", "Q", "ca4", "w_d", "ln_w", "ln_b", "w3")}


def n_part_of(R):
    return 4 * ((R + 63) // 64)


def finish_split(n_part, L, mode):
    """Workgroups per trajectory of k_pair_finish_s: up to 8 (a partial slot per wave, 4 per workgroup of the n_part slots), no more than
    L / 4, one for the confidence."""
    ls = 1 if mode == 2 else min(8, max(1, n_part // 4))
    while ls > 1 and ls * 4 > L:
        ls -= 1
    return ls


def run_head_m(h, c, B=None, sl=slice(None)):
    B = B or c["B"]
    R, L = c["R"], c["L"]
    Rp = 32 * ((R + 31) // 32)
    bufs = {k: (v[sl] if k in ("P", "Q", "ca4") else v) for k, v in head_bufs(c).items()}
    r = run(h, "pair_head_m", dict(bufs, S=Out(np.float32, B * L * Rp)), B=B, R=R, L=L, Rp=Rp)
    return r["S"].reshape(B, L, Rp)


def check_S(name, S, c, key=None):
    R = c["R"]
    s, bound, scale, D, kappa, er = hh.pair_head_m_ref(*[c[k] for k in ("P", "Q", "ca4")], R, c["w_d"], c["ln_w"], c["ln_b"], c["w3"])
    assert float(er.max()) < 0.1
    got = S[:, :, :R].transpose(0, 2, 1)
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} pairs not finite (a poisoned row was read?)"
    assert hh.is_sentinel(S[:, :, R:]).all(), f"{name}: pad columns r >= R were written"
    check(name, got, s, bound, key)
    return s, bound, scale, kappa, got


def finish_s_all_modes(h, name, S, ca4, R, L, n_part, s64=None, s_bound=None):
    """The three modes of k_pair_finish_s on S [B][L][Rp] against float64 reductions of the SAME S; with s64 / s_bound also against the
    float64 head (the head's bound carried through the sums)."""
    B, Rp = S.shape[0], S.shape[2]
    inv_pool = 1.0 / R
    sk = S[:, :, :R].transpose(0, 2, 1)
    fin = hh.finish64(sk, ca4, R, hh.CUT_OFF, inv_pool)
    common = dict(S=S, ca4=ca4)
    sc = dict(B=B, R=R, L=L, Rp=Rp, n_part=n_part, cut_off=hh.CUT_OFF, inv_pool=inv_pool)
    r0 = run(h, "pair_finish_s", dict(common, fvec=Out(np.float32, B * L * 3), clash=Out(np.int32, B * n_part)), mode=0, **sc)
    fb = (R / 64 + 16) * U * fin["fabs"] + 1e-37
    check(name + " fvec", r0["fvec"].reshape(B, L, 3), fin["fvec"], fb, "k_pair_finish_s fvec")
    clash = r0["clash"].reshape(B, n_part)
    used = 4 * finish_split(n_part, L, 0)
    assert (clash.sum(1) == fin["clash"]).all() and (clash[:, used:] == 0).all() and (clash >= 0).all(), name
    r1 = run(h, "pair_finish_s", dict(common, spart=Out(np.float32, B * n_part * 2)), mode=1, **sc)
    sp = r1["spart"].reshape(B, n_part, 2)
    assert not hh.is_sentinel(sp).any() and (sp[:, used:] == 0).all(), f"{name}: the tail slots k_heads sums are not zero"
    check(name + " energy sum", sp[..., 0].astype(np.float64).sum(1), fin["esum"], 2 * U * fin["eabs"] + 1e-37, "k_pair_finish_s energy")
    assert (sp[..., 1].astype(np.float64).sum(1) == fin["count"]).all(), name
    r2 = run(h, "pair_finish_s", dict(common, conf=Out(np.float32, B)), mode=2, **sc)
    check(name + " conf", r2["conf"], fin["conf"], 2 * U * fin["cabs"] + 1e-37, "k_pair_finish_s conf")
    if s64 is not None:
        e2e = hh.finish64(s64, ca4, R, hh.CUT_OFF, inv_pool)
        vec, D = hh.pair_dist64(ca4, R)
        unit = np.abs(vec) / np.maximum(D, 1e-12)[..., None]
        check(name + " fvec vs float64 head", r0["fvec"].reshape(B, L, 3), e2e["fvec"],
              (unit * s_bound[..., None]).sum(1) * inv_pool + (R / 64 + 16) * U * e2e["fabs"] + 1e-37, "k_pair_head_m + finish_s fvec")
        assert (clash.sum(1) == e2e["clash"]).all() and (sp[..., 1].astype(np.float64).sum(1) == e2e["count"]).all()
    return r0, r1, r2


# ---- k_pair_head_m -> k_pair_finish_s ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,L", hh.PAIR_M_SIZES)
def test_pair_head_m_and_finish_s(h, m_cases, R, L):
    """S[b][l][r] for r < R against float64, pad columns untouched, poisoned rows never read; then the three reductions; trajectory 1
    alone gives trajectory 1 of the batch bit for bit."""
    c = m_cases[f"size_{R}_{L}"]
    S = run_head_m(h, c)
    s, bound, _, _, _ = check_S(f"k_pair_head_m {R}x{L}", S, c, "k_pair_head_m sizes")
    finish_s_all_modes(h, f"k_pair_finish_s {R}x{L}", S, c["ca4"], R, L, n_part_of(R), s, bound)
    S1 = run_head_m(h, c, B=1, sl=slice(1, 2))
    assert (S1.view(np.uint32) == S[1:2].view(np.uint32)).all(), "a trajectory's bits depend on the batch"


@pytest.mark.parametrize("kappa", hh.KAPPAS)
def test_pair_head_m_kappa_sweep(h, m_cases, kappa):
    """A common channel offset on P and Q: the moment variance ez2 - mean^2 cancels kappa-fold; the bound's kappa u term covers it."""
    c = m_cases[f"kappa_{kappa:g}"]
    S = run_head_m(h, c)
    s, bound, scale, kap, got = check_S(f"k_pair_head_m kappa {kappa:g}", S, c, f"k_pair_head_m kappa~{kappa:g}")
    rel = float((np.abs(got - s) / scale).max())
    RATIOS[f"k_pair_head_m kappa~{kappa:g}: median kappa {float(np.median(kap)):.4g}, max |err| / sum|SiLU(y) w3|"] = rel
    print(f"kappa {float(np.median(kap)):.4g}: max |err| / scale = {rel:.3g}")


def test_pair_head_m_nan_isolation(h):
    """NaN in receptor row r0 of P -> exactly S[:, :, r0]; NaN in ligand row l0 of Q -> exactly S[:, l0, :]: the LDS tile, the moments and
    the idle MFMA rows do not spread it.  Downstream, the force of every ligand residue that met the NaN is NaN and no other."""
    c = hh.nan_isolation_case()
    R, L = 33, 65
    r0s, l0 = (5, 32), 40
    c["P"][0, r0s[0]] = np.nan
    c["P"][0, r0s[1], 17] = np.nan
    c["Q"][1, R + l0, 200] = np.nan
    S = run_head_m(h, c)[:, :, :R]
    want = np.zeros(S.shape, bool)
    want[0][:, list(r0s)] = True
    want[1][l0, :] = True
    assert (np.isnan(S) == want).all(), f"NaN at {np.argwhere(np.isnan(S) != want)[:4].tolist()}"
    Sp = np.full((2, L, 64), np.nan, np.float32)
    Sp[:, :, :R] = S
    r = run(h, "pair_finish_s", dict(S=Sp, ca4=c["ca4"], fvec=Out(np.float32, 2 * L * 3), clash=Out(np.int32, 2 * 4)), mode=0, B=2, R=R, L=L, Rp=64,
            n_part=4, cut_off=hh.CUT_OFF, inv_pool=1.0 / R)
    f = np.isnan(r["fvec"].reshape(2, L, 3))
    assert f[0].all() and f[1, l0].all() and not np.delete(f[1], l0, 0).any()


def test_finish_s_nan_pair_and_the_cut_off(h):
    """A NaN in S makes mode 0's fvec[l] NaN and mode 1's energy NaN when the pair is inside the cut-off.  A NaN pair OUTSIDE the cut-off
    leaves mode 1 finite: the kernel selects (D < cut_off ? s : nothing) where the reference multiplies, energy * mask, which would give
    NaN.  Pinned as it is; the same evaluation's fvec carries the NaN."""
    c = hh.nan_cut_off_case()
    R, L = c["R"], c["L"]
    D = hh.pair_dist64(c["ca4"], R)[1]
    inside, outside = np.argwhere(D[0] < hh.CUT_OFF)[0], np.argwhere(D[1] > hh.CUT_OFF)[0]
    S = c["S"].copy()
    S[0, inside[1], inside[0]] = np.nan
    S[1, outside[1], outside[0]] = np.nan
    sc = dict(B=2, R=R, L=L, Rp=c["Rp"], n_part=8, cut_off=hh.CUT_OFF, inv_pool=1.0 / R)
    r0 = run(h, "pair_finish_s", dict(S=S, ca4=c["ca4"], fvec=Out(np.float32, 2 * L * 3), clash=Out(np.int32, 16)), mode=0, **sc)
    f = np.isnan(r0["fvec"].reshape(2, L, 3)).all(-1)
    assert f[0, inside[1]] and f[1, outside[1]] and f.sum() == 2
    r1 = run(h, "pair_finish_s", dict(S=S, ca4=c["ca4"], spart=Out(np.float32, 2 * 8 * 2)), mode=1, **sc)
    e = r1["spart"].reshape(2, 8, 2)[..., 0].sum(1)
    assert np.isnan(e[0]) and np.isfinite(e[1])
    fin = hh.finish64(np.where(np.isnan(S), 0, S)[:, :, :R].transpose(0, 2, 1), c["ca4"], R, hh.CUT_OFF, 1.0)
    check("k_pair_finish_s energy beside a NaN outside the cut-off", e[1:], fin["esum"][1:], 2 * U * fin["eabs"][1:] + 1e-37, "k_pair_finish_s energy")


@pytest.mark.parametrize("R,L,n_part", hh.FINISH_SIZES)
def test_finish_s_slot_layout(h, R, L, n_part):
    """The ligand split of launch_pair_finish_s where 4 ls > L cuts it down, and n_part above the slots any split fills (40, 300): the
    n_part slots sum to the reference, the unused ones are zero."""
    c = hh.finish_case(R, L, n_part)
    finish_s_all_modes(h, f"k_pair_finish_s {R}x{L} n_part {n_part}", c["S"], c["ca4"], R, L, n_part)


# ---- k_pair_head<1> -> k_pair_finish ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def x_cases():
    return hh.pair_x_cases()


@pytest.mark.parametrize("name", [f"size_{R}_{L}" for R, L in hh.PAIR_X_SIZES] + [f"kappa_{k:g}" for k in hh.KAPPAS[1:]])
def test_pair_head_exact_and_finish(h, x_cases, name):
    """k_pair_head<1> in its three modes, then k_pair_finish, against float64 with the bound of the kernel's own loop order."""
    c = x_cases[name]
    R, L = c["R"], c["L"]
    B, RT = c["B"], (R + 63) // 64
    inv_pool = 1.0 / R
    s, sb, scale, D = hh.pair_head_x_ref(c["P"], c["Q"], c["ca4"], R, c["w_d"], c["ln_w"], c["ln_b"], c["w3"])
    RATIOS[f"k_pair_head<1> {name}: largest bound / sum|SiLU(y) w3|"] = float((sb / scale).max())
    fin = hh.finish64(s, c["ca4"], R, hh.CUT_OFF, inv_pool)
    vec, _ = hh.pair_dist64(c["ca4"], R)
    unit = np.abs(vec) / np.maximum(D, 1e-12)[..., None]
    sc = dict(B=B, R=R, L=L, cut_off=hh.CUT_OFF, inv_pool=inv_pool)
    r0 = run(h, "pair_head", dict(head_bufs(c), fpart=Out(np.float32, B * RT * L * 3), clash=Out(np.int32, B * RT * 4)), mode=0, **sc)
    assert (r0["clash"].reshape(B, -1).sum(1) == fin["clash"]).all()
    rf = run(h, "pair_finish", dict(fpart=r0["fpart"], fvec=Out(np.float32, B * L * 3)), **sc)
    check(f"k_pair_head<1> {R}x{L} fvec", rf["fvec"].reshape(B, L, 3), fin["fvec"],
          (unit * sb[..., None]).sum(1) * inv_pool + 16 * U * fin["fabs"] + 1e-37, "k_pair_head<1> + k_pair_finish fvec")
    r1 = run(h, "pair_head", dict(head_bufs(c), spart=Out(np.float32, B * RT * 4 * 2)), mode=1, **sc)
    sp = r1["spart"].reshape(B, RT * 4, 2).astype(np.float64)
    mask = D < hh.CUT_OFF
    check(f"k_pair_head<1> {R}x{L} energy sum", sp[..., 0].sum(1), fin["esum"], np.where(mask, sb, 0).sum((1, 2)) + 2 * U * fin["eabs"] + 1e-37,
          "k_pair_head<1> energy")
    assert (sp[..., 1].sum(1) == fin["count"]).all()
    r2 = run(h, "pair_head", dict(head_bufs(c), spart=Out(np.float32, B * RT * 4 * 2)), mode=2, **sc)
    rc = run(h, "pair_finish", dict(spart=r2["spart"], conf=Out(np.float32, B)), **sc)
    check(f"k_pair_head<1> {R}x{L} conf", rc["conf"], fin["conf"], sb.mean((1, 2)) + 2 * U * fin["cabs"] + 1e-37, "k_pair_head<1> + k_pair_finish conf")


@pytest.mark.parametrize("R,L", [(3, 5), (1, 1)])
def test_pair_dist(h, R, L):
    c = hh.pair_case(R, L, seed=5)
    w3t = (np.random.default_rng(5).standard_normal((H, 64)) / 16).astype(np.float32)
    ref, bound, _, _ = hh.pair_head_exact_ref(c["P"], c["Q"], c["ca4"], R, c["w_d"], c["ln_w"], c["ln_b"], w3t, ns=9, nacc=67)
    r = run(h, "pair_dist", dict(head_bufs(c), w3=w3t, dist=Out(np.float32, 2 * R * L * 64)), B=2, R=R, L=L)
    check(f"k_pair_dist {R}x{L}", r["dist"].reshape(2, R, L, 64), ref, bound, "k_pair_dist")


# ---- k_energy_pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,L", hh.ENERGY_SIZES)
def test_energy_pairs(h, R, L):
    """Masked energy sums, counts and clash counts per receptor residue; the pair at exactly D == cut_off is out, the pair at exactly
    D == 3 is a clash (the inputs place both: test_heads_harness_cpu.py); want_energy = 0 leaves the sums zero and the counts as they are."""
    c = hh.energy_case(R, L)
    B = c["B"]
    D = hh.pair_dist64(c["ca4"], R)[1]
    assert (D[:, 0, 0] == hh.CUT_OFF).all()
    z = hh.f64(c["enA"])[:, :R, None, :] + hh.f64(c["enB"])[:, None, R:, :]
    a, da = hh.ln_silu_bound(z, U * np.abs(z), c["en_ln_w"], c["en_ln_b"], ns=9)
    e, de, eabs = hh.dot_bound(a, da, c["en_w3"], 9)
    mask = D < hh.CUT_OFF
    bufs = {k: c[k] for k in ("enA", "enB", "ca4", "en_ln_w", "en_ln_b", "en_w3")}
    for want in (1, 0):
        r = run(h, "energy_pairs", dict(bufs, spart=Out(np.float32, B * R * 2), clash=Out(np.int32, B * R)), B=B, R=R, L=L, cut_off=hh.CUT_OFF,
                want_energy=want)
        sp = r["spart"].reshape(B, R, 2)
        assert (sp[..., 1] == mask.sum(2)).all() and (r["clash"].reshape(B, R) == (D <= 3.0).sum(2)).all()
        if want:
            check(f"k_energy_pairs {R}x{L}", sp[..., 0], np.where(mask, e, 0).sum(2), np.where(mask, de + 2 * U * eabs, 0).sum(2) + 1e-37,
                  "k_energy_pairs")
        else:
            assert (sp[..., 0] == 0).all()


# ---- k_time_embed -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [(0.5,), (0.0, 1e-3, 1.0)], ids=["n1", "n3"])
def test_time_embed(h, t):
    w = hh.heads_weights(2)
    t = np.array(t, np.float32)
    base, dbase = hh.time_embed64(t, w)
    r = run(h, "time_embed", dict({k: w[k] for k in hh.HEAD_W}, t=t, base=Out(np.float32, len(t) * 256)), n_times=len(t))
    check(f"k_time_embed n {len(t)}", r["base"].reshape(len(t), 2, 128), base, dbase + 1e-37, "k_time_embed")


# ---- k_heads ----------------------------------------------------------------------------------------------------------------------
STEP = dict(g2_r=1.69, g_r=1.3, hg2_r=0.845, g2_t=4.41, g_t=2.1, hg2_t=2.205, dt=0.025, sqrt_dt=float(np.sqrt(0.025)), rot_noise=0.5,
            tr_noise=0.5, step=7)
NAN_STEP = dict({k: np.nan for k in hh.STEP_FIELDS}, step=0xffffffff)


def heads_inputs(L, B=3, R=5, n_part=40, seed=0, sat=None, zero_f=False, shared_t=False):
    rng = np.random.default_rng([seed, L, 17])
    w = hh.heads_weights(seed, sat)
    base = hh.time_embed64(np.array([0.4] if shared_t else rng.uniform(0.05, 1, B), np.float32), w)[0].astype(np.float32)
    fvec = np.zeros((B, L, 3), np.float32) if zero_f else rng.standard_normal((B, L, 3)).astype(np.float32)
    en = np.zeros((B, n_part, 2), np.float32)
    en[..., 0] = rng.standard_normal((B, n_part))
    en[..., 1] = rng.integers(0, 50, (B, n_part))
    en[0, :, 1] = 0                                               # a trajectory without a pair inside the cut-off
    clash = rng.integers(0, 9, (B, n_part)).astype(np.int32)
    return dict(w=w, base=base, fvec=fvec, ca4=hh.lattice_coords(rng, B, R + L), en=en, clash=clash, B=B, R=R, L=L, n_part=n_part)


def heads_bufs(x):
    return dict({k: x["w"][k] for k in hh.HEAD_W}, fvec=x["fvec"], ca4=x["ca4"], base=x["base"], spart=x["en"], clash=x["clash"])


@pytest.mark.parametrize("L", [1, 85, 86, 257])
@pytest.mark.parametrize("mean_pool,en_mode,n_part,shared_t", [(True, 0, 40, False), (False, 1, 300, True), (True, 2, 40, True)])
def test_heads_scores(h, L, mean_pool, en_mode, n_part, shared_t):
    """Scores, energy in its three modes (one trajectory has a zero pair count) and clash total; pooling by L and by 1; n_part 40 and 300;
    hid_bstride 256 and 0; trace_scores at its stride."""
    x = heads_inputs(L, n_part=n_part, shared_t=shared_t)
    B, R = x["B"], x["R"]
    pool = float(L) if mean_pool else 1.0
    base = np.repeat(x["base"], B, 0) if shared_t else x["base"]
    ref, bound, _ = hh.heads64(x["fvec"], x["ca4"], R, x["w"], base, pool, x["en"], x["clash"], en_mode)
    r = run(h, "heads", dict(heads_bufs(x), scores=Out(np.float32, B * 8), trace_scores=Out(np.float32, B * 24)), B=B, R=R, L=L, n_part=n_part,
            want_energy=1, en_mode=en_mode, pool_div=pool, hid_bstride=0 if shared_t else 256, trace_s_bstride=24)
    sc = r["scores"].reshape(B, 8)
    check(f"k_heads scores L {L} en_mode {en_mode}", sc[:, :7], ref[:, :7], bound[:, :7], "k_heads scores")
    assert (sc[:, 7] == ref[:, 7]).all() and np.isfinite(sc).all()
    tr = r["trace_scores"].reshape(B, 24)
    assert (tr[:, :8].view(np.uint32) == sc.view(np.uint32)).all() and hh.is_sentinel(tr[:, 8:]).all()


@pytest.mark.parametrize("sat", [(25.0, -60.0), (-60.0, 25.0), (0.0, 0.3)])
def test_heads_softplus_branches(h, sat):
    """Softplus(threshold 20): pre-activation > 20 (identity), ~ 0 and < -50 (exp alone: no underflow to zero, no log of 1)."""
    x = heads_inputs(9, sat=sat, seed=1)
    ref, bound, pre = hh.heads64(x["fvec"], x["ca4"], x["R"], x["w"], x["base"], 9.0)
    assert np.allclose(pre, np.array(sat)[None], atol=1e-3)
    r = run(h, "heads", dict(heads_bufs(x), scores=Out(np.float32, 24)), B=3, R=5, L=9, n_part=40, want_energy=0, pool_div=9.0, hid_bstride=256)
    sc = r["scores"].reshape(3, 8)
    check(f"k_heads softplus {sat}", sc[:, :6], ref[:, :6], bound[:, :6], "k_heads softplus branches")
    assert (sc[:, :6] != 0).all() and (sc[:, 6:] == 0).all()


def test_heads_zero_force(h):
    """fvec == 0: the norms are 0 and the scores exactly 0 (pred / (0 + 1e-6)), not NaN."""
    x = heads_inputs(9, zero_f=True)
    r = run(h, "heads", dict(heads_bufs(x), scores=Out(np.float32, 24)), B=3, R=5, L=9, n_part=40, want_energy=1, pool_div=9.0, hid_bstride=256)
    assert (r["scores"].reshape(3, 8)[:, :6] == 0).all()


def update_launch(h, x, lig, rot0, tr0, z, ode, all_atoms, rec_pos=None, ctl=None, params=None, base=None, scalars=STEP, seed=11):
    B, R, L = x["B"], x["R"], x["L"]
    N = R + L
    bufs = dict(heads_bufs(x), scores=Out(np.float32, B * 8), z_rot=None if z is None else z[0], z_tr=None if z is None else z[1], lig=Out(np.float32, init=lig),
                tr_upd=Out(np.float32, init=tr0), rot_upd=Out(np.float32, init=rot0), trace_pose=Out(np.float32, B * 2 * L * 9))
    if base is not None:
        bufs["base"] = base
    if rec_pos is not None:
        bufs.update(rec_pos=rec_pos, prep_pos=Out(np.float32, B * N * 4), prep_ca4=Out(np.float32, B * N * 4), prep_cb4=Out(np.float32, B * N * 4))
    if ctl is not None:
        bufs.update(ctl=ctl, step_params=params)
    fl = {k: float(scalars[k]) for k in hh.STEP_FIELDS}
    return run(h, "heads", bufs, B=B, R=R, L=L, n_part=x["n_part"], want_energy=1, en_mode=1, pool_div=float(L), hid_bstride=0 if ctl is not None else 256,
               do_update=1, ode=ode, all_atoms=all_atoms, z_bstride=6, trace_bstride=2 * L * 9, prep_next=int(rec_pos is not None),
               step=int(scalars["step"]) & 0x7fffffff, seed=seed, **fl)


def update_inputs(x, seed=0):
    rng = np.random.default_rng([seed, 19])
    B, R, L = x["B"], x["R"], x["L"]
    lig = (rng.standard_normal((B, L, 9)) * 6 + 2).astype(np.float32)
    z = np.full((2, B, 6), np.nan, np.float32)                    # z_bstride 6: the gaps are never read
    z[:, :, :3] = rng.standard_normal((2, B, 3))
    rot0 = np.array([[0.3, -0.2, 0.5], [0.0, 0.0, 0.0], [-0.7, 0.4, 0.1]], np.float32)[:B]
    tr0 = rng.standard_normal((B, 3)).astype(np.float32) * 3
    rec_pos = (rng.standard_normal((R, 9)) * 6).astype(np.float32)
    return lig, rot0, tr0, z, rec_pos


@pytest.mark.parametrize("L,ode,all_atoms", [(86, 0, 0), (86, 0, 1), (86, 1, 0), (86, 1, 1), (1, 0, 0), (1, 1, 1), (85, 0, 1), (85, 1, 0),
                                             (257, 0, 0), (257, 1, 1)])
def test_heads_update(h, L, ode, all_atoms):
    """The Euler-Maruyama / axis-angle update with injected draws against the float64 replay: pose, tr_update, a rot_update that starts
    non-zero; trace_pose at its stride; prep_next equals launch_prep_pose run on the updated pose, bit for bit.  The update loop covers
    3 L atoms with 256 threads: L = 1 (3 atoms), 85 (255: one idle thread), 86 (258: two passes), 257 (771: four passes, and two of the
    CA-centroid loop)."""
    x = heads_inputs(L, seed=2)
    B, R, L = x["B"], x["R"], x["L"]
    N = R + L
    lig, rot0, tr0, z, rec_pos = update_inputs(x)
    r = update_launch(h, x, lig, rot0, tr0, z, ode, all_atoms, rec_pos)
    sref, sb, _ = hh.heads64(x["fvec"], x["ca4"], R, x["w"], x["base"], float(L), x["en"], x["clash"], 1)
    check("k_heads scores (update launch)", r["scores"].reshape(B, 8)[:, :7], sref[:, :7], sb[:, :7], "k_heads scores")
    nl, nt, nr, rot, tr = hh.update64(sref, lig, rot0, tr0, STEP, z[0][:, :3], z[1][:, :3], ode, all_atoms)
    g2dt = np.array([STEP["g2_t"], STEP["g2_r"]]) * STEP["dt"]
    dtr = g2dt[0] * sb[:, :3].max(1) + 6 * U * (np.abs(tr).max(1) + 1)
    drot = g2dt[1] * np.linalg.norm(sb[:, 3:6], axis=1) + 6 * U * (np.linalg.norm(rot, axis=1) + 1)
    x3 = lig.reshape(B, -1, 3).astype(np.float64)
    cen = x3.mean(1) if all_atoms else lig.reshape(B, L, 3, 3)[:, :, 1].astype(np.float64).mean(1)
    rad = np.linalg.norm(x3 - cen[:, None], axis=-1).max(1)
    dpose = 2 * rad * (drot + 32 * U) + dtr + 8 * U * (np.abs(x3).max((1, 2)) + np.abs(cen).max(1) + np.abs(tr).max(1))
    tag = f"L {L} ode {ode} all_atoms {all_atoms}"
    got = r["lig"].reshape(B, L * 9)
    check(f"k_heads pose {tag}", got, nl.reshape(B, L * 9), dpose[:, None], "k_heads update pose")
    check(f"k_heads tr_update {tag}", r["tr_upd"].reshape(B, 3), nt, (dtr + 2 * U * (np.abs(tr0).max(1) + np.abs(tr).max(1)))[:, None], "k_heads tr_update")
    check(f"k_heads rot_update {tag}", r["rot_upd"].reshape(B, 3), nr, (2 * drot + 256 * U)[:, None], "k_heads rot_update")
    tp = r["trace_pose"].reshape(B, 2 * L * 9)
    assert (tp[:, :L * 9].view(np.uint32) == got.view(np.uint32)).all() and hh.is_sentinel(tp[:, L * 9:]).all()
    pp = run(h, "prep_pose", dict(rec_pos=rec_pos, lig=r["lig"], prep_pos=Out(np.float32, B * N * 4), prep_ca4=Out(np.float32, B * N * 4),
                                  prep_cb4=Out(np.float32, B * N * 4)), B=B, R=R, L=L, all_atoms=all_atoms)
    for k in ("prep_pos", "prep_ca4", "prep_cb4"):
        assert not hh.is_sentinel(r[k]).any() and (r[k].view(np.uint32) == pp[k].view(np.uint32)).all(), k


def test_heads_replayed_step_indexing(h):
    """ctl[0] = 3: the step's scalars are step_params[2] and its time embedding hid_base + 2 * 256, for every trajectory; the by-value
    scalars and every other entry are NaN.  The launch equals, bit for bit, the direct launch given entry 2's scalars."""
    x = heads_inputs(9, seed=3, shared_t=True)
    lig, rot0, tr0, z, _ = update_inputs(x, seed=1)
    # (the direct launch reads hid_base with stride 256 per trajectory: give it one copy of the entry each)
    x3 = dict(x, base=np.repeat(x["base"], 3, 0))
    direct = update_launch(h, x3, lig, rot0, tr0, z, 0, 0)
    base4 = np.full((4, 2, 128), np.nan, np.float32)
    base4[2] = x["base"][0]
    params = hh.step_params([NAN_STEP, NAN_STEP, STEP, NAN_STEP])
    ctl = np.array([3, 11, 0], np.uint32)
    rep = update_launch(h, x, lig, rot0, tr0, z, 0, 0, ctl=ctl, params=params, base=base4, scalars=NAN_STEP)
    for k in ("scores", "lig", "tr_upd", "rot_upd"):
        assert np.isfinite(rep[k]).all(), k
        assert (rep[k].view(np.uint32) == direct[k].view(np.uint32)).all(), k


def test_heads_replayed_step_draws(h):
    """The same with the kernel's own draws (no injected z): the Philox counter takes step_params[2].step and the key ctl[1], ctl[2].
    The by-value seed and step of the replayed launch are different numbers; the launch still equals the direct one bit for bit, and a
    direct launch at another step or with the seed words swapped does not."""
    x = heads_inputs(9, seed=3, shared_t=True)
    lig, rot0, tr0, _, _ = update_inputs(x, seed=1)
    x3 = dict(x, base=np.repeat(x["base"], 3, 0))
    seed = 0x1234567890
    direct = update_launch(h, x3, lig, rot0, tr0, None, 0, 0, seed=seed)
    base4 = np.full((4, 2, 128), np.nan, np.float32)
    base4[2] = x["base"][0]
    params = hh.step_params([NAN_STEP, NAN_STEP, STEP, NAN_STEP])
    ctl = np.array([3, seed & 0xffffffff, seed >> 32], np.uint32)
    rep = update_launch(h, x, lig, rot0, tr0, None, 0, 0, ctl=ctl, params=params, base=base4, scalars=NAN_STEP, seed=0xdeadbeef)
    other_step = update_launch(h, x3, lig, rot0, tr0, None, 0, 0, seed=seed, scalars=dict(STEP, step=8))
    swapped = update_launch(h, x3, lig, rot0, tr0, None, 0, 0, seed=((seed & 0xffffffff) << 32) | (seed >> 32))
    for k in ("lig", "tr_upd", "rot_upd"):
        assert np.isfinite(rep[k]).all(), k
        assert (rep[k].view(np.uint32) == direct[k].view(np.uint32)).all(), k
        assert (other_step[k] != direct[k]).any() and (swapped[k] != direct[k]).any(), k


# ---- non-finite poses (include/dfmdock_amd.h: contained, visible) ------------------------------------------------------------------------
def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("all_atoms", (0, 1))
@pytest.mark.parametrize("where,value", [((40, 0), np.nan), ((40, 4), np.nan), ((85, 8), np.inf), ((0, 3), -np.inf)],
                         ids=["nan_in_N", "nan_in_CA", "inf_in_C", "neg_inf_in_CA"])
def test_prep_pose_non_finite(h, where, value, all_atoms):
    """One NaN or infinite coordinate in ANY backbone atom of pose 1 of B = 3 (an N atom: without the mark the CA centroid, every CA and so
    every distance of the pose stayed finite and only angle bins went to 0): every prepared coordinate of that pose is NaN on all three
    axes, w stays 0, and poses 0 and 2 have the bits of the launch with pose 1 finite."""
    B, R, L = 3, 5, 86
    N = R + L
    rng = np.random.default_rng([L, 23])
    rec_pos = (rng.standard_normal((R, 9)) * 6).astype(np.float32)
    lig = (rng.standard_normal((B, L, 9)) * 6 + 2).astype(np.float32)
    bad = lig.copy()
    bad[1, where[0], where[1]] = value
    out = lambda: dict(prep_pos=Out(np.float32, B * N * 4), prep_ca4=Out(np.float32, B * N * 4), prep_cb4=Out(np.float32, B * N * 4))
    good = run(h, "prep_pose", dict(rec_pos=rec_pos, lig=lig, **out()), B=B, R=R, L=L, all_atoms=all_atoms)
    r = run(h, "prep_pose", dict(rec_pos=rec_pos, lig=bad, **out()), B=B, R=R, L=L, all_atoms=all_atoms)
    for k in ("prep_pos", "prep_ca4", "prep_cb4"):
        g, x = good[k].reshape(B, N, 4), r[k].reshape(B, N, 4)
        assert np.isfinite(g).all()
        assert same_bits(x[[0, 2]], g[[0, 2]]), f"{k}: another pose's bits changed"
        assert np.isnan(x[1, :, :3]).all() and (x[1, :, 3] == 0).all(), f"{k}: the non-finite pose has numbers among its prepared coordinates"


def test_energy_pairs_non_finite(h):
    """Trajectory 1 of B = 3 as k_prep_pose leaves a non-finite pose (every CA NaN) and NaN activations: no pair passes D < cut_off or
    D <= 3, so its sums, counts and clash counts are exactly 0 - the kernel alone would report a pose out of contact; k_heads turns that
    energy into NaN (test_heads_non_finite) and num_clashes is documented as 0.  The other trajectories keep their bits."""
    R, L = hh.ENERGY_SIZES[-1]
    c = hh.energy_case(R, L, B=3)
    bufs = {k: c[k] for k in ("enA", "enB", "ca4", "en_ln_w", "en_ln_b", "en_w3")}
    out = lambda: dict(spart=Out(np.float32, 3 * R * 2), clash=Out(np.int32, 3 * R))
    good = run(h, "energy_pairs", dict(bufs, **out()), B=3, R=R, L=L, cut_off=hh.CUT_OFF, want_energy=1)
    bad = dict(bufs, ca4=bufs["ca4"].copy(), enA=bufs["enA"].copy(), enB=bufs["enB"].copy())
    bad["ca4"][1, :, :3] = np.nan
    bad["enA"][1] = np.nan
    bad["enB"][1] = np.nan
    r = run(h, "energy_pairs", dict(bad, **out()), B=3, R=R, L=L, cut_off=hh.CUT_OFF, want_energy=1)
    sp, sg = r["spart"].reshape(3, R, 2), good["spart"].reshape(3, R, 2)
    assert same_bits(sp[[0, 2]], sg[[0, 2]]) and (r["clash"].reshape(3, R)[[0, 2]] == good["clash"].reshape(3, R)[[0, 2]]).all()
    assert (sp[1] == 0).all() and (r["clash"].reshape(3, R)[1] == 0).all()
    assert (sg[1, :, 1] > 0).any(), "the finite pose has pairs inside the cut-off"


@pytest.mark.parametrize("en_mode", (0, 1, 2))
def test_heads_non_finite(h, en_mode):
    """k_heads on B = 3 with trajectory 1 non-finite as the kernels before it leave it: every prepared CA NaN, the force NaN, the energy
    parts those of k_energy_pairs / k_pair_finish_s for a pose no pair of which passes the cut-off (sums and counts 0).  Its tr_score,
    rot_score AND energy are NaN - not 0 / 1e-6, the energy of a pose out of contact -, num_clashes is 0; trajectories 0 and 2 have the
    bits of the launch with trajectory 1 finite."""
    L = 86
    x = heads_inputs(L, n_part=40)
    B, R = x["B"], x["R"]
    kw = dict(B=B, R=R, L=L, n_part=40, want_energy=1, en_mode=en_mode, pool_div=float(L), hid_bstride=256, trace_s_bstride=24)
    out = lambda: dict(scores=Out(np.float32, B * 8), trace_scores=Out(np.float32, B * 24))
    good = run(h, "heads", dict(heads_bufs(x), **out()), **kw)["scores"].reshape(B, 8)
    y = dict(x, fvec=x["fvec"].copy(), ca4=x["ca4"].copy(), en=x["en"].copy(), clash=x["clash"].copy())
    y["fvec"][1] = np.nan
    y["ca4"][1, :, :3] = np.nan
    y["en"][1] = 0
    y["clash"][1] = 0
    r = run(h, "heads", dict(heads_bufs(y), **out()), **kw)
    sc = r["scores"].reshape(B, 8)
    assert np.isfinite(good).all() and same_bits(sc[[0, 2]], good[[0, 2]])
    assert np.isnan(sc[1, :7]).all(), f"finite outputs of a non-finite pose: {sc[1]}"
    assert sc[1, 7] == 0
    assert same_bits(r["trace_scores"].reshape(B, 24)[:, :8][[0, 2]], good[[0, 2]]) and np.isnan(r["trace_scores"].reshape(B, 24)[1, :7]).all()


def test_heads_update_non_finite(h):
    """The update launch (with prep_next) on the same batch: the non-finite trajectory's pose, tr_update, rot_update and prepared
    coordinates are NaN, the others' bits are those of the launch with trajectory 1 finite."""
    L = 86
    x = heads_inputs(L, seed=2)
    B, R = x["B"], x["R"]
    lig, rot0, tr0, z, rec_pos = update_inputs(x)
    good = update_launch(h, x, lig, rot0, tr0, z, 0, 0, rec_pos)
    y = dict(x, fvec=x["fvec"].copy(), ca4=x["ca4"].copy(), en=x["en"].copy(), clash=x["clash"].copy())
    y["fvec"][1] = np.nan
    y["ca4"][1, :, :3] = np.nan
    y["en"][1] = 0
    y["clash"][1] = 0
    lb = lig.copy()
    lb[1, 40, 4] = np.nan
    r = update_launch(h, y, lb, rot0, tr0, z, 0, 0, rec_pos)
    for k, shape in (("lig", (B, L * 9)), ("tr_upd", (B, 3)), ("rot_upd", (B, 3)), ("prep_pos", (B, -1)), ("prep_ca4", (B, -1)), ("prep_cb4", (B, -1)),
                     ("scores", (B, 8))):
        a, g = r[k].reshape(shape), good[k].reshape(shape)
        assert same_bits(a[[0, 2]], g[[0, 2]]), k
    assert np.isnan(r["lig"].reshape(B, L * 9)[1]).all() and np.isnan(r["tr_upd"].reshape(B, 3)[1]).all() and np.isnan(r["rot_upd"].reshape(B, 3)[1]).all()
    for k in ("prep_pos", "prep_ca4", "prep_cb4"):
        assert np.isnan(r[k].reshape(B, R + L, 4)[1, :, :3]).all(), k
    assert np.isnan(r["scores"].reshape(B, 8)[1, :7]).all()


def pair_batch3(c):
    """A pair-head case as B = 3 (trajectory 0 once more as the third) and the same with trajectory 1 non-finite: CA NaN, P and Q NaN."""
    pick = [0, 1, 0]
    good = dict(c, **{k: np.ascontiguousarray(c[k][pick]) for k in ("P", "Q", "ca4")}, B=3)
    bad = dict(good, **{k: good[k].copy() for k in ("P", "Q", "ca4")})
    bad["ca4"][1, :, :3] = np.nan
    bad["P"][1] = np.nan
    bad["Q"][1] = np.nan
    return good, bad


def test_pair_heads_non_finite(h, m_cases, x_cases):
    """k_pair_head_m (+ k_pair_finish_s), k_pair_head<1> (+ k_pair_finish) and k_pair_dist with trajectory 1 of B = 3 non-finite: the
    other two keep their bits in every output; the bad one's S, force and distance logits are NaN; its masked energy sums and counts and
    its clash count are 0 (no pair passes D < cut_off: k_heads makes the energy NaN)."""
    R, L = hh.PAIR_M_SIZES[3]      # 33 x 65: a partial 32-row tile and a partial ligand tile
    good, bad = pair_batch3(m_cases[f"size_{R}_{L}"])
    Sg, Sb = run_head_m(h, good, B=3), run_head_m(h, bad, B=3)
    assert same_bits(Sb[[0, 2]], Sg[[0, 2]]) and np.isnan(Sb[1, :, :R]).all()
    n_part = n_part_of(R)
    sc = dict(B=3, R=R, L=L, Rp=Sg.shape[2], n_part=n_part, cut_off=hh.CUT_OFF, inv_pool=1.0 / R)
    for S, ca4, tag in ((Sg, good["ca4"], "good"), (Sb, bad["ca4"], "bad")):
        r0 = run(h, "pair_finish_s", dict(S=S, ca4=ca4, fvec=Out(np.float32, 3 * L * 3), clash=Out(np.int32, 3 * n_part)), mode=0, **sc)
        r1 = run(h, "pair_finish_s", dict(S=S, ca4=ca4, spart=Out(np.float32, 3 * n_part * 2)), mode=1, **sc)
        if tag == "good":
            f0, c0, s0 = r0["fvec"].reshape(3, L, 3), r0["clash"].reshape(3, n_part), r1["spart"].reshape(3, n_part, 2)
        else:
            f1, c1, s1 = r0["fvec"].reshape(3, L, 3), r0["clash"].reshape(3, n_part), r1["spart"].reshape(3, n_part, 2)
    assert same_bits(f1[[0, 2]], f0[[0, 2]]) and (c1[[0, 2]] == c0[[0, 2]]).all() and same_bits(s1[[0, 2]], s0[[0, 2]])
    assert np.isnan(f1[1]).all() and (c1[1] == 0).all() and (s1[1] == 0).all()
    # k_pair_head<1>
    name = f"size_{hh.PAIR_X_SIZES[3][0]}_{hh.PAIR_X_SIZES[3][1]}"      # 65 x 7: two receptor tiles
    good, bad = pair_batch3(x_cases[name])
    R, L = good["R"], good["L"]
    RT = (R + 63) // 64
    sc = dict(B=3, R=R, L=L, cut_off=hh.CUT_OFF, inv_pool=1.0 / R)
    res = {}
    for tag, c in (("good", good), ("bad", bad)):
        r0 = run(h, "pair_head", dict(head_bufs(c), fpart=Out(np.float32, 3 * RT * L * 3), clash=Out(np.int32, 3 * RT * 4)), mode=0, **sc)
        rf = run(h, "pair_finish", dict(fpart=r0["fpart"], fvec=Out(np.float32, 3 * L * 3)), **sc)
        r1 = run(h, "pair_head", dict(head_bufs(c), spart=Out(np.float32, 3 * RT * 4 * 2)), mode=1, **sc)
        res[tag] = (rf["fvec"].reshape(3, L, 3), r0["clash"].reshape(3, -1), r1["spart"].reshape(3, -1, 2))
    (f0, c0, s0), (f1, c1, s1) = res["good"], res["bad"]
    assert same_bits(f1[[0, 2]], f0[[0, 2]]) and (c1[[0, 2]] == c0[[0, 2]]).all() and same_bits(s1[[0, 2]], s0[[0, 2]])
    assert np.isnan(f1[1]).all() and (c1[1] == 0).all() and (s1[1] == 0).all()
    # k_pair_dist
    c = hh.pair_case(3, 5, seed=5)
    good, bad = pair_batch3(dict(c, R=3, L=5))
    w3t = (np.random.default_rng(5).standard_normal((H, 64)) / 16).astype(np.float32)
    d0 = run(h, "pair_dist", dict(head_bufs(good), w3=w3t, dist=Out(np.float32, 3 * 3 * 5 * 64)), B=3, R=3, L=5)["dist"].reshape(3, -1)
    d1 = run(h, "pair_dist", dict(head_bufs(bad), w3=w3t, dist=Out(np.float32, 3 * 3 * 5 * 64)), B=3, R=3, L=5)["dist"].reshape(3, -1)
    assert same_bits(d1[[0, 2]], d0[[0, 2]]) and np.isnan(d1[1]).all() and np.isfinite(d0).all()
