"""Kernel-level harness of the five launchers the other harnesses leave out (tests/kernels/aux_harness.hip): launch_pair_dist_sum
(k_pair_dist_sum + k_dist_finish + k_dist_mean), launch_restraint (k_restraint), launch_symmetry (k_symmetry), launch_igso3_cdf and
launch_start_pose.

The shim drives the shipped launchers of dfmdock_amd/libdfmdock_amd.so under the guard-band protocol of tests/kernel_harness.py, after
checking everything a kernel would follow as an index.  This module binds it and holds
  * the float64 references, written from the definitions and not from the kernels: heads_harness.pair_z64 / layernorm64 / silu64, then
    W3 and distogram.pair_maps / pose_scores / pcontact_mean; restraints.evaluate / apply_step; refine.inverse_cdf / forward_marginal and
    the IGSO(3) table of refine.igso3_cdf in extended precision;
  * the bounds of each kernel relative to those references (derivations: the docstring of tests/test_gpu_aux_kernels.py);
  * a numpy fp32 restatement of k_pair_dist_sum with nine seeded mutants and restatements of the restraint arg-min and of the
    first-crossing rule with theirs, with which tests/test_aux_harness_cpu.py shows that the comparisons have power;
  * the input generators of the GPU tests, so that the CPU tests can check conditions on the very inputs the GPU tests use.
"""
import ctypes as C
import functools
import math

import numpy as np

import geom_harness as gh
import heads_harness as hh
import kernel_harness as kh
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, LIBDIR, ROOT, Out, guards_intact, is_sentinel      # noqa: F401 (re-exported)

from dfmdock_amd import distogram as DG
from dfmdock_amd import refine as RF
from dfmdock_amd import restraints as RS
from dfmdock_amd import symmetry as SY

LAUNCHERS = ("_ZN3dfm20launch_pair_dist_sumERKNS_15PairDistSumArgsEP12ihipStream_t",
             "_ZN3dfm16launch_restraintERKNS_13RestraintArgsEiP12ihipStream_t",
             "_ZN3dfm15launch_symmetryERKNS_12SymmetryArgsEiP12ihipStream_t",
             "_ZN3dfm16launch_igso3_cdfEdPdP12ihipStream_t",
             "_ZN3dfm17launch_start_poseERKNS_9StartArgsEiP12ihipStream_t")
H = hh.H
U = hh.U                          # unit roundoff of fp32
E64 = 2.0 ** -53                  # unit roundoff of float64
SILU_S = hh.SILU_S
PM_RT, PM_LC, PM_LW = 32, 64, 16  # k_pair_dist_sum: receptor x ligand residues of a workgroup, ligand rows of a wave
RS_SMALL, RS_MAX_GROUPS = 16, 4096
IGSO3_N = 1000
RNG_START = 4

SLOTS = ("P", "Q", "ca4", "w_d", "ln_w", "ln_b", "w3f", "pair_nll", "pcontact", "edist", "pcontact_mean", "part", "res",
         "rec_pos", "gstart", "pairs", "upper", "weight", "big", "lig", "tr_upd", "rot_upd", "t_dev", "ctl", "out",
         "prep_pos", "prep_ca4", "prep_cb4",
         "cdf", "start", "u_inj", "axis_inj", "tr_inj", "sym_out", "step_out")
DOUBLES = ("sigma", "sigma_r3")
FLOATS = ("near_cut", "k_tr", "k_rot", "max_tr", "max_rot", "t_start", "gain_rot", "gain_tr")
INTS = ("B", "R", "L", "contact_bins", "all_atoms", "perturb", "G", "n_big", "n_pairs", "apply", "prep_next", "n_t", "n", "snap_last")
UINTS = ("step", "seed_lo", "seed_hi", "num_steps")
OPS = ("pair_dist_sum", "restraint", "igso3_cdf", "start_pose", "symmetry")
SYM_OUT, SYM_MIN_ORDER, SYM_MAX_ORDER = 12, 2, 24

f32 = np.float32


def f64(x):
    return np.asarray(x, np.float64)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if np.asarray(x).dtype.itemsize == 4 else np.uint64)


class Call(C.Structure):
    _fields_ = ([("buf", kh.Buf * len(SLOTS))] + [(n, C.c_double) for n in DOUBLES] + [("start_bstride", C.c_longlong)] +
                [(n, C.c_float) for n in FLOATS] + [(n, C.c_int) for n in INTS] + [(n, C.c_uint) for n in UINTS])


compile_shim = functools.partial(kh.compile_shim, "aux")


def parts_of(R, L):
    """dfm_internal.h pair_dist_sum_parts: one slot per wave of every (receptor tile, ligand chunk) workgroup."""
    return ((R + PM_RT - 1) // PM_RT) * ((L + PM_LC - 1) // PM_LC) * 4


# ---- binding -----------------------------------------------------------------------------------------------------------------------
class Harness(kh.KernelHarness):
    check = True      # run() asserts success unless told check=False

    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)
        self.lib.ax_check.argtypes = [C.POINTER(Call), C.c_int]
        self.lib.ax_check.restype = C.c_int
        self.lib.ax_parts.argtypes = [C.c_int, C.c_int]
        self.lib.ax_parts.restype = C.c_longlong
        assert int(self.lib.ax_rs_small()) == RS_SMALL and int(self.lib.ax_rs_max_groups()) == RS_MAX_GROUPS
        assert (int(self.lib.ax_sym_out()), int(self.lib.ax_sym_min_order()), int(self.lib.ax_sym_max_order())) == (SYM_OUT, SYM_MIN_ORDER, SYM_MAX_ORDER)
        assert (SYM_MIN_ORDER, SYM_MAX_ORDER) == (SY.MIN_ORDER, SY.MAX_ORDER)
        assert all(int(self.lib.ax_parts(R, L)) == parts_of(R, L) for R, L in ((1, 1), (33, 65), (65, 129)))

    def check_only(self, op, bufs, **scalars):
        """The shim's range checks alone: no device is touched."""
        call, _, keep = self.fill_call(bufs, scalars)
        return int(self.lib.ax_check(C.byref(call), OPS.index(op)))

    # ---- the operations
    def dist_sum(self, c, maps=("pair_nll", "pcontact", "edist", "pcontact_mean"), contact_bins=7, near_cut=12.0, sl=slice(None), check=True):
        """One launch_pair_dist_sum on the case c (dist_case).  maps: the optional outputs asked for.  part and res start as the 0xff
        sentinel (NaN as a double).  sl: the trajectories of the case that take part."""
        P, Q, ca4 = c["P"][sl], c["Q"][sl], c["ca4"][sl]
        B, R, L = len(P), c["R"], c["L"]
        bufs = dict(P=P, Q=Q, ca4=ca4, w_d=c["w_d"], ln_w=c["ln_w"], ln_b=c["ln_b"], w3f=c["w3f"],
                    part=Out(np.float64, B * parts_of(R, L) * 4), res=Out(np.float64, B * 4))
        for m in maps:
            bufs[m] = Out(f32, (1 if m == "pcontact_mean" else B) * R * L)
        r = self.run("pair_dist_sum", bufs, check=check, B=B, R=R, L=L, contact_bins=contact_bins, near_cut=near_cut)
        if r["err"] == HIP_SUCCESS:
            r["res"] = r["res"].reshape(B, 4)
            for m in maps:
                r[m] = r[m].reshape((R, L) if m == "pcontact_mean" else (B, R, L))
        return r

    def restraint(self, c, apply=0, out=True, prep=False, t_dev=None, step=0, ctl=None, sl=slice(None), rot0=None, tr0=None, check=True,
                  **over):
        """One launch_restraint on the case c (restraint_case).  apply: lig, tr_upd and rot_upd are in / out (rot0 / tr0 their start);
        otherwise the pose is an input.  prep: prep_next with its three outputs."""
        lig = np.ascontiguousarray(c["lig"][sl])
        B, R, L = len(lig), c["R"], c["L"]
        N = R + L
        bufs = dict(rec_pos=c["rec_pos"], gstart=c["gstart"], pairs=c["pairs"], upper=c["upper"], weight=c["weight"],
                    big=c["big"] if len(c["big"]) else None, lig=Out(f32, init=lig) if apply else lig, t_dev=t_dev, ctl=ctl)
        if apply:
            bufs.update(tr_upd=Out(f32, init=np.zeros((B, 3), f32) if tr0 is None else tr0),
                        rot_upd=Out(f32, init=np.zeros((B, 3), f32) if rot0 is None else rot0))
        if out:
            bufs["out"] = Out(f32, B * 8)
        if prep:
            bufs.update(prep_pos=Out(f32, B * N * 4), prep_ca4=Out(f32, B * N * 4), prep_cb4=Out(f32, B * N * 4))
        sc = dict(B=B, R=R, L=L, all_atoms=c["all_atoms"], G=len(c["upper"]), n_big=len(c["big"]), n_pairs=len(c["pairs"]), apply=apply,
                  prep_next=int(prep), n_t=0 if t_dev is None else len(t_dev), step=step, **{k: c["params"][k] for k in FLOATS[1:6]})
        sc.update(over)
        r = self.run("restraint", bufs, check=check, **sc)
        if "out" in r:
            r["out"] = r["out"].reshape(B, 8)
        return r

    def symmetry(self, c, apply=0, out=True, step_out=True, prep=False, t_dev=None, step=0, num_steps=0, ctl=None, sl=slice(None), rot0=None,
                 tr0=None, check=True, **over):
        """One launch_symmetry on the case c (sym_case).  The pose is in / out in both modes (evaluation mode must return its bits);
        apply: tr_upd and rot_upd are in / out (rot0 / tr0 their start).  out / step_out: the two optional outputs; prep: prep_next with
        its three outputs.  Returns the slots reshaped per trajectory, `ev` (sym_unpack) when `out` was asked for."""
        lig = np.ascontiguousarray(c["lig"][sl])
        B, L = len(lig), c["L"]
        N = 2 * L
        bufs = dict(rec_pos=c["rec_pos"], lig=Out(f32, init=lig), t_dev=t_dev, ctl=ctl)
        if apply:
            bufs.update(tr_upd=Out(f32, init=np.zeros((B, 3), f32) if tr0 is None else tr0),
                        rot_upd=Out(f32, init=np.zeros((B, 3), f32) if rot0 is None else rot0))
        if out:
            bufs["sym_out"] = Out(np.float64, B * SYM_OUT)
        if step_out:
            bufs["step_out"] = Out(f32, B * 6)
        if prep:
            bufs.update(prep_pos=Out(f32, B * N * 4), prep_ca4=Out(f32, B * N * 4), prep_cb4=Out(f32, B * N * 4))
        p = c["params"]
        sc = dict(B=B, R=L, L=L, all_atoms=c["all_atoms"], n=c["n"], apply=apply, prep_next=int(prep), n_t=0 if t_dev is None else len(t_dev),
                  step=step, num_steps=num_steps, snap_last=p["snap_last"], **{k: p[k] for k in ("gain_rot", "gain_tr", "max_rot", "max_tr", "t_start")})
        sc.update(over)
        r = self.run("symmetry", bufs, check=check, **sc)
        if r["err"] == HIP_SUCCESS:
            r["lig"] = r["lig"].reshape(B, L * 9)
            for k in ("tr_upd", "rot_upd"):
                if k in r:
                    r[k] = r[k].reshape(B, 3)
            if step_out:
                r["step_out"] = r["step_out"].reshape(B, 6)
            if out:
                r["sym_out"] = r["sym_out"].reshape(B, SYM_OUT)
                r["ev"] = sym_unpack(r["sym_out"], r["step_out"] if step_out else np.full((B, 6), np.nan, f32))
        return r

    def igso3(self, sigma, extra=24):
        """launch_igso3_cdf into a block of IGSO3_N + extra doubles: the entries past the table must keep the sentinel."""
        return self.run("igso3_cdf", dict(cdf=Out(np.float64, IGSO3_N + extra)), sigma=sigma)["cdf"]

    def start(self, start, cdf, B, L, bstride, all_atoms=0, perturb=1, sigma_r3=1.0, u=None, axis=None, tr=None, pose=True, seed=0, check=True):
        """One launch_start_pose.  pose: lig_cur given (else the evaluation mode).  Returns lig [B][L*9], tr_upd, rot_upd [B][3]."""
        bufs = dict(start=np.ascontiguousarray(start, f32), cdf=None if cdf is None else np.ascontiguousarray(cdf, np.float64),
                    u_inj=None if u is None else np.ascontiguousarray(u, f32), axis_inj=None if axis is None else np.ascontiguousarray(axis, f32),
                    tr_inj=None if tr is None else np.ascontiguousarray(tr, f32), tr_upd=Out(f32, B * 3), rot_upd=Out(f32, B * 3))
        if pose:
            bufs["lig"] = Out(f32, B * L * 9)
        r = self.run("start_pose", bufs, check=check, B=B, L=L, start_bstride=bstride, all_atoms=all_atoms, perturb=perturb, sigma_r3=sigma_r3,
                     seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32)
        if r["err"] == HIP_SUCCESS:
            r["tr_upd"], r["rot_upd"] = r["tr_upd"].reshape(B, 3), r["rot_upd"].reshape(B, 3)
            if pose:
                r["lig"] = r["lig"].reshape(B, L * 9)
        return r


# =====================================================================================================================================
# k_pair_dist_sum / k_dist_finish / k_dist_mean
# =====================================================================================================================================
def pack_w3f(W3):
    """PairDArgs::w3f from its comment: w3f[((ob 64 + c4) 32 + m) 4 + e] = W3[ob 32 + m][c4 4 + e] / SILU_S, in numpy float32 with
    float32(1 / SILU_S) folded in as one product.  W3 [64][256]."""
    W3 = np.asarray(W3, f32)
    inv = f32(1.0) / SILU_S
    return np.ascontiguousarray((W3 * inv).reshape(2, 32, 64, 4).transpose(0, 2, 1, 3)).reshape(-1)


def lattice_vector(n16, rng=None):
    """A vector of the quarter-angstrom lattice with d^2 = n16 / 16 exactly: integers (a, b, c) / 4 with a^2 + b^2 + c^2 = n16, or None
    (numbers of the form 4^k (8 m + 7) have none).  The first solution in a fixed order."""
    top = int(math.isqrt(n16))
    for a in range(top, -1, -1):
        rest = n16 - a * a
        for b in range(min(a, int(math.isqrt(rest))), -1, -1):
            c2 = rest - b * b
            c = int(math.isqrt(c2))
            if c * c == c2 and c <= b:
                return np.array([a, b, c]) * 0.25
    return None


def neighbours16(n16):
    """The nearest representable d^2 (in sixteenths) below and above n16: one lattice step where a vector exists, two where
    n16 -+ 1 has the form 4^k (8 m + 7) (729 - 1/16 and 144 - 1/16 are such numbers)."""
    lo = next(n for n in range(n16 - 1, -1, -1) if lattice_vector(n) is not None)
    hi = next(n for n in range(n16 + 1, n16 + 9) if lattice_vector(n) is not None)
    return lo, hi


# d^2 in sixteenths of the planted pairs: the three bin bounds the fp32 table holds exactly and the near cutoff, each with its
# neighbours; D = 0; the last bin
BOUND16 = (169, 11664, 41209)      # 3.25^2, 27^2, 50.75^2
NEAR16 = 2304                      # 12^2
NEAR_CUT = 12.0


@functools.lru_cache(maxsize=None)
def planted_offsets():
    """[(name, offset [3])]: the issue's own vectors first ((3, 1.25, 0), (18, 18, 9), (50.75, 0, 0), (12, 0, 0), (8, 8, 4)), then the
    neighbours of each bound, D = 0 and two pairs past 50.75 A."""
    out = [("on 3.25", np.array([3.0, 1.25, 0.0])), ("on 27", np.array([18.0, 18.0, 9.0])), ("on 50.75", np.array([50.75, 0.0, 0.0])),
           ("on near 12 a", np.array([12.0, 0.0, 0.0])), ("on near 12 b", np.array([8.0, 8.0, 4.0]))]
    for n in BOUND16 + (NEAR16,):
        lo, hi = neighbours16(n)
        out += [(f"below {n}/16", lattice_vector(lo)), (f"above {n}/16", lattice_vector(hi))]
    out += [("D = 0", np.zeros(3)), ("past the last bound", np.array([51.0, 0.0, 0.0])), ("far", np.array([60.0, 60.0, 60.0]))]
    return tuple(out)


def dist_coords(rng, B, R, L, span=40):
    """ca4 [B][N][4] on the quarter-angstrom lattice, |coordinate| <= 64: dx, d^2 and, at perfect squares, D are exact in fp32.
    Trajectory 0 carries the planted pairs (receptor 0, ligand k) for as many k as L allows, trajectory B - 1 the same mirrored onto
    the LAST receptor and the last ligand residues, so that tail tiles see them too."""
    ca = np.zeros((B, R + L, 4), f32)
    ca[..., :3] = rng.integers(-span, span + 1, (B, R + L, 3)) * 0.25
    offs = planted_offsets()
    ca[0, 0, :3] = (-2.0, 1.5, -0.25)
    for k, (_, off) in enumerate(offs[:L]):
        ca[0, R + k, :3] = ca[0, 0, :3] + off
    b = B - 1
    if b or R > 1:
        ca[b, R - 1, :3] = (1.0, -3.0, 0.5)
    for k, (_, off) in enumerate(offs[:min(len(offs), L if b else max(0, L - len(offs)))]):
        ca[b, R + L - 1 - k, :3] = ca[b, R - 1, :3] - off
    assert np.abs(ca).max() <= 64.0
    return ca


def dist_case(R, L, B=1, regime="natural", seed=0, kappa=1.0):
    """Inputs of one launch_pair_dist_sum.  Regimes:
      natural   P / Q ~ N(0, 1), the generator's weight scales (dfmdock_amd/weights.py), W3 ~ N(0, 1) / 16;
      kappa     a common channel offset on P and Q: E[z^2] / Var[z] ~ kappa;
      spread    W3 120 times larger: the logits of a pair spread over several hundred and most exp2 underflow;
      wd0       w_d = 0;
      onehot    ln_w = 0, ln_b = 1, W3[o][o] = -0.05 o: every pair has the same logits z_o = -0.05 o SiLU(1), all 64 different, so that
                pair_nll identifies the bin the kernel used (bin_from_nll)."""
    rng = np.random.default_rng([seed, R, L, B])
    N = R + L
    off = f32(0.5 * np.sqrt(2.0 * (kappa - 1.0)))
    P = (rng.standard_normal((B, N, H)) + off).astype(f32)
    Q = (rng.standard_normal((B, N, H)) + off).astype(f32)
    P[:, R:] = np.nan      # the rows the kernel must not read
    Q[:, :R] = np.nan
    w_d, ln_w, ln_b, _ = hh.head_weights(rng)
    W3 = (rng.standard_normal((64, H)) / 16).astype(f32)
    if regime == "spread":
        W3 *= f32(120.0)
    elif regime == "wd0":
        w_d[:] = 0
    elif regime == "onehot":
        ln_w[:] = 0
        ln_b[:] = 1
        W3[:] = 0
        W3[np.arange(64), np.arange(64)] = f32(-0.05) * np.arange(64, dtype=f32)
    return dict(P=P, Q=Q, ca4=dist_coords(rng, B, R, L), w_d=w_d, ln_w=ln_w, ln_b=ln_b, W3=W3, w3f=pack_w3f(W3), R=R, L=L, B=B, regime=regime)


DIST_SHAPES = ((1, 1, 1), (1, 3, 3), (31, 4, 1), (32, 5, 3), (33, 65, 1), (32, 63, 1), (31, 64, 3), (65, 129, 1), (33, 129, 3))      # (R, L, B)
DIST_TAIL_SHAPES = ((33, 65, 1), (65, 129, 1))
TAIL_CONTACT_BINS = (1, 4, 5, 32, 33, 63)


def dist_cases():
    """name -> case of every launch the GPU tests compare with float64."""
    out = {f"natural_{R}_{L}_{B}": dist_case(R, L, B, seed=1) for R, L, B in DIST_SHAPES}
    out.update({f"onehot_{R}_{L}_{B}": dist_case(R, L, B, "onehot", seed=2) for R, L, B in DIST_SHAPES})
    for k in (50.0, 2000.0):
        out[f"kappa_{k:g}"] = dist_case(33, 65, 1, "kappa", seed=3, kappa=k)
    out["spread"] = dist_case(33, 65, 3, "spread", seed=4)
    out["wd0"] = dist_case(33, 65, 1, "wd0", seed=5)
    return out


def dist_logits64(c, sl=slice(None)):
    """(logits [B][R][L][64], eps_z, D, er) in float64 from the definition (pair_z64 -> layernorm64 -> silu64 -> W3) and the bound of the
    kernel's logits: heads_harness.pair_head_m_ref's up to the projection, which here is 128 32x32x2 MFMA steps per accumulator - at
    most 256 roundings of a partial sum - on an operand packed with two roundings (1 / SILU_S, the product) and multiplied with a third."""
    P, Q, ca4, R = c["P"][sl], c["Q"][sl], c["ca4"][sl], c["R"]
    W3t = f64(c["W3"]).T
    with np.errstate(all="ignore"):
        s, bound, scale, D, kappa, er = hh.pair_head_m_ref(P, Q, ca4, R, c["w_d"], c["ln_w"], c["ln_b"], W3t)
        eps_z = bound + (256 - 130) * U * scale
    return s, eps_z, D, er


def dist_ref(c, contact_bins=7, near_cut=NEAR_CUT, sl=slice(None)):
    """Everything launch_pair_dist_sum returns, from the definitions (distogram.pair_maps / pose_scores / pcontact_mean on the float64
    logits), and the bound of each output.  Derivation: tests/test_gpu_aux_kernels.py.  Non-finite inputs give non-finite references
    (and NaN bounds) exactly where the definition does."""
    z, ez, D, er = dist_logits64(c, sl)
    B, R, L = z.shape[:3]
    with np.errstate(all="ignore"):
        E = ez.max(-1)
        m = DG.pair_maps(z, D, contact_bins)
        zs = z - z.max(-1, keepdims=True)
        ev = np.exp(zs)
        es = ev.sum(-1)
        x = np.abs(zs) / np.log(2.0)
        # exp2 of an argument with three roundings (difference, log2 e, product) and its own ulp; 32 + 1 additions of the sum; underflow
        dev = (3 * np.log(2.0) * x + 1) * U * ev + 2.0 ** -126
        des = dev.sum(-1) + 33 * U * es
        bin_ = DG.bin_of(D)
        zt = np.take_along_axis(zs, bin_[..., None], -1)[..., 0]
        nll_b = 2 * E + des / es + 4 * U * np.abs(np.log(es)) + U * np.abs(zt) + 2 * U * np.abs(m["pair_nll"]) + 2.0 ** -126
        grow = np.expm1(2 * E)
        pc_b = m["pcontact"] * (grow + des / es + 2 * U) + (dev[..., :contact_bins].sum(-1) + 33 * U * ev[..., :contact_bins].sum(-1)) / es + 2.0 ** -126
        cen = DG.CENTRES
        dcen = 3 * U * (DG.MIN_BIN + DG.STEP * 63)      # 3.25f + step_f (k - 0.5f): the step, the product, the sum
        ed_b = m["edist"] * (grow + des / es + 2 * U) + ((dev * cen).sum(-1) + dcen * es + 34 * U * (ev * cen).sum(-1)) / es
    ref = dict(pair_nll=m["pair_nll"], pcontact=m["pcontact"], edist=m["edist"], bin=bin_, D=D, E=E, er=er,
               b_pair_nll=nll_b, b_pcontact=pc_b, b_edist=ed_b)
    near = D < near_cut
    n_add = PM_LW + 6 + parts_of(R, L) + 1      # float64 additions of one quantity: a lane's pairs, the butterfly, k_dist_finish; the division
    res, res_b = np.zeros((B, 4)), np.zeros((B, 4))
    with np.errstate(all="ignore"):
        for b in range(B):
            s = DG.pose_scores(z[b], D[b], contact_bins, near_cut)
            nn = s["n_near"]
            res[b] = (s["nll"], s["nll_near"], nn, s["exp_contacts"])
            res_b[b, 0] = nll_b[b].sum() / (R * L) + n_add * E64 * np.abs(m["pair_nll"][b]).sum() / (R * L)
            res_b[b, 1] = (nll_b[b][near[b]].sum() + n_add * E64 * np.abs(m["pair_nll"][b][near[b]]).sum()) / nn if nn else 0.0
            res_b[b, 3] = pc_b[b].sum() + n_add * E64 * m["pcontact"][b].sum()
        ref.update(res=res, b_res=res_b, near=near, pcontact_mean=DG.pcontact_mean(m["pcontact"]))
        ref["b_pcontact_mean"] = pc_b.mean(0) + U * ref["pcontact_mean"]
    return ref


def onehot_nll(c):
    """The 64 values -log_softmax(z)[o] of the onehot regime's pair-independent logits, float64."""
    a = float(hh.silu64(np.float64(1.0)))
    return -DG.log_softmax(a * f64(c["W3"])[np.arange(64), np.arange(64)])


def bin_from_nll(c, pair_nll):
    """The bin whose logit the kernel took, for every pair of a onehot case: the nearest of the 64 known values, and the distance to it."""
    ref = onehot_nll(c)
    d = np.abs(f64(pair_nll)[..., None] - ref)
    return d.argmin(-1), d.min(-1)


def bound_table_f32():
    """The kernel's bin table restated in numpy float32: (bounds^2 [63] = (3.25f + step_f k)^2, centres [64] = 3.25f + step_f (k - 0.5f))."""
    step = (f32(50.75) - f32(3.25)) / f32(62.0)
    k = np.arange(64, dtype=f32)
    bd = f32(3.25) + step * k
    return (bd * bd)[:63], f32(3.25) + step * (k - f32(0.5))


DIST_MUTANTS = {      # name -> the comparison of the GPU tests that rejects it
    "hh_logits_swapped": "bin", "contact_bins_without_4hh": "pcontact", "moments_of_next_row": "pair_nll", "count_ge": "bin",
    "near_le": "n_near", "partial_in_neighbour_slot": "res", "variance_without_2dot": "pair_nll", "centres_half_step": "edist",
    "mean_over_B_minus_1": "pcontact_mean"}


def dist_fp32(c, contact_bins=7, near_cut=NEAR_CUT, mutant=None):
    """k_pair_dist_sum + k_dist_finish + k_dist_mean restated in numpy float32 (the same formulas; sums in numpy's order): row moments and
    P.Q -> mean, ez2 - mean^2 -> rstd; S y as the five-term sum; SiLU as y' rcp(1 + exp2(y')); the packed W3; exp2-softmax against the
    row maximum, the fp32 bin table, the float64 partials of every wave in the kernel's slots.  mutant: one of DIST_MUTANTS -
      hh_logits_swapped          logits 4..7 and 0..3 of every group of eight swapped between the hh halves;
      contact_bins_without_4hh   the hh = 1 lanes compare their logit index without the + 4;
      moments_of_next_row        a wave reads the moments of its ligand row it + 1 for row it (an idle row's are 0);
      count_ge                   d^2 >= bound in the bin count;
      near_le                    D <= near_cut;
      partial_in_neighbour_slot  a wave writes the slot after its own (the last one nowhere): slot 0 keeps the sentinel;
      variance_without_2dot      ez2 without the 2 P.Q term;
      centres_half_step          centre k = 3.25 + step k;
      mean_over_B_minus_1        pcontact_mean divided by B - 1."""
    f = f32
    R, L, B = c["R"], c["L"], c["B"]
    P, Q, ca = np.asarray(c["P"], f), np.asarray(c["Q"], f), np.asarray(c["ca4"], f)
    w_d, ln_w, ln_b = (np.asarray(c[k], f) for k in ("w_d", "ln_w", "ln_b"))
    Pr, Ql = P[:, :R], Q[:, R:]
    with np.errstate(all="ignore"):
        vec = ca[:, :R, None, :3] - ca[:, None, R:, :3]
        d2 = ((vec[..., 0] * vec[..., 0] + vec[..., 1] * vec[..., 1]) + vec[..., 2] * vec[..., 2]).astype(f)
        D = np.sqrt(d2).astype(f)
        mP, mP2, mPw = Pr.sum(-1, dtype=f), (Pr * Pr).sum(-1, dtype=f), (Pr * w_d).sum(-1, dtype=f)
        sQ, sQ2, sQw = Ql.sum(-1, dtype=f), (Ql * Ql).sum(-1, dtype=f), (Ql * w_d).sum(-1, dtype=f)
        if mutant == "moments_of_next_row":
            l = np.arange(L)
            nxt = l + 4
            ok = nxt < np.minimum(L, (l // PM_LC) * PM_LC + PM_LC)
            pick = lambda s: np.where(ok, s[:, np.where(ok, nxt, 0)], f(0))
            sQ, sQ2, sQw = pick(sQ), pick(sQ2), pick(sQw)
        sum_w, sum_w2 = w_d.sum(dtype=f), (w_d * w_d).sum(dtype=f)
        dot = np.einsum("brc,blc->brl", Pr, Ql).astype(f)
        inv = f(1.0 / H)
        mean = ((mP[:, :, None] + sQ[:, None, :]) + D * sum_w) * inv
        two_dot = f(0) if mutant == "variance_without_2dot" else f(2) * dot
        ez2 = (((mP2[:, :, None] + sQ2[:, None, :]) + two_dot) + D * (f(2) * (mPw[:, :, None] + sQw[:, None, :]) + D * sum_w2)) * inv
        rstd = (f(1) / np.sqrt(np.maximum(ez2 - mean * mean, f(0)) + f(hh.LN_EPS))).astype(f)
        lw = SILU_S * ln_w
        y = (rstd[..., None] * (Pr * lw)[:, :, None, :] + (rstd * D)[..., None] * (lw * w_d)) + (rstd[..., None] * (Ql * lw)[:, None, :, :])
        y = (y + (-mean * rstd)[..., None] * lw) + SILU_S * ln_b
        a = (y * (f(1) / (f(1) + np.exp2(y)))).astype(f)
        w3 = c["w3f"].reshape(2, 64, 32, 4).transpose(0, 2, 1, 3).reshape(64, H)      # unpacked again: [o][c], 1 / S folded in
        z = (a @ w3.T).astype(f)
        if mutant == "hh_logits_swapped":
            z = z[..., np.arange(64) ^ 4]
        b2, cen = bound_table_f32()
        if mutant == "centres_half_step":
            cen = f(3.25) + ((f(50.75) - f(3.25)) / f(62.0)) * np.arange(64, dtype=f)
        bin_ = ((d2[..., None] >= b2) if mutant == "count_ge" else (d2[..., None] > b2)).sum(-1)
        zm = z.max(-1)
        ev = np.exp2((z - zm[..., None]) * f(1.44269504088896340736)).astype(f)
        es = ev.sum(-1, dtype=f)
        o = np.arange(64)
        inc = np.where((o & 4) != 0, o - 4, o) < contact_bins if mutant == "contact_bins_without_4hh" else o < contact_bins
        pc = (ev * inc).sum(-1, dtype=f)
        ed = (ev * cen).sum(-1, dtype=f)
        zt = np.take_along_axis(z, bin_[..., None], -1)[..., 0]
        nll = ((zm - zt) + np.log(es)).astype(f)
        pcon, edv = (pc / es).astype(f), (ed / es).astype(f)
        near = (D <= f(near_cut)) if mutant == "near_le" else (D < f(near_cut))
        # the partials: slot (((b nrt + rt) nlc + lc) 4 + wave) holds the pairs r in tile rt, l in chunk lc with l % 4 == wave
        nrt, nlc = (R + PM_RT - 1) // PM_RT, (L + PM_LC - 1) // PM_LC
        part = np.full((B * nrt * nlc * 4 + 1, 4), np.nan)
        for b in range(B):
            for rt in range(nrt):
                for lc in range(nlc):
                    for w in range(4):
                        rs, ls = slice(rt * PM_RT, rt * PM_RT + PM_RT), slice(lc * PM_LC + w, min(L, lc * PM_LC + PM_LC), 4)
                        nn, nr = f64(nll[b, rs, ls]), near[b, rs, ls]
                        slot = ((b * nrt + rt) * nlc + lc) * 4 + w + (1 if mutant == "partial_in_neighbour_slot" else 0)
                        part[slot] = (nn.sum(), nn[nr].sum(), nr.sum(), f64(pcon[b, rs, ls]).sum())
        part = part[:-1].reshape(B, -1, 4)
        tot = part.sum(1)
        res = np.stack([tot[:, 0] / (R * L), tot[:, 1] / tot[:, 2], tot[:, 2], tot[:, 3]], 1)
        pm = (f64(pcon).sum(0) / (B - 1 if mutant == "mean_over_B_minus_1" else B)).astype(f)
    return dict(pair_nll=nll, pcontact=pcon, edist=edv, pcontact_mean=pm, res=res, part=part)


def worst_ratio(got, ref, bound):
    """The largest |got - ref| / bound over the elements whose reference is finite (NaN in `got` there counts as infinite)."""
    got, ref = f64(got), f64(ref)
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    with np.errstate(all="ignore"):
        ratio = np.abs(got - ref)[fin] / np.broadcast_to(bound, ref.shape)[fin]
    return float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))


def dist_compare(c, got, ref, maps=("pair_nll", "pcontact", "edist", "pcontact_mean")):
    """Every comparison of one launch against dist_ref: {name: worst |error| / bound (continuous) or number of mismatches (discrete)}.
    'bin' only for the onehot regime; 'nonfinite': elements the definition makes non-finite that came back finite."""
    out = {}
    bad = 0
    for m in maps:
        out[m] = worst_ratio(got[m], ref[m], ref["b_" + m])
        bad += int((np.isfinite(got[m]) & ~np.isfinite(ref[m])).sum())
    res = f64(got["res"])
    out["n_near"] = int((res[:, 2] != ref["res"][:, 2]).sum())
    for k, name in ((0, "nll"), (1, "nll_near"), (3, "exp_contacts")):
        out[name] = worst_ratio(res[:, k], ref["res"][:, k], ref["b_res"][:, k])
        bad += int((np.isfinite(res[:, k]) & ~np.isfinite(ref["res"][:, k])).sum())
    out["res"] = max(out["nll"], out["nll_near"], out["exp_contacts"]) if not out["n_near"] else np.inf
    out["nonfinite"] = bad
    if c["regime"] == "onehot" and "pair_nll" in maps:
        b, _ = bin_from_nll(c, got["pair_nll"])
        out["bin"] = int((b != ref["bin"]).sum())
    return out


# =====================================================================================================================================
# k_restraint
# =====================================================================================================================================
GROUP_SIZES = (1, 16, 17, 63, 64, 65, 200)
DEFAULT_PARAMS = dict(k_tr=0.25, k_rot=3e-3, max_tr=10.0, max_rot=0.3, t_start=1.0)


def pack_groups(groups, R, L):
    gs, pairs, up, w = RS.pack(groups, R, L)
    big = np.array([g for g in range(len(groups)) if gs[g + 1] - gs[g] > RS_SMALL], np.int32)
    return dict(gstart=gs, pairs=pairs, upper=up, weight=w, big=big)


def restraint_case(G, L, R=40, B=2, all_atoms=0, seed=0, sizes=GROUP_SIZES, params=None, spread=6.0, upper=(4.0, 12.0)):
    """Inputs of one launch_restraint: G groups whose sizes cycle through `sizes`, an exact tie (the first pair listed again) in every
    fifth, weight 0 in every sixth, a group every pose satisfies (u = 500) in every seventh; poses ~ N(2, spread^2)."""
    rng = np.random.default_rng([seed, G, L, R])
    groups = []
    for g in range(G):
        n = sizes[g % len(sizes)]
        pairs = [(int(rng.integers(R)), int(rng.integers(L))) for _ in range(n)]
        if g % 5 == 1 and n > 1:
            pairs[-1] = pairs[0]
        up = 500.0 if g % 7 == 3 else float(f32(rng.uniform(*upper)))
        w = 0.0 if g % 6 == 2 else float(f32(rng.uniform(0.2, 3.0)))
        groups.append(RS.RestraintGroup(tuple(pairs), up, w))
    p = {k: float(f32(v)) for k, v in dict(DEFAULT_PARAMS, **(params or {})).items()}
    c = dict(groups=groups, rec_pos=(rng.standard_normal((R, 9)) * spread).astype(f32), lig=(rng.standard_normal((B, L, 9)) * spread + 2).astype(f32),
             R=R, L=L, B=B, all_atoms=all_atoms, params=p)
    c.update(pack_groups(groups, R, L))
    return c


def custom_case(groups, rec_ca, lig_ca, all_atoms=0, params=None, B=1):
    """A case from explicit CA positions: rec_ca [R][3], lig_ca [L][3] (N and C placed 1.5 A off along x and y)."""
    rec_ca, lig_ca = np.asarray(rec_ca, f32), np.asarray(lig_ca, f32)
    R, L = len(rec_ca), len(lig_ca)
    mk = lambda ca: np.concatenate([ca - f32([1.5, 0, 0]), ca, ca + f32([0, 1.5, 0])], -1).astype(f32)
    p = {k: float(f32(v)) for k, v in dict(DEFAULT_PARAMS, **(params or {})).items()}
    c = dict(groups=list(groups), rec_pos=mk(rec_ca), lig=np.tile(mk(lig_ca)[None], (B, 1, 1)), R=R, L=L, B=B, all_atoms=all_atoms, params=p)
    c.update(pack_groups(c["groups"], R, L))
    return c


def restraint_ref(c, b):
    """restraints.evaluate at pose b of the case, plus the bound of energy and of the six step components.

    Bound.  d^2, d and v are the definition's own float64 operations in its own order (-ffp-contract=off): no error.  A group's terms
    (w v^2; s (x - y) with s = -2 w v / d against the definition's ((-2 w) v) (x - y) / d; r x f) differ by at most three float64
    roundings each.  Lane t folds the groups t, t + 256, .. in order (ceil(G / 256) additions), the wave butterfly adds 6 times, thread 0
    adds the four waves (3): (ceil(G / 256) + 12) 2^-53 sum |terms|.  The torque also carries the centroid, which the kernel sums in another
    order than numpy: (ceil(n / 256) + 12 + log2 n) 2^-53 max|x| times sum |f|.  Then k, the clip (norm, m / n, the product: 6 more
    roundings of the result) and ONE fp32 rounding."""
    p = c["params"]
    prm = RS.RestraintParams(**p)
    center = "all_atoms" if c["all_atoms"] else "ca"
    with np.errstate(all="ignore"):
        ev = RS.evaluate(c["groups"], c["rec_pos"], c["lig"][b].reshape(-1, 3, 3), prm, center)
    G = len(c["groups"])
    y = f64(c["rec_pos"]).reshape(-1, 3, 3)[:, 1]
    lig = f64(c["lig"][b]).reshape(-1, 3, 3)
    x = lig[:, 1]
    cen = lig.reshape(-1, 3).mean(0) if c["all_atoms"] else x.mean(0)
    ncen = lig.shape[0] * (3 if c["all_atoms"] else 1)
    dcen = (-(-ncen // 256) + 12 + np.log2(ncen) + 1) * E64 * np.abs(lig).max()
    nsum = (-(-G // 256) + 12) * E64
    e_abs, f_abs, t_abs, fsum = 0.0, np.zeros(3), np.zeros(3), 0.0
    with np.errstate(all="ignore"):
        for g, grp in enumerate(c["groups"]):
            d = ev["d"][g]
            v = d - grp.upper
            if not v > 0:
                if np.isnan(v):
                    e_abs = np.nan
                continue
            e_abs += grp.weight * v * v
            if grp.weight == 0:
                continue
            i, j = grp.pairs[int(ev["arg"][g])]
            fv = np.abs(2.0 * grp.weight * v * (x[j] - y[i]) / d)
            r = np.abs(x[j] - cen)
            f_abs += fv
            t_abs += np.array([r[1] * fv[2] + r[2] * fv[1], r[2] * fv[0] + r[0] * fv[2], r[0] * fv[1] + r[1] * fv[0]])
            fsum += fv.sum()
    step = ev["step"]
    raw = np.concatenate([p["k_tr"] * ev["force"], p["k_rot"] * ev["torque"]])
    raw_b = np.concatenate([p["k_tr"] * nsum * f_abs, p["k_rot"] * (nsum * t_abs + 2 * dcen * fsum)])
    nrm = np.array([np.linalg.norm(raw[:3]), np.linalg.norm(raw[3:])])
    nrm_b = np.array([np.linalg.norm(raw_b[:3]), np.linalg.norm(raw_b[3:])]) + 4 * E64 * nrm
    lim = np.array([p["max_tr"], p["max_rot"]])
    clipped = nrm > lim
    with np.errstate(all="ignore"):
        scale = np.repeat(np.where(clipped, lim / nrm, 1.0), 3)
        # a clipped step: d(v m / n) <= (dv + |v| dn / n) m / n
        step_b = scale * (raw_b + np.abs(raw) * np.repeat(np.where(clipped, nrm_b / nrm, 0.0), 3)) + 6 * E64 * np.abs(step) + U * np.abs(step) + 2.0 ** -149
    return dict(energy=ev["energy"], n_satisfied=ev["n_satisfied"], step=step, arg=ev["arg"], d=ev["d"], b_energy=nsum * e_abs + U * abs(ev["energy"]) + 2.0 ** -149,
                b_step=step_b, norm=nrm, b_norm=nrm_b, limit=lim, clipped=clipped, decided=np.abs(nrm - lim) > nrm_b)


def argmin_restated(c, b, mutant=None):
    """The kernel's two arg-min paths restated in numpy float64 for every group of pose b: (d^2 [G], pair index within the group [G]).
    Small groups: the serial loop.  Large groups: lane-local strided loops, then the butterfly's lexicographic (d^2, pair index) minimum.
    NaN wins (the first NaN in list order), as np.argmin has it.  mutants:
      nan_dropped    `d2 < best` alone in both loops and `ob < best` in the butterfly (a later NaN loses, an earlier one sticks);
      last_tie       `<=` in the two loops: the last of equal minima of a serial group or of a lane;
      lane_order     the butterfly ignores the pair index on ties (the lower lane's value stays);
      tie_high       the butterfly takes the higher pair index on ties."""
    y = f64(c["rec_pos"]).reshape(-1, 3, 3)[:, 1]
    x = f64(c["lig"][b]).reshape(-1, 3, 3)[:, 1]
    gs, pr = c["gstart"], c["pairs"]
    G = len(c["upper"])
    best_d, best_q = np.zeros(G), np.zeros(G, np.int64)
    with np.errstate(all="ignore"):
        diff = x[pr[:, 1]] - y[pr[:, 0]]
        d2 = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]

    def better(dn, do):
        if mutant == "nan_dropped":
            return dn < do
        if mutant == "last_tie":
            return dn <= do or (np.isnan(dn) and not np.isnan(do))
        return dn < do or (np.isnan(dn) and not np.isnan(do))

    def serial(qs):
        best, arg = 0.0, -1
        for q in qs:
            if arg < 0 or better(d2[q], best):
                best, arg = d2[q], q
        return best, arg

    for g in range(G):
        q0, q1 = int(gs[g]), int(gs[g + 1])
        if q1 - q0 <= RS_SMALL:
            best_d[g], best_q[g] = serial(range(q0, q1))
        else:
            lanes = [serial(range(q0 + ln, q1, 64)) for ln in range(min(64, q1 - q0))]
            bd, bq = lanes[0]
            for od, oq in lanes[1:]:
                tie = (od == bd) or (np.isnan(od) and np.isnan(bd))
                if mutant == "lane_order":
                    take = better(od, bd)
                elif mutant == "tie_high":
                    take = better(od, bd) or (tie and oq > bq)
                elif mutant == "nan_dropped":
                    take = od < bd or (od == bd and oq < bq)
                else:
                    take = better(od, bd) or (tie and oq < bq)
                if take:
                    bd, bq = od, oq
            best_d[g], best_q[g] = bd, bq
        best_q[g] -= q0
    return best_d, best_q


def tie_cases():
    """name -> one-group cases with exact ties at the minimum: the tied pairs sit at the same distance from their receptor residue in
    DIFFERENT directions, so that the step tells which pair the kernel took.  Integer coordinates: every d^2 is exact.
      serial       a small group (5 pairs): pairs 1 and 3 tie;
      in_lane      a 200-pair group: pairs 7 and 7 + 64 (the same lane, consecutive strides);
      across       pairs 70 and 9 (lane 6's second stride against lane 9's first: the LOWER pair index 9 must win though lane 6 < lane 9);
      first_last   pairs 0 and 199."""
    out = {}
    for name, n, tied in (("serial", 5, (1, 3)), ("in_lane", 200, (7, 71)), ("across", 200, (9, 70)), ("first_last", 200, (0, 199))):
        rng = np.random.default_rng([11, n, tied[0]])
        L = n
        rec = np.array([[0.0, 0.0, 0.0]])
        lig = rng.integers(12, 30, (L, 3)).astype(np.float64) * rng.choice([-1, 1], (L, 3))      # every other pair far: d^2 >= 432
        lig[tied[0]] = (9.0, 12.0, 0.0)      # d = 15
        lig[tied[1]] = (0.0, -12.0, 9.0)
        grp = RS.RestraintGroup(tuple((0, j) for j in range(L)), 6.0, 1.5)
        c = custom_case([grp], rec, lig, params=dict(k_tr=1e-3, k_rot=1e-4))
        c["tied"] = tied
        out[name] = c
    return out


def ulp_cases():
    """One single-pair group each: d exactly `upper` (satisfied), one fp32 ulp below (satisfied) and above (violated); d = 0; weight 0."""
    up = f32(7.5)
    rows = [("d = u", up, 1.0), ("d = u - ulp", np.nextafter(up, f32(0)), 1.0), ("d = u + ulp", np.nextafter(up, f32(100)), 1.0), ("d = 0", f32(0), 1.0),
            ("weight 0", f32(9.0), 0.0)]
    rec = np.zeros((len(rows), 3))
    lig = np.array([[float(d), 0.0, 0.0] for _, d, _ in rows])
    groups = [RS.RestraintGroup(((k, k),), float(up), w) for k, (_, _, w) in enumerate(rows)]
    return custom_case(groups, rec, lig), [r[0] for r in rows]


def nan_cases():
    """name -> (case, group) with one NaN ligand CA: the first pair of a small group, a later pair of it; in a 200-pair group the first
    pair, a later lane (pair 37) and a later stride of lane 0 (pair 128).  restraints.evaluate is the specification: that group's
    distance, the energy and the step are NaN."""
    out = {}
    for name, n, where in (("small_first", 5, 0), ("small_later", 5, 3), ("big_first", 200, 0), ("big_later_lane", 200, 37),
                           ("big_later_stride", 200, 128), ("big_last", 200, 199)):
        rng = np.random.default_rng([13, n, where])
        rec = rng.standard_normal((3, 3)) * 5
        lig = rng.standard_normal((n, 3)) * 5 + 8
        lig[where] = np.nan
        groups = [RS.RestraintGroup(tuple((int(rng.integers(3)), j) for j in range(n)), 2.0, 1.0), RS.RestraintGroup(((1, (where + 1) % n),), 3.0, 2.0)]
        out[name] = custom_case(groups, rec, lig, B=2)
        out[name]["lig"][1] = np.nan_to_num(out[name]["lig"][1], nan=3.0)      # trajectory 1 is finite
    return out


RESTRAINT_SHAPES = ((1, 1, 0), (255, 85, 1), (256, 86, 0), (257, 300, 1), (4096, 300, 0))      # (G, L, all_atoms)


def restraint_cases():
    out = {}
    for G, L, aa in RESTRAINT_SHAPES:
        sizes = GROUP_SIZES if G < 4096 else (1, 1, 2, 5, 16, 17, 1, 64, 1, 3)      # 4096 groups of mostly single pairs, as real sets are
        out[f"G{G}_L{L}_a{aa}"] = restraint_case(G, L, B=2, all_atoms=aa, seed=1, sizes=sizes, params=dict(k_tr=1e-5, k_rot=1e-8) if G % 2 else None)
    return out


def satisfied_case():
    """Every group satisfied (u = 500): zero step, `moves` false."""
    c = restraint_case(20, 30, seed=5)
    groups = [RS.RestraintGroup(g.pairs, 500.0, g.weight) for g in c["groups"]]
    c.update(groups=groups, **pack_groups(groups, c["R"], c["L"]))
    return c


def apply_ref(c, b, step, rot0, tr0):
    """restraints.apply_step in float64 and the heads tests' bound of the same pose update (tests/test_gpu_head_kernels.py): returns
    (pose [L*9], tr_update, rot_update, bounds of the three)."""
    center = "all_atoms" if c["all_atoms"] else "ca"
    lig = f64(c["lig"][b]).reshape(-1, 3, 3)
    new, ru, tu = RS.apply_step(lig, step, f64(rot0), f64(tr0), center)
    x3 = lig.reshape(-1, 3)
    cen = x3.mean(0) if c["all_atoms"] else lig[:, 1].mean(0)
    rad = np.linalg.norm(x3 - cen, axis=-1).max()
    dtr, drot = 2 * U * (np.abs(step[:3]).max() + 2.0 ** -126), 2 * U * (np.linalg.norm(step[3:]) + 2.0 ** -126)
    dpose = 2 * rad * (drot + 32 * U) + dtr + 8 * U * (np.abs(x3).max() + np.abs(cen).max() + np.abs(step[:3]).max())
    return new.reshape(-1), tu, ru, dpose, dtr + 2 * U * (np.abs(tr0).max() + np.abs(step[:3]).max()), 2 * drot + 256 * U


# =====================================================================================================================================
# k_symmetry
# =====================================================================================================================================
SYM_SIZES = (1, 21, 22, 85, 86, 300)      # residues: 3, 63, 66, 255, 258, 900 atoms - a partial wave, the wave edge, the block stride edge, several strides
SYM_PARAMS = dict(gain_rot=0.5, gain_tr=0.75, max_rot=0.3, max_tr=10.0, t_start=1.0, snap_last=1)      # (the two gains differ: a swap shows)
SYM_MIDPOINTS = {5: ((1, 2),), 8: ((1, 3),), 12: ((1, 5),), 24: ((1, 5), (5, 7), (7, 11))}      # neighbouring generators m | m' of each order
SYM_MUTANTS = {      # name -> the comparison that rejects it
    "larger_m": "order_m", "no_gcd": "order_m", "no_w_flip": "order_m", "clip_under_snap": "step", "gains_swapped": "step",
    "centre_all_atoms": "pose", "screw_sign": "step", "compose_order": "rot_update", "last_off_by_one": "step", "last_from_num_steps": "step"}


def sym_unpack(out, step):
    """[B][SYM_OUT] doubles and [B][6] floats -> the dict symmetry_fixtures.check_eval takes."""
    out = f64(out)
    m = np.where(np.isnan(out[:, 10]), -1.0, out[:, 10])      # (a slot that was not written holds the sentinel, a NaN)
    return dict(theta=out[:, 0], screw=out[:, 1], axis=out[:, 2:5], axis_point=out[:, 5:8], fit_rmsd=out[:, 8], sym_rmsd=out[:, 9],
                order_m=m.astype(np.int64), step=np.asarray(step, f32))


def sym_chain(L, seed=0):
    """A backbone [L][3][3] float32: CA on a random walk of 3.8 A steps, N and C 1.46 / 1.52 A off in independent directions."""
    rng = np.random.default_rng([31, seed, L])
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    ca = np.cumsum(3.8 * unit(rng.standard_normal((L, 3))), 0) + rng.standard_normal(3) * 5
    return np.stack([ca + 1.46 * unit(rng.standard_normal((L, 3))), ca, ca + 1.52 * unit(rng.standard_normal((L, 3)))], 1).astype(f32)


def sym_params(**over):
    return {k: (int(v) if k == "snap_last" else float(f32(v))) for k, v in dict(SYM_PARAMS, **over).items()}


def sym_case_of(y, lig, n, all_atoms, params=None):
    L = len(y)
    lig = np.asarray(lig, f32).reshape(-1, L, 9)
    return dict(rec_pos=np.ascontiguousarray(y, f32).reshape(L, 9), lig=np.ascontiguousarray(lig), R=L, L=L, B=len(lig), all_atoms=all_atoms, n=n,
                params=sym_params(**(params or {})))


@functools.lru_cache(maxsize=None)
def sym_case(L, n, all_atoms, B=8, seed=0):
    """The special poses of symmetry_fixtures.poses - [0] symmetric, [1] theta = pi, [2] clips, [3] does not, [4] an exact translation (no
    axis), [5] a NaN - and B - 6 random ones, of a chain of L residues."""
    import symmetry_fixtures as SF
    y = sym_chain(L, seed)
    return sym_case_of(y, SF.poses(y, n, B, np.random.default_rng([32, seed, L, n])), n, all_atoms)


@functools.lru_cache(maxsize=None)
def sym_midpoint_case(n, L=22, all_atoms=0):
    """Poses 1e-3 rad either side of the midpoint between neighbouring generators, one with theta below the first generator and one above
    the last.  Returns (case, expected m of each pose)."""
    import symmetry_fixtures as SF
    y = sym_chain(L, seed=n)
    rng = np.random.default_rng([33, n])
    thetas, want = [], []
    for m1, m2 in SYM_MIDPOINTS[n]:
        mid = np.pi * (m1 + m2) / n
        thetas += [mid - 1e-3, mid + 1e-3]
        want += [m1, m2]
    first = 2 * np.pi / n
    last = max(m for m in range(1, n // 2 + 1) if math.gcd(m, n) == 1)
    thetas += [0.4 * first, 0.5 * (2 * np.pi * last / n + np.pi)]
    want += [1, last]
    lig = [SF.turn(y, th, rng.standard_normal(3), SF.outside_point(y, rng.standard_normal(3), 4.0), rng.standard_normal()).astype(f32) for th in thetas]
    return sym_case_of(y, np.stack(lig), n, all_atoms), tuple(want)


def sym_p32(c):
    return SY.SymmetryParams(**c["params"])


def symmetry_ref(c, b, last=False):
    """symmetry.evaluate on the kernel's own fp32 coordinates and fp32 parameters at pose b - the definition, never a second run of the
    kernel - and the margins that make a decision `decided`: m_gap (best against second-best |theta - 2 pi m / n| over the coprime m; inf
    with one candidate), clip_margin [2] (| |gain v| - max | of translation and rotation), vn (|v| of the fit's quaternion, against
    symmetry.NO_AXIS) and clipped [2]."""
    p = sym_p32(c)
    center = "all_atoms" if c["all_atoms"] else "ca"
    y, x = c["rec_pos"].reshape(-1, 3, 3), c["lig"][b].reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        ev = SY.evaluate(y, x, c["n"], p, center, last)
    ref = dict(ev, ev=ev, m_gap=np.inf, clip_margin=np.full(2, np.inf), vn=np.nan, clipped=np.zeros(2, bool))
    if ev["Q"] is None:
        return ref
    q = SY._quaternion(ev["Q"])
    ref["vn"] = float(np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
    if ev["m"] == 0:
        return ref
    d = sorted(abs(ev["theta"] - 2.0 * math.pi * m / c["n"]) for m in range(1, c["n"] // 2 + 1) if math.gcd(m, c["n"]) == 1)
    if len(d) > 1:
        ref["m_gap"] = d[1] - d[0]
    raw = np.array([abs(p.gain_tr * ev["screw"]), abs(p.gain_rot * (ev["theta_star"] - ev["theta"]))])
    lim = np.array([p.max_tr, p.max_rot])
    ref["clip_margin"], ref["clipped"] = np.abs(raw - lim), raw > lim
    return ref


def symmetry_restated(c, b, mutant=None, idx=None, num_steps=0, ctl=None, rot0=None, tr0=None):
    """k_symmetry's decisions restated in float64 on top of the definition's fit (symmetry.fit_transform): the quaternion's sign, the
    choice of m, `last` from the by-value arguments or the control words, the gains, the clip, the move and the composition.  idx: the
    step index (None: no t_dev, never the last).  Returns order_m, theta, screw, step [6] and, with rot0 / tr0, pose, tr_update,
    rot_update.  mutant: one of SYM_MUTANTS -
      larger_m             of the two generators that bracket theta the larger m, however near the smaller one is
      no_gcd               m not filtered by gcd(m, n) = 1
      no_w_flip            the quaternion with w < 0 kept: theta = 2 pi - theta about -u
      clip_under_snap      the clip applied to the snapped step too
      gains_swapped        gain_rot on the translation, gain_tr on the rotation
      centre_all_atoms     the all-atom centroid for the CA family
      screw_sign           dtau = + gain s u
      compose_order        rot_update = axis_angle(R(rot_update) R(domega))
      last_off_by_one      last iff idx == num_steps
      last_from_num_steps  the by-value num_steps although the control words are given."""
    p, n = sym_p32(c), c["n"]
    y, x = f64(c["rec_pos"]).reshape(-1, 3, 3), f64(c["lig"][b]).reshape(-1, 3, 3)
    center = "all_atoms" if (c["all_atoms"] or mutant == "centre_all_atoms") else "ca"
    Q, tau, _ = SY.fit_transform(y, x)
    q = SY._quaternion(Q)
    w, v = q[0], q[1:]
    vn = float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    out = dict(order_m=0, theta=0.0, screw=np.nan, step=np.zeros(6))
    if vn > SY.NO_AXIS:
        if mutant == "no_w_flip":
            w, v = -w, -v
        theta, u = 2.0 * math.atan2(vn, w), v / vn
        cen = SY._centroid(x, center)
        s = float(u @ (cen - Q.T @ (cen - tau)))
        best = None
        for m in range(1, n // 2 + 1):
            if mutant != "no_gcd" and math.gcd(m, n) != 1:
                continue
            d = abs(theta - 2.0 * math.pi * m / n)
            if best is None or d < best[0]:
                best = (d, 2.0 * math.pi * m / n, m)
        if mutant == "larger_m":      # the larger of the two generators that bracket theta (or the nearest one's larger neighbour)
            ms = [m for m in range(1, n // 2 + 1) if math.gcd(m, n) == 1]
            above = [m for m in ms if 2.0 * math.pi * m / n >= theta]
            m = above[0] if above else ms[-1]
            best = (0.0, 2.0 * math.pi * m / n, m)
        _, ts, m_sel = best
        last = False
        if idx is not None:
            S = num_steps if (ctl is None or mutant == "last_from_num_steps") else int(ctl[3])
            last = (idx == S) if mutant == "last_off_by_one" else (idx + 1 == S)
        snap = last and bool(p.snap_last)
        g_tr, g_rot = (1.0, 1.0) if snap else ((p.gain_rot, p.gain_tr) if mutant == "gains_swapped" else (p.gain_tr, p.gain_rot))
        st = np.concatenate([(g_tr if mutant == "screw_sign" else -g_tr) * s * u, g_rot * (ts - theta) * u])
        if not snap or mutant == "clip_under_snap":
            st = np.concatenate([SY._clip(st[:3], p.max_tr), SY._clip(st[3:], p.max_rot)])
        out.update(order_m=m_sel, theta=theta, screw=s, step=st)
    if rot0 is not None:
        cen = SY._centroid(x, center)
        st = out["step"]
        Rm = RS.axis_angle_to_matrix(st[3:])
        out["pose"] = ((x - cen) @ Rm.T + cen + st[:3]).reshape(-1)
        out["tr_update"] = f64(tr0) + st[:3]
        R0 = RS.axis_angle_to_matrix(f64(rot0))
        out["rot_update"] = RS.matrix_to_axis_angle(R0 @ Rm if mutant == "compose_order" else Rm @ R0)
    return out


# =====================================================================================================================================
# k_igso3_cdf
# =====================================================================================================================================
def igso3_sigmas():
    """The smallest, the largest and ten more grid values of refine.discrete_sigma(), and three values that are not on the grid."""
    ds = RF.discrete_sigma()
    idx = (0, 1, 6, 50, 137, 250, 400, 555, 700, 850, 998, 999)
    return tuple(float(ds[i]) for i in idx) + (0.3141592653589793, 1.0, float(0.5 * (ds[10] + ds[11])))


def _ld(x):
    return np.asarray(x, np.longdouble)


PI_LD = np.longdouble("3.14159265358979323846264338327950288")      # (pi cancels between pdf and cdf; the pdf rows are held against mpmath)


def igso3_terms(sigma):
    """The table's terms in numpy.longdouble from the definition's float64 inputs (sigma, refine.OMEGA, l): coef [1000], the arguments
    omega (l + 1/2) (exact: 53 + 11 bits), the terms [k][l] and lo = sin(omega / 2)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is not the 80-bit extended format here"
    ls = _ld(np.arange(IGSO3_N))
    s = _ld(float(sigma))
    coef = (2 * ls + 1) * np.exp(-ls * (ls + 1) * (s * s) / 2)
    om = _ld(RF.OMEGA)
    arg = om[:, None] * (ls[None, :] + _ld(0.5))
    lo = np.sin(om / 2)
    return coef, arg, coef[None, :] * np.sin(arg) / lo[:, None], lo


@functools.lru_cache(maxsize=None)
def igso3_ref(sigma):
    """(cdf [1000] float64 = refine.igso3_cdf's formula in extended precision, rounded once; gate [1000]).

    Reference: numpy.longdouble (eps 2^-64) throughout - the whole table in mpmath would take minutes per sigma;
    tests/test_aux_harness_cpu.py holds rows of it against mpmath at 200 bits.
    Gate, counted from k_igso3_cdf, with e = 2^-53 and 1 ulp = 2 e:
      coef_l   (2l+1) exp(x), x = -l(l+1) (sigma sigma) / 2: two roundings of x, exp within 1 ulp, the product: (|x| + 4) e relative
      term     coef sin(arg) / lo: arg = fl(omega (l + 1/2)) moves the sine by e |arg|; sin within 2 ulp (4 e); lo = sin(omega / 2) 5 e;
               product and division 2 e:  coef / lo e |arg| + |term| ((|x| + 4) + 11) e
      e_k      1000 sequential additions: 1000 e sum |term|
      pdf      e_k (1 - cos omega) / pi: cos within 2 ulp and the subtraction, 5 e absolute on 1 - cos; three more roundings
      cdf_k    the scan: 6 shuffles + 15 wave totals + 1, 22 e sum_{j <= k} |pdf_j|; / 1000 * pi: 3 e."""
    coef, arg, terms, lo = igso3_terms(sigma)
    om = _ld(RF.OMEGA)
    e = terms.sum(1)      # (the longdouble pairwise sum of 1000 terms: 10 x 2^-64 sum |terms|, 200 000 times below the gate's e_k term)
    one_m_cos = 2 * np.sin(om / 2) ** 2
    pdf = e * one_m_cos / PI_LD
    cdf = np.cumsum(pdf) / IGSO3_N * PI_LD
    x = np.abs(f64(-np.arange(IGSO3_N) * (np.arange(IGSO3_N) + 1.0)) * float(sigma) ** 2 / 2)
    tabs = np.abs(f64(terms))
    dterm = f64(coef)[None, :] / np.abs(f64(lo))[:, None] * E64 * np.abs(f64(arg)) + tabs * ((x + 4) + 11)[None, :] * E64
    de = dterm.sum(1) + 1000 * E64 * tabs.sum(1)
    omc = f64(one_m_cos)
    dpdf = (de * omc + np.abs(f64(e)) * 5 * E64) / np.pi + 3 * E64 * np.abs(f64(pdf))
    gate = (np.cumsum(dpdf) + 22 * E64 * np.cumsum(np.abs(f64(pdf)))) / IGSO3_N * np.pi + 3 * E64 * np.abs(f64(cdf))
    return f64(cdf), gate


def igso3_mp_rows(sigma, rows):
    """pdf[k] for the rows k in mpmath at 200 bits from the same float64 inputs."""
    import mpmath as mp
    out = []
    with mp.workprec(200):
        s = mp.mpf(float(sigma))
        for k in rows:
            om = mp.mpf(float(RF.OMEGA[k]))
            e = mp.fsum((2 * l + 1) * mp.exp(-l * (l + 1) * s * s / 2) * mp.sin(om * (l + mp.mpf(0.5))) for l in range(IGSO3_N)) / mp.sin(om / 2)
            out.append(e * (1 - mp.cos(om)) / mp.pi)
    return out


# =====================================================================================================================================
# k_start_pose
# =====================================================================================================================================
def hand_tables():
    """name -> (cdf [1000], [(u, expected first index or None)]).  Every value is a float32 number (u is an fp32 draw) so that `>=`
    against the float64 table is decided exactly."""
    k = np.arange(IGSO3_N, dtype=np.float64)
    inc = (k + 1) / 1024.0                                  # strictly increasing, entries on a 2^-10 grid, the last 1000 / 1024
    flat = inc.copy()
    flat[300:400] = flat[300]                               # a flat stretch: the first of the equal entries is the crossing
    dip = inc.copy()
    dip[500:520] = inc[480:500][::-1]                       # a dip: entries 500..519 fall back below entry 499
    tail = np.minimum(inc, 600 / 1024.0)
    tail[700:] -= 2.0 ** -20 * ((k[700:] % 3) - 1)          # a non-monotone tail around the plateau
    g = lambda v: float(f32(v))
    return {
        "increasing": (inc, [(g(0.25), 255), (g(0.2501), 256), (g(1 / 1024.0), 0), (g(2 / 1024.0), 1), (g(0.0), 0), (g(1.0), None),
                             (g(1000 / 1024.0), 999), (g(999.5 / 1024.0), 999), (g(0.5 / 1024.0), 0), (g(512 / 1024.0), 511)]),
        "flat": (flat, [(g(301 / 1024.0), 300), (g(301.5 / 1024.0), 400), (g(300.5 / 1024.0), 300), (g(401 / 1024.0), 400)]),
        "dip": (dip, [(g(490.5 / 1024.0), 490), (g(500 / 1024.0), 499), (g(500.5 / 1024.0), 520), (g(485.5 / 1024.0), 485)]),
        "tail": (tail, [(g(600 / 1024.0), 599), (g(600 / 1024.0 + 2.0 ** -21), 702), (g(0.9), None), (g(599.5 / 1024.0), 599)]),
        "all_below": (inc * 0.5, [(g(0.75), None), (g(1.0), None)]),
        "first_above": (inc + 0.5, [(g(0.25), 0), (g(0.0), 0), (g(0.5), 0)]),
    }


def first_crossing(cdf, u, mutant=None):
    """The rule restated: the first index with cdf[k] >= u, or None.  mutants: 'last' (the last crossing from below: a binary search on a
    table with a dip), 'gt' (cdf[k] > u)."""
    cdf = f64(cdf)
    hit = np.nonzero(cdf > u if mutant == "gt" else cdf >= u)[0]
    if hit.size == 0:
        return None
    if mutant == "last":
        below = np.nonzero(cdf < u)[0]
        return int(below[-1] + 1) if below.size and below[-1] + 1 < len(cdf) else (None if below.size else 0)
    return int(hit[0])


def angle_of(cdf, u, k):
    """The angle the kernel forms from first index k (None: pi)."""
    dw = np.pi / IGSO3_N
    if k is None:
        return np.pi
    if k == 0:
        return dw
    w0, w1 = k * dw, (np.pi if k == IGSO3_N - 1 else (k + 1) * dw)
    return (w1 - w0) / (cdf[k] - cdf[k - 1]) * (u - cdf[k - 1]) + w0


def start_draws64(b, seed):
    """The native draws of trajectory b in float64: Philox blocks (b, 0..3, 0, RNG_START); u = u01(word 0 of block 0) exactly (an fp32
    number); six normals sqrt(-2 ln u_a) cos(2 pi u_b) on word pairs with geom_harness.init_draws64's bound.  Returns (u, axis [3],
    z [3], |dz| of the six)."""
    w = np.stack(gh.philox_np(np.full(4, b), np.arange(4), 0, RNG_START, seed & 0xFFFFFFFF, seed >> 32), -1)      # [block][word]
    u = f64(gh.u01_np(w))
    ua = np.array([u[1, 0], u[1, 2], u[2, 0], u[2, 2], u[3, 0], u[3, 2]])
    ub = np.array([u[1, 1], u[1, 3], u[2, 1], u[2, 3], u[3, 1], u[3, 3]])
    r = np.sqrt(-2.0 * np.log(ua))
    z = r * np.cos(2 * np.pi * ub)
    dz = r * (4 * np.pi + 4) * U + 3 * U * np.abs(z) + 2 * U * r
    return float(u[0, 0]), z[:3], z[3:], dz


def start_ref(start, cdf, u, axis, z, sigma_r3, all_atoms, daxis=0.0, dz=0.0):
    """One trajectory of k_start_pose in float64 from refine.inverse_cdf / forward_marginal's formulas: (rot, tr, pose [L*9], bounds of
    the three).  daxis / dz: the bounds of the draws themselves (0 when injected).  rot / tr: ONE fp32 rounding of float64 values a few
    float64 roundings from the definition's; the pose: the update bound of tests/test_gpu_head_kernels.py."""
    with np.errstate(all="ignore"):
        ang = float(RF.inverse_cdf(np.array([u]), cdf)[0])
        ax = f64(axis)
        n = np.linalg.norm(ax)
        rot, tr = ax / n * ang, sigma_r3 * f64(z)
        drot_v = np.abs(rot) * (U + 8 * E64) + ang * 2 * np.max(daxis) / n + 2.0 ** -149
        dtr_v = np.abs(tr) * (U + 2 * E64) + abs(sigma_r3) * dz + 2.0 ** -149
        x = f64(start).reshape(-1, 3, 3)
        x3 = x.reshape(-1, 3)
        cen = x3.mean(0) if all_atoms else x[:, 1].mean(0)
        pose = (x - cen) @ hh.aa_to_mat64(rot).T + cen + tr
        rad = np.linalg.norm(x3 - cen, axis=-1).max()
        dpose = 2 * rad * (np.linalg.norm(drot_v) + 32 * U) + np.max(dtr_v) + 8 * U * (np.abs(x3).max() + np.abs(cen).max() + np.abs(tr).max())
    return rot, tr, pose.reshape(-1), drot_v, dtr_v, dpose


def start_pose_inputs(L, B, seed=0):
    rng = np.random.default_rng([seed, L, B])
    return (rng.standard_normal((B, L, 9)) * 6 + 2).astype(f32)
