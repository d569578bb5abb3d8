"""The node-model GEMMs (k_gemm_split in all six instantiations, k_gemm_f32 / k_gemm_f32v) and the GraphNorm statistics, kernel by
kernel against float64 computed from the same fp32 inputs, through the host shim of tests/dense_harness.py.

GEMM bound of k_gemm_split, per output element (r, c), relative to S = (|A| |W|^T)[r, c]:
  * split: x = hi + lo + d with hi = bf16(x), lo = bf16(x - hi): |lo| <= 2^-9 |x|, |d| <= 2^-9 |lo| <= 2^-18 |x|.  The kernel forms
    a_hi w_hi + a_hi w_lo + a_lo w_hi; what it leaves out of a w is a_lo w_lo + d_a w + a d_w (+ products of the small parts):
    <= (2^-18 + 2^-18 + 2^-18) |a w| = 3 * 2^-18 |a w| < 2^-16.4 |a w|.
  * accumulation: every 32 x 32 x 16 MFMA adds 16 exact bf16 products to the fp32 accumulator; 3 K / 16 <= 96 roundings of a partial
    sum bounded by S: <= 96 * 2^-24 S < 2^-17.4 S (K <= 512).
  * together < 2^-15.8 S, so C_SPLIT = 2^-15.  The bias / residual adds round once each: + 2 u (|out| + |bias| + |R|), u = 2^-24;
    a 16-bit output rounds once more: + 2^-11 |out| + 2^-25.
  * tight: test_dense_harness_cpu.py::test_bound_has_power - bf16-only operands, each two-of-three-term form and fp16 operands all
    exceed 4 C_SPLIT on the coherent inputs used below, and the exact three-term split stays under C_SPLIT / 4.
With the GraphNorm + SiLU prologue the kernel's activations carry their own error (act_err below), propagated as act_err |W|^T.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_harness as dh
from dense_harness import Out

pytestmark = pytest.mark.gpu

U = dh.U32
N_DEFAULT = 300


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return dh.compile_shim(tmp_path_factory.mktemp("dense_harness_gpu"))


@pytest.fixture(scope="module")
def h(shim):
    return dh.Harness(shim)


@pytest.fixture(scope="module")
def cus(h):
    c = h.cus()
    assert c > 0
    return c


# ---- launch descriptions ------------------------------------------------------------------------------------------------------
def split_launch(M, K, Nout, A0, W, *, A1=None, bias=None, pro=0, epi=0, R=None, rpg=0, a0_period=0, r_period=0, stats=False,
                 zbuf=False, outs=("C",), ldc=None, gn=None, op="split", a0_offset=0):
    """One launch as {op, bufs, scalars}: inputs are arrays, outputs Out.  gn: dict of gn_shift / gn_den / gn_w / gn_b / gn_part / gn_ms arrays."""
    ldc = ldc or (256 if epi == 2 else Nout)
    bufs = {"A0": A0, "A1": A1, "bias": bias, "R": R}
    if op == "split":
        bufs["Whi"], bufs["Wlo"] = dh.split_bf16(W)
    else:
        bufs["W"] = np.ascontiguousarray(W, np.float32)
        if a0_offset:
            bufs["A0"] = np.concatenate([np.zeros(a0_offset // 4, np.float32), np.ravel(A0)])
    bufs.update(gn or {})
    for s in outs:
        n = M * ldc if s == "C" else M * 256
        bufs[s] = Out(np.uint16 if s in ("C2b", "Cb") else np.float32, n)
    if stats:
        bufs["stat_part"] = Out(np.float32, (M // rpg) * ((rpg + 31) // 32) * 256 * 2)
    if zbuf:
        bufs["zbuf"] = Out(np.float32, M * 256)
    scalars = dict(M=M, K=K, Nout=Nout, lda=A0.shape[-1], ldw=K, ldc=ldc, pro=pro, epi=epi, rows_per_graph=rpg, a0_period=a0_period,
                   r_period=r_period, a0_offset=a0_offset)
    return {"op": op, "bufs": bufs, "scalars": scalars}


def run(h, L):
    r = h.run(L["op"], L["bufs"], **L["scalars"])
    assert r["err"] == dh.HIP_SUCCESS, f"hipError {r['err']}"
    for s, v in L["bufs"].items():
        if isinstance(v, Out):
            assert dh.guards_intact(r, s), f"{s}: bytes outside the output block changed"
    return r


def a_rows(A0, M, period):
    return A0[np.arange(M) % period] if period else A0[:M]


def den_rel_bound(u, N, ms, fused):
    """Relative error bound of the den GraphNorm's prologue uses, per trajectory and channel.
    Both paths: the shift is an fp32 value sft = fp32(fp32(mean) * mean_scale) (|sft - shift| <= 2u |shift|), and the variance is
    taken about it: var' - var = 2 (mean - shift) (shift - sft) + (shift - sft)^2.
    fused (stat_part -> gn_finish_col): the statistics come from fp32 (mean, M2) per 32-row half.  Per half t of n_t rows, range r_t,
    mean m_t (shifted sums about the half's first value over 8-row lane groups, two Chan merge levels):
      mean error e_t <= 4u |m_t| + 16u r_t;  M2 error <= 4u n_t (n_t r_t^2 + 4 r_t (|m_t| + r_t))
    merged in float64, the pooled M2 picks up 2 n_t |m_t - mean| e_t + n_t e_t^2.  (unfused, k_gn_stats: float64 sums, exact here.)
    den = sqrt(var + eps): half the relative error of var, + 4u for the fp32 rounding of var, sqrtf and the fold."""
    u = np.asarray(u, np.float64).reshape(-1, N, np.shape(u)[-1])
    mean = u.mean(1)
    shift = mean * np.asarray(ms, np.float64)
    var = ((u - shift[:, None]) ** 2).mean(1)
    es = 2 * U * np.abs(shift)
    err = N * (2 * np.abs(mean - shift) * es + es * es)
    if fused:
        for t in range(0, N, 32):
            blk = u[:, t:t + 32]
            n = blk.shape[1]
            m = blk.mean(1)
            r = blk.max(1) - blk.min(1)
            em = 4 * U * np.abs(m) + 16 * U * r
            err = err + 4 * U * n * (n * r * r + 4 * r * (np.abs(m) + r)) + 2 * n * np.abs(m - mean) * em + n * em * em
    return 0.5 * (err / N) / (var + 1e-5) + 4 * U


def gn_activation(u, N, w, b, ms, den_rel):
    """float64 SiLU(GraphNorm(u)) and the error bound of the kernel's activation: y = fmaf(x, sc, sh) with the folded sc = w / den,
    sh = b - sc shift in fp32 (den relative error den_rel, per trajectory and channel), SiLU by exp2 / rcp (a few ulp plus the
    rounding of y log2 e: (8 + |y|) u relative)."""
    y, shift, den, _ = dh.graphnorm64(u, N, w, b, ms)
    x = np.asarray(u, np.float64)
    sc = np.repeat(np.asarray(w, np.float64) / den, N, 0)
    sft = np.repeat(shift, N, 0)
    er = np.repeat(den_rel, N, 0) if np.ndim(den_rel) else den_rel
    a = dh.silu64(y)
    yerr = (np.abs(x * sc) + np.abs(sc * sft)) * (er + 4 * U) + 4 * U * (np.abs(b) + np.abs(y))
    return a, 1.1 * yerr + (8 + np.abs(y)) * U * np.abs(a) + 1e-38


def check_out(name, got, ref, bound, fracs=None):
    bad = ~(np.abs(got - ref) <= bound)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} outside the bound; worst |err| / bound = "
                           f"{float(np.nanmax(np.abs(got - ref) / bound)):.3g} at {np.argwhere(bad)[:3].tolist()}")
    if fracs is not None:
        fracs[name] = float((np.abs(got - ref) / bound).max())


def worst_ratio(got, ref, S):
    """max |out - ref| / (|A||W|^T): the figure the GEMM bound C_SPLIT limits."""
    return float((np.abs(got - ref) / S).max())


def check_gemm(r, L, A_eff, W, *, act_err=None, report=None, fracs=None):
    """Every output of launch L against float64 of A_eff (the prologue's output, [M][K]) times W^T + bias (+ R)."""
    M, Nout, epi, ldc = L["scalars"]["M"], L["scalars"]["Nout"], L["scalars"]["epi"], L["scalars"]["ldc"]
    W64 = np.asarray(W, np.float64)
    acc = A_eff @ W64.T
    S = np.abs(A_eff) @ np.abs(W64).T
    err = dh.C_SPLIT * S if L["op"] == "split" else (L["scalars"]["K"] + 4) * U * S
    if act_err is not None:
        err = err + act_err @ np.abs(W64).T
    bias = L["bufs"]["bias"]
    b64 = np.zeros(Nout) if bias is None else np.asarray(bias, np.float64)
    ref = acc + b64
    Rf = 0.0
    if epi == 1:
        R = L["bufs"]["R"].astype(np.float64)
        Rf = a_rows(R, M, L["scalars"]["r_period"])
        ref = ref + Rf
    b32 = err + 2 * U * (np.abs(ref) + np.abs(b64) + np.abs(Rf))
    b16 = b32 * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    outs = L["bufs"]      # (the output slots: no input has one of their names)
    if "C" in outs:
        C = r["C"].reshape(M, ldc)
        if epi == 2:
            check_out("C", C[:, :256].astype(np.float64), ref[:, :256], b32[:, :256], fracs)
        else:
            check_out("C", C[:, :Nout].astype(np.float64), ref, b32)
            assert (C[:, Nout:].view(np.uint32) == 0xffffffff).all(), "C: the padding columns past Nout changed"
        if report is not None:
            cols = slice(0, 256) if epi == 2 else slice(0, Nout)
            report.append(worst_ratio(C[:, cols].astype(np.float64), ref[:, cols], S[:, cols]))
    if "Cb" in outs:
        check_out("Cb", dh.h_to_f64(r["Cb"]).reshape(M, 256), ref[:, :256], b16[:, :256], fracs)
    if "C2" in outs:
        check_out("C2", r["C2"].reshape(M, 256).astype(np.float64), ref[:, 256:], b32[:, 256:], fracs)
    if "C2b" in outs:
        check_out("C2b", dh.h_to_f64(r["C2b"]).reshape(M, 256), ref[:, 256:], b16[:, 256:], fracs)
    if "zbuf" in outs:
        assert (r["zbuf"].view(np.uint32) == 0).all(), "zbuf is not exactly zero over [M][256]"
    return ref


def check_stat_part(r, L, C):
    """stat_part = (mean, M2) per 32-row half of every trajectory, against float64 of the kernel's own fp32 C (bound: the fused
    per-half terms of den_rel_bound, from the fp32 shifted sums and the Chan merges of the kernel)."""
    N = L["scalars"]["rows_per_graph"]
    sp = r["stat_part"].reshape(-1, (N + 31) // 32, 256, 2).astype(np.float64)
    assert np.isfinite(sp).all(), "stat_part: a slot was not written (sentinel left) or is not finite"
    ref = dh.half_stats64(C, N)
    Cg = np.asarray(C, np.float64).reshape(-1, N, 256)
    for t in range(ref.shape[1]):
        blk = Cg[:, t * 32:t * 32 + 32]
        n, m = blk.shape[1], np.abs(ref[:, t, :, 0])
        rg = blk.max(1) - blk.min(1)
        em = 4 * U * m + 16 * U * rg
        eM2 = 4 * U * n * (n * rg * rg + 4 * rg * (m + rg)) + 1e-30
        check_out(f"stat_part mean, half {t}", sp[:, t, :, 0], ref[:, t, :, 0], em + 1e-38)
        check_out(f"stat_part M2, half {t}", sp[:, t, :, 1], ref[:, t, :, 1], eM2)
    return sp


def gn_params(rng):
    return dict(gn_w=(1 + 0.3 * rng.standard_normal(256)).astype(np.float32), gn_b=(0.3 * rng.standard_normal(256)).astype(np.float32),
                gn_ms=(0.5 + 0.5 * rng.random(256)).astype(np.float32))


def gn_stats_launch(u, B, N, ms, w=None, b=None):
    return {"op": "gn_stats", "bufs": {"A0": u, "gn_ms": ms, "gn_w": w, "gn_b": b, "C": Out(np.float32, B * 256), "C2": Out(np.float32, B * 256)},
            "scalars": dict(gn_B=B, gn_N=N)}


# ---- the node model's launch chain at one size --------------------------------------------------------------------------------
def node_chain(h, rng, B, N, *, kind="normal", fused=True, zbuf=True, r_period=True, check=True):
    """node_mlp.0 (pro 1 concat, a0_period = N, stat_part) -> [launch_gn_stats fold] -> node_mlp.3 (pro 2, epi 1 residual, zbuf),
    as the 16-bit engine runs them, each checked against float64.  Returns (launches, results)."""
    M = B * N
    # the trajectory-independent draws first: trajectory 0's data is then the same at every B (test_split_batch_invariance)
    h0 = dh.family(kind, rng, N, 256, 1)[0]
    W3 = dh.family(kind, rng, 1, 512, 256)[1]         # [256][512]
    b3 = (0.1 * rng.standard_normal(256)).astype(np.float32)
    g = gn_params(rng)
    W4 = (rng.standard_normal((256, 256)) / 16).astype(np.float32)
    b4 = (0.1 * rng.standard_normal(256)).astype(np.float32)
    agg = dh.family(kind, rng, M, 256, 1)[0]
    Rm = h0 if r_period else rng.standard_normal((M, 256)).astype(np.float32)
    L1 = split_launch(M, 512, 256, h0, W3, A1=agg, bias=b3, pro=1, rpg=N, a0_period=N, stats=True)
    r1 = run(h, L1)
    u = r1["C"].reshape(M, 256)
    if check:
        check_gemm(r1, L1, np.concatenate([a_rows(h0, M, N), agg], 1).astype(np.float64), W3)
        check_stat_part(r1, L1, u)
    if fused:
        gn = dict(gn_w=g["gn_w"], gn_b=g["gn_b"], gn_part=r1["stat_part"], gn_ms=g["gn_ms"])
        den_rel = den_rel_bound(u, N, g["gn_ms"], True)
    else:
        Ls = gn_stats_launch(u, B, N, g["gn_ms"], g["gn_w"], g["gn_b"])
        rs = run(h, Ls)
        gn = dict(gn_w=g["gn_w"], gn_b=g["gn_b"], gn_den=rs["C2"], gn_shift=rs["C"])
        den_rel = den_rel_bound(u, N, g["gn_ms"], False)
    L2 = split_launch(M, 256, 256, u, W4, bias=b4, pro=2, epi=1, R=Rm, rpg=N, r_period=N if r_period else 0, zbuf=zbuf, gn=gn)
    r2 = run(h, L2)
    if check:
        a, ae = gn_activation(u, N, g["gn_w"], g["gn_b"], g["gn_ms"], den_rel)
        check_gemm(r2, L2, a, W4, act_err=ae)
    return (L1, L2), (r1, r2)


def pick_B(shape, N, K, Nout, cus, stats):
    """A batch size whose launch lands on the instantiation `shape` (launch_gemm_split's thresholds, dense_harness.tile_shape)."""
    for B in range(1, 4096):
        rt = B * ((N + 63) // 64) if stats else (B * N + 63) // 64
        if dh.tile_shape(rt, Nout, K, cus) == shape:
            return B
    raise AssertionError(f"no batch size reaches {shape}")


SHAPES = ("nj2", "nj1", "qt")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "coherent"])
def test_split_plain_vs_float64(h, cus, shape, kind):
    """pro 0, epi 0: K = 256 with bias and a padded ldc (the columns past Nout stay untouched), K = 512 without bias; each instantiation
    reached through M, and for the three-term split the worst |out - ref| / (|A||W|^T) is printed next to C_SPLIT."""
    rng = np.random.default_rng(10)
    for K, with_bias in ((256, True), (512, False)):
        M = pick_B(shape, N_DEFAULT, K, 256, cus, False) * N_DEFAULT
        A, W = dh.family(kind, rng, M, K, 256)
        bias = (rng.standard_normal(256)).astype(np.float32) if with_bias else None
        L = split_launch(M, K, 256, A, W, bias=bias, ldc=260)
        rep = []
        check_gemm(run(h, L), L, A.astype(np.float64), W, report=rep)
        print(f"k_gemm_split {shape} HALF=0 {kind} K={K}: worst |err|/(|A||W|) = {rep[0]:.3g} (bound {dh.C_SPLIT:.3g})")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_split_node_chain_vs_float64(h, cus, shape, fused):
    """node_mlp.0 (pro 1 concat at K = 512, A0 = h0 read in place through a0_period, A1 = agg, stat_part) then node_mlp.3 (pro 2 with
    the statistics finished in its prologue from gn_part - or folded by launch_gn_stats - epi 1 residual with r_period, zbuf)."""
    rng = np.random.default_rng(11)
    B = pick_B(shape, N_DEFAULT, 256, 256, cus, True)
    node_chain(h, rng, B, N_DEFAULT, kind="coherent" if fused else "normal", fused=fused, r_period=fused)
    node_chain(h, rng, B, N_DEFAULT, fused=fused, zbuf=False, r_period=not fused)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("outs", [("C", "C2"), ("C", "C2b"), ("Cb", "C2b"), ("Cb", "C2", "C2b")], ids=["C_C2", "C_C2b", "half", "Cb_C2_C2b"])
def test_split_epi2_vs_float64(h, cus, shape, outs):
    """epi 2 (the [Wa|Wb] projection, Nout = 512): C + C2 (pair heads), C + C2b, Cb + C2b (HALF = 1: the 16-bit engine's), and
    Cb + C2 + C2b (HALF = 0 with both fp16 paths).  Bias on."""
    rng = np.random.default_rng(12)
    B = pick_B(shape, N_DEFAULT, 256, 512, cus, False)
    M = B * N_DEFAULT
    A, W = dh.family("normal", rng, M, 256, 512)
    bias = rng.standard_normal(512).astype(np.float32)
    L = split_launch(M, 256, 512, A, W, bias=bias, epi=2, outs=outs)
    fracs = {}
    check_gemm(run(h, L), L, A.astype(np.float64), W, fracs=fracs)
    print(f"k_gemm_split {shape} HALF={int(outs == ('Cb', 'C2b'))} epi 2 {'+'.join(outs)}: worst |err| / bound "
          + " ".join(f"{k} {v:.3g}" for k, v in fracs.items()))


def test_split_paired_column_tail(h, cus):
    """Nout = 512 at 64 x 256 tiles runs the paired column-block mapping (groups of 8 row tiles, kernels_dense.hip): every
    ceil(M / 64) % 8 tail, and M not a multiple of 64."""
    rng = np.random.default_rng(13)
    base = 64 * cus
    for M in (base + 1, base + 64 * 3 + 5, base + 64 * 7 - 1, base + 64 * 8):
        assert dh.tile_shape((M + 63) // 64, 512, 256, cus) == "nj2"
        A, W = dh.family("normal", rng, M, 256, 512)
        L = split_launch(M, 256, 512, A, W, epi=2, outs=("C", "C2"))
        check_gemm(run(h, L), L, A.astype(np.float64), W)


@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 127, 300, 695, 4096])
def test_split_rows_per_graph(h, N):
    """Trajectory-aligned row tiles at every awkward trajectory length (partial last tiles and halves, halves past the trajectory that
    keep no slot), at three batch sizes: outputs, stat_part, zbuf and guard bands."""
    rng = np.random.default_rng(14 + N)
    for B in ((1, 2, 5) if N < 4096 else (1, 3)):
        node_chain(h, rng, B, N)


def test_stat_part_large_mean(h):
    """stat_part's M2 where E[x^2] - E[x]^2 would lose every digit: columns with |mean| / std from 1e2 to 1e4 (a large bias).  The
    naive fp32 formula is shown to miss the same bound."""
    rng = np.random.default_rng(15)
    N, B = 300, 3
    M = B * N
    A, W = dh.family("normal", rng, M, 256, 256)
    ratio = 10.0 ** np.linspace(2, 4, 256)
    std = np.sqrt((W.astype(np.float64) ** 2).sum(1))
    bias = (ratio * std * np.where(np.arange(256) % 2, 1, -1)).astype(np.float32)
    L = split_launch(M, 256, 256, A, W, bias=bias, rpg=N, stats=True)
    r = run(h, L)
    C = r["C"].reshape(M, 256)
    check_gemm(r, L, A.astype(np.float64), W)
    check_stat_part(r, L, C)
    # power: M2 from fp32 E[x^2] - E[x]^2 over the first half misses the bound the kernel meets
    blk = C[:32].astype(np.float32)
    naive = (blk * blk).sum(0, dtype=np.float32) - np.float32(32) * blk.mean(0, dtype=np.float32) ** 2
    ref = dh.half_stats64(C, N)[0, 0, :, 1]
    rg = blk.max(0).astype(np.float64) - blk.min(0)
    eM2 = 4 * U * 32 * (32 * rg * rg + 4 * rg * (np.abs(ref) + rg))
    assert (np.abs(naive - ref) > eM2).mean() > 0.5


@pytest.mark.parametrize("N", [1, 2, 33, 300, 4096])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("large_mean", [False, True])
def test_gn_stats_vs_float64(h, N, fold, large_mean):
    """launch_gn_stats against a float64 two-pass GraphNorm: shift = mean * mean_scale (two fp32 roundings of a float64 mean: 2u),
    den = sqrt(var + 1e-5) with var taken about that fp32 shift (the shift the kernel returns; fp32 var, sqrtf: 4u), or the folded
    sc = w / den, sh = b - sc * shift (8u)."""
    rng = np.random.default_rng(16 + N)
    B = 3
    g = gn_params(rng)
    u = rng.standard_normal((B * N, 256))
    if large_mean:
        u = u + 10.0 ** np.linspace(2, 4, 256) * np.where(np.arange(256) % 2, 1, -1)
    u = u.astype(np.float32)
    L = gn_stats_launch(u, B, N, g["gn_ms"], g["gn_w"] if fold else None, g["gn_b"] if fold else None)
    r = run(h, L)
    _, shift, _, mean = dh.graphnorm64(u, N, g["gn_w"], g["gn_b"], g["gn_ms"])
    s32 = (mean.astype(np.float32) * g["gn_ms"]).astype(np.float64)        # the kernel's fp32 shift, restated
    den = np.sqrt(((u.reshape(B, N, 256) - s32[:, None]) ** 2).mean(1) + 1e-5)
    gs, gd = r["C"].reshape(B, 256).astype(np.float64), r["C2"].reshape(B, 256).astype(np.float64)
    if fold:
        sc = g["gn_w"] / den
        sh = g["gn_b"] - sc * s32
        check_out("sc", gd, sc, 8 * U * np.abs(sc))
        check_out("sh", gs, sh, 8 * U * (np.abs(g["gn_b"]) + 2 * np.abs(sc * shift)))
    else:
        check_out("shift", gs, shift, 2 * U * np.abs(shift) + 1e-38)
        check_out("den", gd, den, 4 * U * den)


# ---- bitwise claims -------------------------------------------------------------------------------------------------------
def bitwise_launches(rng, N=300, B=4):
    M = B * N
    h0, W3 = dh.family("normal", rng, N, 512, 256)
    agg = rng.standard_normal((M, 256)).astype(np.float32)
    b3 = rng.standard_normal(256).astype(np.float32)
    L1 = split_launch(M, 512, 256, h0[:, :256].copy(), W3, A1=agg, bias=b3, pro=1, rpg=N, a0_period=N, stats=True)
    return L1, M


def test_split_tile_shapes_bitwise(h, shim, tmp_path):
    """One input set in three child processes, each forcing one tile shape through DFM_GEMM_NARROW_MAXWG / DFM_GEMM_QUARTER_MAXWG:
    outputs and stat_part must be bitwise equal.  Two stages: node_mlp.0 with stat_part, then node_mlp.3 with gn_part (fused
    statistics) from the first child's stat_part, the [Wa|Wb] projection in HALF and in fp32 form."""
    rng = np.random.default_rng(20)
    N, B = 300, 4
    L1, M = bitwise_launches(rng, N, B)
    res1 = {}
    for shape in SHAPES:
        res1[shape] = child(shim, tmp_path, shape, [L1], f"s1_{shape}")
    for shape in SHAPES[1:]:
        for k in ("0/C", "0/stat_part"):
            assert np.array_equal(res1[shape][k].view(np.uint32), res1["nj2"][k].view(np.uint32)), (shape, k)
    u = res1["nj2"]["0/C"].reshape(M, 256)
    g = gn_params(rng)
    W4 = (rng.standard_normal((256, 256)) / 16).astype(np.float32)
    L2 = split_launch(M, 256, 256, u, W4, bias=g["gn_b"], pro=2, epi=1, R=rng.standard_normal((M, 256)).astype(np.float32), rpg=N,
                      zbuf=True, gn=dict(gn_w=g["gn_w"], gn_b=g["gn_b"], gn_part=res1["nj2"]["0/stat_part"], gn_ms=g["gn_ms"]))
    Wab = (rng.standard_normal((512, 256)) / 16).astype(np.float32)
    bab = rng.standard_normal(512).astype(np.float32)
    L3 = split_launch(M, 256, 512, u, Wab, bias=bab, epi=2, outs=("Cb", "C2b"))
    L4 = split_launch(M, 256, 512, u, Wab, bias=bab, epi=2, outs=("C", "C2"))
    res2 = {shape: child(shim, tmp_path, shape, [L2, L3, L4], f"s2_{shape}") for shape in SHAPES}
    for shape in SHAPES[1:]:
        for k in res2["nj2"]:
            assert res2[shape][k].tobytes() == res2["nj2"][k].tobytes(), (shape, k)


def child(shim, tmp_path, shape, launches, tag):
    fin, fout = str(tmp_path / f"{tag}_in.npz"), str(tmp_path / f"{tag}_out.npz")
    dh.save_launches(fin, launches)
    env = dict(os.environ)
    env.pop("DFM_GEMM_NARROW_MAXWG", None)
    env.pop("DFM_GEMM_QUARTER_MAXWG", None)
    env.update(dh.FORCE_ENV[shape])
    p = subprocess.run([sys.executable, os.path.join(dh.ROOT, "tests", "dense_harness.py"), "child", shim, fin, fout], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"child {shape} exited {p.returncode}: {p.stdout[-2000:]}{p.stderr[-2000:]}"
    return dict(np.load(fout))


def test_split_batch_invariance(h, cus):
    """With stat_part and the fused pro 2, trajectory 0's rows (outputs, statistics) are bitwise the same at B = 1 and at batch sizes
    that run the other two tile shapes."""
    N = 300
    Bs = [1, pick_B("nj1", N, 256, 256, cus, True), pick_B("nj2", N, 256, 256, cus, True)]
    out = {}
    for B in Bs:
        rng = np.random.default_rng(21)       # the same trajectory-0 data at every B (family draws: h0 shared, agg rows 0..N-1 first)
        L, R = node_chain(h, rng, B, N, check=False)
        out[B] = (R[0]["C"][:N * 256], R[0]["stat_part"][:((N + 31) // 32) * 512], R[1]["C"][:N * 256])
    for B in Bs[1:]:
        for a, b in zip(out[B], out[1]):
            assert a.tobytes() == b.tobytes(), B


@pytest.mark.parametrize("pro", [0, 1, 2, 3])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_f32_aligned_equals_unaligned(h, pro, epi):
    """k_gemm_f32v (16-byte aligned operands) and k_gemm_f32 (A0 offset by 4 bytes) are the same arithmetic: bitwise equal outputs.
    Both within the fp32 accumulation bound (K + 4) u |A||W|^T (an fmaf chain over K) of float64, plus the prologue's error."""
    rng = np.random.default_rng(30 + 4 * pro + epi)
    N, B = 77, 3
    M = B * N
    K = 512 if pro == 1 else 256
    Nout = 512 if epi == 2 else 256
    A0, W = dh.family("normal", rng, M, K // 2 if pro == 1 else K, Nout)
    W = (rng.standard_normal((Nout, K)) / np.sqrt(K)).astype(np.float32)
    A1 = rng.standard_normal((M, K // 2)).astype(np.float32) if pro == 1 else None
    bias = rng.standard_normal(Nout).astype(np.float32)
    R = rng.standard_normal((M, Nout)).astype(np.float32) if epi == 1 else None
    g = gn_params(rng)
    gn = None
    A_eff = A0.astype(np.float64) if pro != 1 else np.concatenate([A0, A1], 1).astype(np.float64)
    act = None
    if pro == 2:
        _, shift, den, _ = dh.graphnorm64(A0, N, g["gn_w"], g["gn_b"], g["gn_ms"])
        s32, d32 = shift.astype(np.float32), den.astype(np.float32)
        gn = dict(gn_shift=s32, gn_den=d32, gn_w=g["gn_w"], gn_b=g["gn_b"])
        o = A0.astype(np.float64) - np.repeat(s32, N, 0)
        y = g["gn_w"].astype(np.float64) * o / np.repeat(d32, N, 0) + g["gn_b"]
        A_eff = dh.silu64(y)
        act = 1.1 * 4 * U * (np.abs(y) + np.abs(g["gn_b"]) + np.abs(g["gn_w"] * o / np.repeat(d32, N, 0))) + 4 * U * np.abs(A_eff)
    elif pro == 3:
        A_eff = dh.silu64(A0.astype(np.float64))
        act = 4 * U * (np.abs(A_eff) + np.abs(A0))
    outs = ("C", "C2", "C2b") if epi == 2 else ("C",)
    kw = dict(A1=A1, bias=bias, pro=pro, epi=epi, R=R, rpg=N, gn=gn, outs=outs, op="f32")
    La = split_launch(M, K, Nout, A0, W, **kw)
    Lu = split_launch(M, K, Nout, A0, W, a0_offset=4, **kw)
    ra, ru = run(h, La), run(h, Lu)
    for s in outs:
        assert ra[s].tobytes() == ru[s].tobytes(), s
    check_gemm(ra, La, A_eff, W, act_err=act)


# ---- the fp16 conversion contract ------------------------------------------------------------------------------------------
def special_values(rng):
    f = lambda bits: np.array(bits, np.uint32).view(np.float32)
    v = [1 + 2 ** -11, 1 + 3 * 2 ** -11, 2049.0, 2051.0, 2 ** -24, 2 ** -25, 3 * 2 ** -26, 2 ** -26, 5 * 2 ** -25, 2 ** -14,
         2 ** -14 - 2 ** -25, 65504.0, 65519.99, 65520.0, 65536.0, 1e30, np.inf, 1.0, 0.1, 1 / 3]
    v = np.array(v + [-x for x in v], np.float32)
    nans = f([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fa00000, 0xffbfffff, 0x7fffffff])
    rnd = (np.sign(rng.standard_normal(4096)) * np.exp2(rng.uniform(-30, 20, 4096))).astype(np.float32)
    return np.concatenate([v, nans, rnd])


def fp16_contract(got, x, name):
    nan_in = np.isnan(x)
    gnan = ((got & 0x7c00) == 0x7c00) & ((got & 0x3ff) != 0)
    assert gnan[nan_in].all(), f"{name}: NaN inputs {x[nan_in & ~gnan].view(np.uint32)} became {got[nan_in & ~gnan]}"
    want = dh.f2h(x)
    bad = ~nan_in & (got != want)
    assert not bad.any(), f"{name}: {x[bad][:6]} -> {got[bad][:6]} (f2h: {want[bad][:6]})"


@pytest.mark.parametrize("shape", SHAPES)
def test_fp16_outputs_follow_f2h(h, cus, shape):
    """With A = 0 the output is the bias: special fp32 values through the fp16 epilogues of k_gemm_split (Cb / C2b, HALF and not) and
    of k_gemm_f32 (C2b).  Non-NaN: the bit pattern of f2h (RNE, +-65504 for overflow and inf).  NaN: a NaN (payload free).  (-0 cannot
    be tested this way: 0 + (-0) = +0.)  Every chunk of 256 values is the bias of BOTH column halves, so each value reaches Cb and
    C2b of every form, and the two engines' conversions are compared on all of them."""
    rng = np.random.default_rng(40)
    vals = special_values(rng)
    vals = np.concatenate([vals, np.zeros((-vals.size) % 256, np.float32)])
    M = {"qt": 64, "nj1": 64 * (cus // 2), "nj2": 64 * cus + 64}[shape]
    assert dh.tile_shape((M + 63) // 64, 512, 256, cus) == shape
    W = rng.standard_normal((512, 256)).astype(np.float32)
    A = np.zeros((M, 256), np.float32)
    seen = {}
    for i in range(0, vals.size, 256):
        x = vals[i:i + 256]
        bias = np.tile(x, 2)
        rf = run(h, split_launch(M, 256, 512, A, W, bias=bias, epi=2, outs=("C", "C2", "C2b"), op="f32"))
        o32 = rf["C2b"].reshape(M, 256)
        assert (o32 == o32[0]).all(), "k_gemm_f32 C2b: rows differ"
        fp16_contract(o32[0], x, "k_gemm_f32 C2b")
        for tag, outs in (("half", ("Cb", "C2b")), ("nothalf", ("Cb", "C2", "C2b"))):
            r = run(h, split_launch(M, 256, 512, A, W, bias=bias, epi=2, outs=outs))
            for s in ("Cb", "C2b"):
                o = r[s].reshape(M, 256)
                name = f"k_gemm_split {tag} {s}"
                assert (o == o[0]).all(), f"{name}: rows differ"
                fp16_contract(o[0], x, name)
                # the two engines agree on the same terms (NaN: both NaN, checked above)
                fin = ~np.isnan(x)
                assert (o[0][fin] == o32[0][fin]).all(), f"{name} differs from k_gemm_f32 C2b"
                seen[name] = seen.get(name, 0) + int(np.isnan(x).sum() + np.isinf(x).sum() + (np.abs(x) == 65504).sum())
    # every output path saw the 7 NaNs, 2 infinities and +-65504
    assert all(v == 11 for v in seen.values()) and len(seen) == 4, seen
