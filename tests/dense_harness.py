"""Kernel-level harness of the node-model GEMMs and GraphNorm statistics (tests/kernels/dense_harness.hip), and their float64 references.

The shim drives the shipped launchers of dfmdock_amd/libdfmdock_amd.so (dfm::launch_gemm_split, launch_gemm_f32, launch_gn_stats)
under the guard-band protocol of tests/kernel_harness.py.  This module binds it and restates, in numpy, what the engine does on the
host for these kernels: the split-bf16 weight tiles of api_model.hip's split_bf16 ([K/32][4][Nout][8] bf16 hi / lo) and the fp16 conversion
f2h of dfm_device.h.

Run as a script (`python dense_harness.py child SHIM IN.npz OUT.npz`) it replays a list of launches stored in IN.npz and writes every
output to OUT.npz: the tile-shape tests run it in child processes, because the launcher reads its shape overrides once per process.
"""
import ctypes as C
import functools
import sys

import numpy as np

import kernel_harness as kh
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, LIBDIR, ROOT, Out, guards_intact, hipcc, replay, save_launches      # noqa: F401 (re-exported)

LAUNCHERS = ("_ZN3dfm17launch_gemm_splitERKNS_8GemmArgsEPKtS4_P12ihipStream_t",
             "_ZN3dfm15launch_gemm_f32ERKNS_8GemmArgsEP12ihipStream_t",
             "_ZN3dfm15launch_gn_statsEPKfiiS1_PfS2_S1_S1_P12ihipStream_t")
H = 256
U32 = 2.0 ** -24                  # unit roundoff of fp32

# Bound of the three-term split GEMM relative to |A| |W|^T (derivation: the docstring of test_gpu_dense_kernels.py)
C_SPLIT = 2.0 ** -15

SLOTS = ("A0", "A1", "W", "Whi", "Wlo", "bias", "gn_shift", "gn_den", "gn_w", "gn_b", "gn_part", "gn_ms", "R",
         "C", "C2", "C2b", "Cb", "stat_part", "zbuf")
INTS = ("M", "K", "Nout", "lda", "ldw", "ldc", "pro", "epi", "rows_per_graph", "a0_period", "r_period", "a0_offset", "gn_B", "gn_N")
OPS = ("split", "f32", "gn_stats")


class Call(C.Structure):
    _fields_ = [("buf", kh.Buf * len(SLOTS))] + [(n, C.c_int) for n in INTS]


compile_shim = functools.partial(kh.compile_shim, "dense")


class Harness(kh.KernelHarness):
    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)
        self.lib.dh_validate_split.argtypes = [C.c_int] * 10
        self.lib.dh_validate_split.restype = C.c_int
        self.lib.dh_device_cus.argtypes = [C.POINTER(C.c_int)]

    def cus(self):
        n = C.c_int(0)
        e = self.lib.dh_device_cus(C.byref(n))
        assert e == HIP_SUCCESS, f"hipDeviceGetAttribute: {e}"
        return n.value

    def validate_split(self, M, K, Nout, lda, ldc, pro=0, epi=0, rows_per_graph=0, stats=False, zbuf=False):
        return self.lib.dh_validate_split(M, K, Nout, lda, ldc, pro, epi, rows_per_graph, int(stats), int(zbuf))


# ---- host restatements --------------------------------------------------------------------------------------------------------
def to_bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (f2bf of dfm_device.h and the device conversion, finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_hi_lo(x):
    """x = hi + lo + r as the kernels split fp32 values: hi = bf16(x), lo = bf16(x - hi) (both RNE).  Returns float32 arrays."""
    x = np.asarray(x, np.float32)
    hi = bf16_to_f32(to_bf16_bits(x))
    lo = bf16_to_f32(to_bf16_bits((x - hi).astype(np.float32)))
    return hi, lo


def split_bf16(W):
    """api_model.hip split_bf16: W [Nout][K] fp32 -> (hi, lo) bf16 bits in the tile order [K/32][4][Nout][8]."""
    W = np.asarray(W, np.float32)
    Nout, K = W.shape
    assert K % 32 == 0
    hi_bits = to_bf16_bits(W)
    lo_bits = to_bf16_bits((W - bf16_to_f32(hi_bits)).astype(np.float32))
    tile = lambda b: np.ascontiguousarray(b.reshape(Nout, K // 32, 4, 8).transpose(1, 2, 0, 3))
    return tile(hi_bits), tile(lo_bits)


def f2h(x):
    """dfm_device.h f2h: fp32 -> fp16 bits, round to nearest even, +-65504 for overflow and inf, NaN -> (sign | 0x7e00)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7fffffff
    out = np.zeros(u.shape, np.int64)
    nan = a > 0x7f800000
    sat = ~nan & (a >= 0x477ff000)
    zero = a < 0x33000001
    sub = ~nan & ~sat & ~zero & (a < 0x38800000)
    nrm = ~nan & ~sat & ~zero & ~sub
    out[nan] = 0x7e00
    out[sat] = 0x7bff
    # subnormal half
    sh = 126 - (a >> 23)
    m = (a & 0x7fffff) | 0x800000
    shs = np.where(sub, sh, 1)
    rem = m & ((1 << shs) - 1)
    half = 1 << (shs - 1)
    ms = m >> shs
    ms = ms + ((rem > half) | ((rem == half) & ((ms & 1) == 1)))
    out[sub] = ms[sub]
    # normal
    b = a + 0xc8000000 - (1 << 32)          # rebias exponent 127 -> 15 (the uint32 add wraps)
    b = b & 0xffffffff
    rem = b & 0x1fff
    b = b >> 13
    b = b + ((rem > 0x1000) | ((rem == 0x1000) & ((b & 1) == 1)))
    out[nrm] = b[nrm]
    return (out | sign).astype(np.uint16)


def h_to_f64(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def silu64(y):
    return y / (1.0 + np.exp(-y))


def graphnorm64(u, N, w, b, ms):
    """torch_geometric GraphNorm (batch = None per trajectory) in float64: rows grouped N at a time.  Returns (y, shift, den, mean)."""
    u = np.asarray(u, np.float64).reshape(-1, N, u.shape[-1])
    mean = u.mean(1, keepdims=True)
    shift = mean * np.asarray(ms, np.float64)
    var = ((u - shift) ** 2).mean(1, keepdims=True)
    den = np.sqrt(var + 1e-5)
    y = np.asarray(w, np.float64) * (u - shift) / den + np.asarray(b, np.float64)
    return y.reshape(-1, u.shape[-1]), shift[:, 0], den[:, 0], mean[:, 0]


def half_stats64(C, N):
    """(mean, M2) in float64 of every 32-row half of every trajectory of C [B*N][256]: [B][ceil(N/32)][256][2]."""
    C = np.asarray(C, np.float64).reshape(-1, N, C.shape[-1])
    T = (N + 31) // 32
    out = np.zeros((C.shape[0], T, C.shape[-1], 2))
    for t in range(T):
        blk = C[:, t * 32:min(N, t * 32 + 32)]
        m = blk.mean(1)
        out[:, t, :, 0] = m
        out[:, t, :, 1] = ((blk - m[:, None]) ** 2).sum(1)
    return out


# ---- input families -----------------------------------------------------------------------------------------------------------
def coherent(rng, shape, scale=1.0):
    """All-positive values x = h + 0.49 ulp_fp16(h), h a bf16 value in [0.5, 2): bf16(x) = fp16(x) = h, so the low split part
    lo = x - h and the fp16 rounding error have the SAME sign everywhere - precision a kernel drops cannot average out in a sum.
    `scale` must be a power of two (keeps the construction exact)."""
    m = 1.0 + np.floor(rng.random(shape) * 128) / 128          # 8 significant bits: bf16-representable
    e = rng.integers(-1, 1, shape)
    h = np.ldexp(m, e)
    x = (h + 0.49 * np.ldexp(1.0, e - 10)).astype(np.float32)
    return (x * np.float32(scale)).astype(np.float32)


def family(kind, rng, M, K, Nout):
    """(A [M][K], W [Nout][K]) of one input family.  'normal': N(0, 1) activations, N(0, 1/K) weights; 'coherent': see coherent()."""
    if kind == "normal":
        return (rng.standard_normal((M, K)).astype(np.float32),
                (rng.standard_normal((Nout, K)) / np.sqrt(K)).astype(np.float32))
    assert kind == "coherent"
    return coherent(rng, (M, K)), coherent(rng, (Nout, K), 2.0 ** -5)


def product_forms(A, W):
    """float64 products of the fp32 operands as the kernel and five weaker kernels would form them (exact arithmetic on the parts)."""
    A = np.asarray(A, np.float32); W = np.asarray(W, np.float32)
    ah, al = split_hi_lo(A)
    wh, wl = split_hi_lo(W)
    d = lambda x: np.asarray(x, np.float64)
    hh, hl, lh = d(ah) @ d(wh).T, d(ah) @ d(wl).T, d(al) @ d(wh).T
    a16 = A.astype(np.float16).astype(np.float64)
    w16 = W.astype(np.float16).astype(np.float64)
    return {"exact": d(A) @ d(W).T, "abs": np.abs(d(A)) @ np.abs(d(W)).T, "three_terms": hh + hl + lh, "bf16_only": hh,
            "no_alo_whi": hh + hl, "no_ahi_wlo": hh + lh, "no_ahi_whi": hl + lh, "fp16_operands": a16 @ w16.T}


def tile_shape(row_tiles, Nout, K, cus):
    """The instantiation launch_gemm_split (kernels_dense.hip) picks: 'nj2' (64 x 256), 'nj1' (64 x 128) or 'qt' (64 x 64)."""
    if row_tiles * (Nout // 256) >= 2 * cus:
        return "nj2"
    if row_tiles * (Nout // 128) < cus // 2 and (K // 32) % 4 == 0:
        return "qt"
    return "nj1"


# env of a child that forces one tile shape through the launcher's own diagnostics switches
FORCE_ENV = {"nj2": {"DFM_GEMM_NARROW_MAXWG": "0"},
             "nj1": {"DFM_GEMM_NARROW_MAXWG": "1000000000", "DFM_GEMM_QUARTER_MAXWG": "0"},
             "qt": {"DFM_GEMM_NARROW_MAXWG": "1000000000", "DFM_GEMM_QUARTER_MAXWG": "1000000000"}}


if __name__ == "__main__":
    kh.child_main(Harness, sys.argv)
