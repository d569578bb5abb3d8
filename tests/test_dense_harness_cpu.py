"""The kernel harness of the node-model GEMMs without a GPU (tests/dense_harness.py, tests/kernels/dense_harness.hip): it builds and
links against the library, the launcher refuses bad shapes before any device work, the float64 restatements agree with numpy, and
the GEMM bound of tests/test_gpu_dense_kernels.py is tight enough to catch a kernel that drops precision."""

import numpy as np
import pytest

import dense_harness as dh
import kernel_harness as kh


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return dh.compile_shim(tmp_path_factory.mktemp("dense_harness"))


@pytest.fixture(scope="module")
def harness(shim):
    return dh.Harness(shim)


def test_library_exports_the_launchers():
    """The harness links against dfm::launch_* by name: a build with hidden visibility would break it silently."""
    out = kh.exported_symbols(dh.LIBDIR + "/libdfmdock_amd.so", True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in dh.LAUNCHERS:
        assert s in syms, s


def test_shim_links(shim, harness):
    out = kh.exported_symbols(shim, False)
    for s in dh.LAUNCHERS:
        assert s in out, s
    assert harness.guard >= 1024


@pytest.mark.parametrize("case", [
    dict(M=64, K=255, Nout=256, lda=256, ldc=256),                                   # K % 32
    dict(M=64, K=272, Nout=256, lda=272, ldc=256),                                   # K % 32 (a multiple of 16)
    dict(M=64, K=256, Nout=128, lda=256, ldc=128),                                   # Nout % 256
    dict(M=64, K=256, Nout=384, lda=256, ldc=384),
    dict(M=64, K=96, Nout=256, lda=256, ldc=256, pro=1),                             # pro 1: K / 2 = 48
    dict(M=100, K=256, Nout=256, lda=256, ldc=256, rows_per_graph=33, stats=True),   # M % rows_per_graph with stats
    dict(M=100, K=256, Nout=256, lda=256, ldc=256, rows_per_graph=33, pro=2),        # ... with pro 2
    dict(M=100, K=256, Nout=256, lda=256, ldc=256, rows_per_graph=0, pro=2),
    dict(M=64, K=256, Nout=512, lda=256, ldc=256, rows_per_graph=64, stats=True),    # stats need Nout = 256
    dict(M=64, K=256, Nout=512, lda=256, ldc=256, epi=2, zbuf=True),                 # zbuf with Nout = 512
    dict(M=64, K=256, Nout=256, lda=258, ldc=256),                                   # lda % 4
    dict(M=64, K=256, Nout=256, lda=256, ldc=254),                                   # ldc % 4
], ids=["K255", "K272", "N128", "N384", "pro1_K96", "stats_M", "pro2_M", "pro2_rpg0", "stats_N512", "zbuf_N512",
        "lda", "ldc"])
def test_split_refuses_bad_shapes(harness, case):
    """launch_gemm_split returns hipErrorInvalidValue for every shape its kernel cannot run, before touching a pointer (all null)."""
    assert harness.validate_split(**case) == dh.HIP_INVALID_VALUE


def test_split_accepts_engine_shapes(harness):
    """The control: the shapes the engine launches are not refused (no device: the launch itself fails, never with InvalidValue)."""
    for case in (dict(M=600, K=512, Nout=256, lda=256, ldc=256, pro=1, rows_per_graph=300, stats=True),
                 dict(M=600, K=256, Nout=256, lda=256, ldc=256, pro=2, epi=1, rows_per_graph=300, zbuf=True),
                 dict(M=600, K=256, Nout=512, lda=256, ldc=256, epi=2),
                 dict(M=64, K=192, Nout=256, lda=256, ldc=256, pro=1)):       # pro 1: K / 2 = 96, a multiple of 32
        assert harness.validate_split(**case) != dh.HIP_INVALID_VALUE, case


def test_split_restatement():
    """split_bf16's tile order [K/32][4][Nout][8]: element (o, k) sits at ((k/32*4 + k%32/8)*Nout + o)*8 + k%8; hi + lo = w to 2^-17."""
    rng = np.random.default_rng(0)
    W = rng.standard_normal((256, 64)).astype(np.float32)
    hi, lo = dh.split_bf16(W)
    assert hi.shape == (2, 4, 256, 8)
    for o, k in ((0, 0), (5, 9), (255, 63), (17, 40)):
        d = ((k // 32 * 4 + k % 32 // 8) * 256 + o) * 8 + k % 8
        assert hi.ravel()[d] == dh.to_bf16_bits(W[o:o + 1, k])[0]
        rec = dh.bf16_to_f32(hi.ravel()[d:d + 1]).astype(np.float64) + dh.bf16_to_f32(lo.ravel()[d:d + 1])
        assert abs(rec[0] - W[o, k]) <= 2.0 ** -17 * abs(W[o, k])
    # RNE of the bf16 conversion, ties included
    x = np.array([1 + 2 ** -8, 1 + 3 * 2 ** -8, 1 + 2 ** -8 + 2 ** -20, -1 - 2 ** -8], np.float32)
    np.testing.assert_array_equal(dh.bf16_to_f32(dh.to_bf16_bits(x)), [1.0, 1 + 2 ** -6, 1 + 2 ** -7, -1.0])


def test_f2h_restatement_matches_numpy():
    """The numpy f2h agrees with np.float16 (IEEE RNE) on finite values below 65504: normals, subnormals, exact ties of both."""
    rng = np.random.default_rng(1)
    e = rng.uniform(-27, 16, 200000)
    x = (np.sign(rng.standard_normal(e.size)) * np.exp2(e)).astype(np.float32)
    ties = []
    for b in range(1, 0x7bff, 97):                       # midpoints between consecutive fp16 values (normal and subnormal)
        lo, hi = np.array([b, b + 1], np.uint16).view(np.float16).astype(np.float64)
        ties.append((lo + hi) / 2)
    x = np.concatenate([x, np.array(ties, np.float32), -np.array(ties, np.float32),
                        np.float32([2 ** -24, 2 ** -25, 3 * 2 ** -26, 2 ** -26, 2 ** -14, 65504.0, 65503.0, 1e-30, 0.0])])
    x = x[np.abs(x) < 65504 + 1]
    np.testing.assert_array_equal(dh.f2h(x), x.astype(np.float16).view(np.uint16))
    # the saturating and NaN cases of f2h
    sp = np.float32([65519.99, 65520.0, 1e30, np.inf, -np.inf, np.nan])
    np.testing.assert_array_equal(dh.f2h(sp), np.uint16([0x7bff, 0x7bff, 0x7bff, 0x7bff, 0xfbff, 0x7e00]))


@pytest.mark.parametrize("kind,K", [("coherent", 256), ("coherent", 512), ("normal", 512)])
def test_bound_has_power(kind, K):
    """Each weaker kernel - bf16 operands only (a_hi w_hi), any two of the three split terms, fp16 operands - exceeds the GEMM bound
    C_SPLIT |A| |W|^T by at least 4x on the coherent inputs the GPU tests use, and the three-term split itself stays well inside it.
    On normal inputs the dropped terms partly cancel; the bound still catches bf16-only and dropped hi x hi there."""
    rng = np.random.default_rng(2)
    A, W = dh.family(kind, rng, 512, K, 256)
    f = dh.product_forms(A, W)
    ratio = {k: float((np.abs(v - f["exact"]) / f["abs"]).max()) for k, v in f.items() if k not in ("exact", "abs")}
    assert ratio["three_terms"] < dh.C_SPLIT / 4, ratio
    weak = ("bf16_only", "no_alo_whi", "no_ahi_wlo", "no_ahi_whi", "fp16_operands") if kind == "coherent" else ("bf16_only", "no_ahi_whi")
    for k in weak:
        assert ratio[k] > 4 * dh.C_SPLIT, (k, ratio)


def test_tile_shape_restatement():
    """tile_shape follows launch_gemm_split's thresholds (2 x CUs 64 x 256 workgroups, CUs / 2 64 x 128 workgroups)."""
    assert dh.tile_shape(512, 256, 256, 256) == "nj2" and dh.tile_shape(511, 256, 256, 256) == "nj1"
    assert dh.tile_shape(64, 256, 256, 256) == "nj1" and dh.tile_shape(63, 256, 256, 256) == "qt"
    assert dh.tile_shape(256, 512, 256, 256) == "nj2" and dh.tile_shape(31, 512, 512, 256) == "qt"
    assert dh.tile_shape(1, 256, 32 * 6, 256) == "nj1"       # the quarter tiles need K / 32 % 4 == 0
