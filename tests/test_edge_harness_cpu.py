"""The kernel harness of the message kernels without a GPU (tests/edge_harness.py, tests/kernels/edge_harness.hip): it builds and links
against the library, the launchers refuse shapes their kernels cannot run before any device work, the numpy restatements of api_model.hip
round-trip, the task-form restatement equals edge_msg_tile_tasks, and the bound of tests/test_gpu_edge_kernels.py is tight enough to
catch a kernel that is subtly wrong."""
import subprocess
import sys

import numpy as np
import pytest

import dense_harness as dh
import edge_harness as eh
import kernel_harness as kh

H = eh.H
S = eh.S


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return eh.compile_shim(tmp_path_factory.mktemp("edge_harness"))


@pytest.fixture(scope="module")
def harness(shim):
    return eh.Harness(shim)


@pytest.fixture(scope="module")
def layer():
    return eh.make_layer(seed=0)


def test_library_exports_the_launchers():
    """The harness links against the launchers by name: a build with hidden visibility would break it silently."""
    out = kh.exported_symbols(eh.LIBDIR + "/libdfmdock_amd.so", True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in eh.LAUNCHERS:
        assert s in syms, s


def test_shim_links(shim, harness):
    out = kh.exported_symbols(shim, False)
    for s in eh.LAUNCHERS:
        assert s in out, s
    assert harness.guard >= 1024


BAD = [("K0", dict(B=1, N=8, R=2, K=0)), ("K61", dict(B=1, N=80, R=2, K=61)), ("K64", dict(B=1, N=80, R=2, K=64)),
       ("B0", dict(B=0, N=8, R=2, K=4)), ("N0", dict(B=1, N=0, R=0, K=4)), ("R_gt_N", dict(B=1, N=8, R=9, K=4)),
       ("R_neg", dict(B=1, N=8, R=-1, K=4))]


@pytest.mark.parametrize("op", ["edge_bf16", "coord_bf16", "edge_f32"])
@pytest.mark.parametrize("name,case", BAD, ids=[b[0] for b in BAD])
def test_launchers_refuse_bad_shapes(harness, op, name, case):
    """hipErrorInvalidValue before any HIP call for shapes the kernels cannot run (all device pointers null)."""
    assert harness.validate(op, **case) == eh.HIP_INVALID_VALUE


@pytest.mark.parametrize("op,last,lig_only", [("edge_bf16", 1, 0), ("edge_bf16", 0, 1), ("edge_f32", 1, 0), ("edge_f32", 0, 1),
                                              ("coord_bf16", 0, 0)])
def test_launchers_refuse_launches_without_ligand(harness, op, last, lig_only):
    """A coordinate update, last-layer or ligand-only launch needs a ligand node (R < N)."""
    assert harness.validate(op, 2, 16, 16, 8, last, lig_only) == eh.HIP_INVALID_VALUE


def test_launchers_accept_engine_shapes(harness):
    """The control: shapes the engine launches are not refused (no device: the launch itself fails, never with InvalidValue)."""
    for op in ("edge_bf16", "edge_f32"):
        for case in (dict(B=8, N=600, R=300, K=60), dict(B=1, N=5, R=4, K=1, last=1), dict(B=3, N=20, R=20, K=33),
                     dict(B=1, N=29, R=0, K=60), dict(B=2, N=40, R=10, K=32, lig_only=1)):
            assert harness.validate(op, **case) != eh.HIP_INVALID_VALUE, (op, case)
    assert harness.validate("coord_bf16", 8, 600, 300, 60) != eh.HIP_INVALID_VALUE


def test_frag_and_bias_restatements():
    """pack_frags places W[n][k] at [kk][nt][lane][e] with n = nt*32 + lane%32, k = kk*16 + (lane/32)*8 + e (frag_channel); both
    forms round-trip to the 16-bit rounding of W; pack_bias hi + lo = SILU_S b within 2^-16 relative + 2^-25, lanes 32..63 zero."""
    rng = np.random.default_rng(0)
    W = (rng.standard_normal((H, H)) * 0.06).astype(np.float32)
    for f16 in (0, 1):
        fr = eh.pack_frags(W, f16)
        assert fr.shape == (16, 8, 64, 8)
        for n, k in ((0, 0), (5, 9), (255, 255), (37, 200)):
            kk, hh, e = k // 16, (k % 16) // 8, k % 8
            got = fr[kk, n // 32, (n % 32) + 32 * hh, e]
            want = dh.f2h(W[n:n + 1, k])[0] if f16 else dh.to_bf16_bits(W[n:n + 1, k])[0]
            assert got == want
        back = eh.unpack_frags(fr, f16)
        rel = 2.0 ** -11 if f16 else 2.0 ** -8
        assert (np.abs(back - W) <= rel * np.abs(W) + 2.0 ** -25).all()
    b = (rng.standard_normal(H) * 0.1).astype(np.float32)
    for f16 in (0, 1):
        v = eh.pack_bias(b, f16).reshape(8, 64)
        assert not v[:, 32:].any()
        x = S * b.astype(np.float64)
        assert (np.abs(eh.unpack_bias(v, f16) - x) <= 2.0 ** -16 * np.abs(x) + eh.SUB16).all()      # (an fp16 lo may be subnormal)


def test_merged_table_restatement(layer):
    """Every T2b row equals the sum of its T rows (times SILU_S) within fp16 rounding; codes round-trip through pack_code."""
    Td = layer["Td"]
    T2 = dh.h_to_f64(layer["slots"]["T2b"]).reshape(eh.NTAB2, H)
    om, th, ph = 22, 5, 10
    want = S * (Td[40 + om] + Td[64 + th] + Td[88 + ph])
    got = T2[(om * 24 + th) * 12 + ph]
    assert (np.abs(got - want) <= eh.C16 * np.abs(want) + eh.SUB16).all()
    rp, d = 65, 39
    want = S * (Td[100 + rp] + Td[d])
    assert (np.abs(T2[6912 + rp * 40 + d] - want) <= eh.C16 * np.abs(want) + eh.SUB16).all()
    assert (np.abs(T2 - layer["T2exact"]) <= eh.C16 * np.abs(layer["T2exact"]) + eh.SUB16).all()
    c = eh.pack_code(39, 22, 22, 10, 65)
    assert [int(x) for x in eh.unpack_code(c)] == [39, 22, 22, 10, 65]


def test_task_form_restatement(harness):
    """tile_tasks equals edge_msg_tile_tasks at 256 CUs (the launcher's fallback without a device) across the sizes around its
    threshold; without a device, device_cus() is 256."""
    cus = harness.cus()
    if cus == 256:
        for B in (1, 2, 3, 8, 16):
            for N in (1, 17, 255, 256, 257, 600, 1024, 2049):
                for K in (1, 32, 33, 60):
                    assert eh.tile_tasks(B, N, K, cus) == harness.tile_tasks(B, N, K), (B, N, K)
    assert eh.tile_tasks(8, 600, 60, 256) and eh.tile_tasks(8, 513, 60, 256) and not eh.tile_tasks(8, 512, 60, 256)
    assert eh.task_form(8, 512, 60, 256) == "dynamic" and eh.task_form(3, 37, 60, 256) == "tile" and eh.task_form(3, 37, 32, 256) == "static"


def test_no_device_cus_fallback(harness):
    ndev = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True).stdout.strip()
    if ndev == "0":
        assert harness.cus() == 256


# ---- the bound's power ----------------------------------------------------------------------------------------------------------
def pkrtz(x):
    """v_cvt_pkrtz_f16_f32: round toward zero to fp16 (finite results: truncation saturates at 65504)."""
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32).astype(np.float16).astype(np.float64)
    over = np.abs(f) > np.abs(x)
    f = np.where(over, np.nextafter(f.astype(np.float16), np.float16(0)).astype(np.float64), f)
    return np.clip(f, -65504, 65504)


def emulate_f16_rows(L, A_s, Bm_s, code, rad):
    """The shipped arithmetic of k_edge_msg<1, 1> per edge row (gm in the scaled unit): fp16 table rows and operands, two packed fp16
    adds, fp32 fma_mix adds, the biased exp2 / rcp SiLU, v_cvt_pkrtz, fp16 weight fragments and bias pair; sums exact (fp32 roundings of
    the accumulation are not modelled)."""
    d, om, th, ph, rp = (x.astype(np.int64) for x in eh.unpack_code(code))
    T2 = dh.h_to_f64(L["slots"]["T2b"]).reshape(eh.NTAB2, H)
    t0 = T2[(om * 24 + th) * 12 + ph]
    t1 = T2[6912 + rp * 40 + d]
    f16 = lambda x: np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
    s16 = f16(f16(t0 + t1) + dh.h_to_f64(dh.f2h(Bm_s)))
    ah = dh.h_to_f64(dh.f2h(A_s))
    wrs = L["slots"]["w_r_s"].astype(np.float64)
    pv = (wrs * np.asarray(rad, np.float64)[:, None] + ah).astype(np.float32).astype(np.float64)
    pv = (pv + s16).astype(np.float32).astype(np.float64)
    c = 0.999755859375
    m = pkrtz(pv / (np.exp2(pv) * c + c))
    W2 = eh.unpack_frags(L["slots"]["W2f16"], 1)
    acc = m @ W2.T + eh.unpack_bias(L["slots"]["b2p16"], 1)
    m2 = acc / (1 + np.exp2(acc))
    g = 1 / (1 + np.exp2(m2 @ L["att_w"].astype(np.float64) + np.float32(L["att_b"] * np.float32(S))))
    return m2 * g[:, None]


def power_inputs(L, seed, B=2, N=24, K=60):
    rng = np.random.default_rng(seed)
    hfeat = rng.standard_normal((B, N, H))
    _, _, A_s, Bm_s = eh.node_operands(L, hfeat)
    edges = rng.integers(0, N, (B, N, K))
    codes = eh.pack_code(rng.integers(0, 40, (B, N, K)), rng.integers(0, 23, (B, N, K)), rng.integers(0, 23, (B, N, K)),
                         rng.integers(0, 11, (B, N, K)), rng.integers(0, 66, (B, N, K)))
    rad = rng.uniform(0, 400, (B, N, K)).astype(np.float32)
    return A_s, Bm_s, edges, codes, rad


def rows_of(A_s, Bm_s, edges, codes, rad, b, a_traj=None):
    N, K = edges.shape[1:]
    i = np.repeat(np.arange(N), K)
    j = edges[b].ravel()
    ab = b if a_traj is None else a_traj
    return A_s[ab, i], Bm_s[b, j], j, codes[b].ravel(), rad[b].ravel()


def test_bound_has_power(layer):
    """The exact emulation of the fp16-operand kernel stays under the bounds of tests/test_gpu_edge_kernels.py, reaching 1/10 of the
    stored-message bound on some element (1/100 of the agg bound: that bound adds worst-case magnitudes over 60 rows of 256-term
    contractions, while the actual errors have random signs and grow like the square root of the term count).  Each weaker form
    exceeds a bound at least tenfold on some element: any one of the five table rows dropped (stored messages), one edge slot dropped
    or duplicated at K = 60 (agg against the launch's own stored messages, agg_rows_bound), a masked row left ungated (a stored masked
    row must be exactly zero; in agg at K = 4), and the wrong trajectory's A (agg)."""
    A_s, Bm_s, edges, codes, rad = power_inputs(layer, 1)
    K = edges.shape[2]
    b = 0
    a, bm, j, code, rd = rows_of(A_s, Bm_s, edges, codes, rad, b)
    ref = eh.edge_rows(layer, a, bm, j, code, rd, f16=1, aw16=1)
    agg, bound = eh.agg_from_rows(ref["gm"], ref["e_gm"], K)
    sbound = eh.store_bound(ref["gm"], ref["e_gm"], 1)
    emu = emulate_f16_rows(layer, a, bm, code, rd)
    agg_emu = emu.reshape(-1, K, H).sum(1) / S
    ratio = np.abs(agg_emu - agg) / bound
    assert 0.01 <= ratio.max() < 1, ratio.max()
    rs = np.abs(emu - ref["gm"]) / sbound                                             # the stored messages, row by row
    assert 0.1 <= rs.max() < 1, rs.max()

    def worst(weak_agg):
        return float((np.abs(weak_agg - agg) / bound).max())

    def worst_row(weak_gm):
        return float((np.abs(weak_gm - ref["gm"]) / sbound).max())

    for lo, hi in ((0, 40), (40, 64), (64, 88), (88, 100), (100, 166)):                # d, omega, theta, phi, relpos rows
        Lw = dict(layer, Td=layer["Td"].copy())
        Lw["Td"][lo:hi] = 0
        w = eh.edge_rows(Lw, a, bm, j, code, rd, f16=1, aw16=1)
        assert worst_row(w["gm"]) > 10, (lo, worst_row(w["gm"]))
    # agg against the launch's own stored messages: the emulated kernel passes, a dropped or duplicated slot does not
    stored = emu.astype(np.float16).astype(np.float64)
    g = stored.reshape(-1, K, H)
    cb = eh.agg_rows_bound(stored, K, 1)
    assert (np.abs(agg_emu - g.sum(1) / S) / cb).max() < 1
    gf = emu.reshape(-1, K, H)
    assert (np.abs(gf[:, :K - 1].sum(1) / S - g.sum(1) / S) / cb).max() > 10          # slot K - 1 dropped from the sum
    assert (np.abs((gf.sum(1) + gf[:, 0] - gf[:, K - 1]) / S - g.sum(1) / S) / cb).max() > 10     # slot 0 twice
    # a masked row left ungated: its stored value is no longer the exact zero the GPU tests require, and agg moves
    N = edges.shape[1]
    ii = np.arange(N)
    masked = eh.edge_rows(layer, A_s[b, ii], Bm_s[b, ii], ii, np.zeros(N, np.uint32), np.zeros(N, np.float32), f16=1, aw16=1)
    assert (np.abs(masked["gm"]).max(1) > 0).all()
    k4 = 4
    gr = ref["gm"].reshape(-1, K, H)
    agg4, bound4 = eh.agg_from_rows(gr[:, :k4].reshape(-1, H), ref["e_gm"].reshape(-1, K, H)[:, :k4].reshape(-1, H), k4)
    assert float((np.abs((gr[:, :k4].sum(1) + masked["gm"]) / S - agg4) / bound4).max()) > 10
    a2, bm2, j2, code2, rd2 = rows_of(A_s, Bm_s, edges, codes, rad, b, a_traj=1)
    w = eh.edge_rows(layer, a2, bm2, j2, code2, rd2, f16=1, aw16=1)
    assert worst(w["gm"].reshape(-1, K, H).sum(1) / S) > 10                           # wrong trajectory's A
