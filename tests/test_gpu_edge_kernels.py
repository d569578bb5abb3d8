"""The message kernels (k_edge_msg in its four instantiations and its row-list form, k_edge_coord, k_edge_f32m, k_l0_gather /
k_l0_gather32) launch by launch against float64 computed from the same fp32 inputs, through the host shim of tests/edge_harness.py.

Inputs.  The 16-bit kernels read the fp32 A_s = S (Wa h + b1) and Bm_s = S Wb h that the [Wa|Wb] GEMM writes (S = SILU_S = -log2 e);
the tests derive Bmb = f2h(Bm_s) and Ah = f2h(A_s) themselves, so fp16 storage belongs to the kernel's error budget.  The reference
uses the exact fp32 values and the float64 table Td.  Every bound below is first-order error propagation computed in float64 from the
actual data, one stage at a time (edge_harness.edge_rows); u = 2^-24.  In the scaled unit of the kernel (values times S):
  1. fp16 storage of the table rows, Bm_j and, with AW16, A_i: the kernel's inputs are known exactly, so their actual rounding errors;
  2. the two packed fp16 adds (t0 + t1, + Bm_j): half an ulp of the binade of each exact sum (2^-25 when subnormal);
  3. the fp32 fma_mix adds (w_r r^2 + A_i, + the fp16 sum) and the fp32 rounding of S w_r: 4u (|w_r r^2| + |A_i| + |pre|);
  4. SiLU on exp2 / rcp: propagated by |silu'(pre)| (the scaled SiLU m' = S silu(pre) has derivative silu'(pre)), + 4u |m'| evaluation;
  5. operand rounding: bf16 RNE 2^-8 |m'| (bf16 keeps 8 significant bits); fp16 the biased v_cvt_pkrtz, within (-0.625, 0.375) ulp
     (kernels_edge.hip, the comment at the conversion): 0.625 (2^-10 |m'| + 2^-24);
  6. weight fragments: bf16 2^-8, fp16 2^-11 of |W2| |m'| (+ 2^-25 sum |m'| for subnormal fp16 weights);
  7. fp32 accumulation of 16 MFMA k-steps plus the bias step: 18u (|W2| |m'| + |S b2|); the bias as a (hi, lo) 16-bit pair: 2^-16 |S b2| + 2^-25
     (an fp16 lo can be subnormal);
  8. epilogue SiLU (|silu'(acc)|, 4u), the gate logit (propagated through att_w, 10u for its fp32 sums), sigmoid by exp2 / rcp
     (g (1 - g) dlogit + 4u g), the gated message (first order in m2 and g) and the K-row sum: (K + 4) u sum |g m2| (node tasks add the
     two tiles' sums, tile tasks add them atomically in either order: the same two roundings);
  9. a stored message: + 2^-11 |gm| + 2^-25 (fp16 RNE) or 2^-8 |gm| (bf16 RNE);
 10. the coordinate MLP, on the stored messages as they are (the test feeds k_edge_coord the decoded buffer, so its bound holds its own
     stage only): weight fragments and accumulation as in 6-7, SiLU, the wc2 dot (12u), clamp (1-Lipschitz), the normalised
     differences (8u each) and the mean (K + 2)u, and (x + f) - x in fp32: 2u (|x| + |f|);
 11. beyond fp16 range the fp16 operand saturates at +-65504 and a stored fp16 message at -65504: the reference clamps (1-Lipschitz).
Last-layer launches also check agg against the launch's own stored messages (edge_harness.agg_rows_bound: their 16-bit rounding and
the fp32 K-row sum), which is tight at any K.
The fp32 kernel k_edge_f32m has its own bound (edge_harness.f32m_rows): fp32 T rows (u) and seven fp32 adds (8u of the sum of
magnitudes), the SiLU on exp2 / rcp with (8 + |x|) u relative (about 3 ulp plus the rounding of x log2 e), 256-term fp32 MFMA
accumulation over 128 k-steps with rounded products (132u |W| |m|), the gate logit's fmaf chain and reduce-scatter (16u), sigmoid_exact
(4u) and the 60-row sum (20u).
Power: tests/test_edge_harness_cpu.py::test_bound_has_power emulates the shipped arithmetic of the fp16-operand kernel in numpy: it
stays under the bounds and reaches 1/10 of the stored-message bound; any one table row dropped exceeds the stored-message bound
tenfold, a dropped or duplicated slot at K = 60 the agg-against-stored-messages bound, and a misapplied ab_bstride the agg bound.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_harness as dh
import edge_harness as eh
from edge_harness import Out

pytestmark = pytest.mark.gpu

H = eh.H
S = eh.S
SENT_F32 = np.frombuffer(b"\xff\xff\xff\xff", np.float32)[0]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return eh.compile_shim(tmp_path_factory.mktemp("edge_harness_gpu"))


@pytest.fixture(scope="module")
def h(shim):
    return eh.Harness(shim)


@pytest.fixture(scope="module")
def cus(h):
    c = h.cus()
    assert c > 0
    return c


@pytest.fixture(scope="module")
def layer():
    return eh.make_layer(seed=0)


def check(name, got, ref, bound):
    got = np.asarray(got, np.float64)
    bad = ~(np.abs(got - ref) <= bound)
    ratio = np.abs(got - ref) / bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} outside the bound; worst |err| / bound = "
                           f"{float(np.nanmax(np.where(np.isnan(ratio), np.inf, ratio))):.3g} at {np.argwhere(bad)[:3].tolist()}")
    print(f"{name}: worst |err| / bound = {float(ratio.max()):.3g}")


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def random_codes(rng, shape):
    return eh.pack_code(rng.integers(0, 40, shape), rng.integers(0, 23, shape), rng.integers(0, 23, shape),
                        rng.integers(0, 11, shape), rng.integers(0, 66, shape))


def make_inputs(L, B, N, K, R, seed, per_traj=True, rad_max=400.0, codes=None, rad=None):
    rng = np.random.default_rng(seed)
    Ab = B if per_traj else 1
    hfeat = rng.standard_normal((Ab, N, H))
    A, Bm, A_s, Bm_s = eh.node_operands(L, hfeat)
    edges = rng.integers(0, N, (B, N, K)).astype(np.int32)
    pos = (rng.standard_normal((B, N, 3)) * 8).astype(np.float32)
    ca4 = np.zeros((B, N, 4), np.float32)
    ca4[..., :3] = pos
    if codes is None:
        codes = random_codes(rng, (B, N, K))
    if rad is None:
        rad = rng.uniform(0, rad_max, (B, N, K)).astype(np.float32)
    return dict(B=B, N=N, K=K, R=R, Ab=Ab, A=A, Bm=Bm, A_s=A_s, Bm_s=Bm_s, edges=edges, codes=np.asarray(codes, np.uint32),
                rad=np.asarray(rad, np.float32), ca4=ca4)


def ints(inp, **kw):
    d = dict(B=inp["B"], N=inp["N"], R=inp["R"], K=inp["K"], ab_bstride=(inp["N"] * H if inp["Ab"] > 1 else 0), att_b=0.0)
    d.update(kw)
    return d


def agg_init(inp, zero):
    n = inp["B"] * inp["N"] * H
    return io(np.zeros(n, np.float32) if zero else np.full(n, SENT_F32, np.float32))


def io(a):
    """An in / out block that starts as array a."""
    a = np.asarray(a)
    return Out(a.dtype, init=a)


def msg_launch(L, inp, *, f16, aw16, last=0, lig_only=0, agg_zero=True, task_ctr=True, repeat=1, mbuf=None, A_s=None):
    A_s = inp["A_s"] if A_s is None else A_s
    Lig = inp["N"] - inp["R"]
    bufs = {"A": A_s, "Bmb": dh.f2h(inp["Bm_s"]), "Ah": dh.f2h(A_s) if aw16 else None, "edges": inp["edges"], "codes": inp["codes"],
            "radial": inp["rad"], "ca4": inp["ca4"]}
    bufs.update({k: v for k, v in L["slots"].items()})
    bufs["agg"] = agg_init(inp, agg_zero)
    if task_ctr:
        bufs["task_ctr"] = io(np.zeros(2 * eh.TASK_CTR_WGS, np.uint32))
    if last:
        bufs["mbuf"] = io(mbuf) if mbuf is not None else Out(np.uint16, inp["B"] * Lig * 64 * H)
        bufs["fout"] = Out(np.float32, inp["B"] * Lig * 3)
    return {"op": "edge_bf16", "bufs": bufs,
            "scalars": ints(inp, last=last, f16=f16, lig_only=lig_only, agg_is_zero=int(agg_zero), repeat=repeat, att_b=L["att_b"])}


def f32_launch(L, inp, *, last=0, lig_only=0, A=None):
    Lig = inp["N"] - inp["R"]
    bufs = {"A": inp["A"] if A is None else A, "Bm": inp["Bm"], "edges": inp["edges"], "codes": inp["codes"], "radial": inp["rad"],
            "ca4": inp["ca4"]}
    bufs.update(L["slots"])
    bufs.update(agg=agg_init(inp, False), range=io(np.zeros(2, np.uint32)))
    if last:
        bufs["fout"] = Out(np.float32, inp["B"] * Lig * 3)
    return {"op": "edge_f32", "bufs": bufs, "scalars": ints(inp, last=last, lig_only=lig_only, att_b=L["att_b"])}


def run(h, Lc):
    r = h.run(Lc["op"], Lc["bufs"], **Lc["scalars"])
    assert r["err"] == dh.HIP_SUCCESS, f"hipError {r['err']}"
    for s, v in Lc["bufs"].items():
        if isinstance(v, Out):
            assert eh.guards_intact(r, s), f"{s}: bytes outside the output block changed"
    if "task_ctr" in r:
        assert not r["task_ctr"].any(), "task counters not zero after the launch"
    return r


def node_rows(inp, nodes):
    """(ab row of A, A rows, Bm rows, j, code, rad) of every edge row s < K of the listed (b, i) nodes, node-major."""
    K = inp["K"]
    b = np.repeat(nodes[:, 0], K)
    i = np.repeat(nodes[:, 1], K)
    s = np.tile(np.arange(K), len(nodes))
    j = inp["edges"][b, i, s]
    ab = b if inp["Ab"] > 1 else np.zeros_like(b)
    return ab, i, j, inp["codes"][b, i, s], inp["rad"][b, i, s]


def all_nodes(B, N, node0=0):
    return np.array([(b, i) for b in range(B) for i in range(node0, N)])


def ref_agg16(L, inp, nodes, f16, aw16, chunk=64):
    aggs, bounds, gms, egms = [], [], [], []
    for c in range(0, len(nodes), chunk):
        nd = nodes[c:c + chunk]
        ab, i, j, code, rad = node_rows(inp, nd)
        r = eh.edge_rows(L, inp["A_s"][ab, i], inp["Bm_s"][ab, j], j, code, rad, f16=f16, aw16=aw16)
        a, bd = eh.agg_from_rows(r["gm"], r["e_gm"], inp["K"])
        aggs.append(a); bounds.append(bd); gms.append(r["gm"]); egms.append(r["e_gm"])
    return np.concatenate(aggs), np.concatenate(bounds), np.concatenate(gms), np.concatenate(egms)


FORMS16 = [(0, 0), (0, 1), (1, 0), (1, 1)]


# ---- k_edge_msg against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16,aw16", FORMS16, ids=["bf16_A32", "bf16_A16", "f16_A32", "f16_A16"])
@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 59, 60])
def test_msg_matches_float64(h, cus, layer, f16, aw16, K):
    """agg of every node against float64, odd N (below K for the large degrees), B = 3 per trajectory (odd K) or pose independent
    (even K: ab_bstride 0), then B = 1; agg zeroed (agg_is_zero) or sentinel (the memset of tile tasks, or every element stored)."""
    for B, N in ((3, 37 if K < 59 else 45), (1, 29)):
        inp = make_inputs(layer, B, N, K, 0, seed=K * 7 + f16 * 2 + aw16, per_traj=(K % 2 == 1))
        form = eh.task_form(B, N, K, cus)
        assert form == ("tile" if h.tile_tasks(B, N, K) else "static") and form != "dynamic"
        for zero in ((True, False) if form == "tile" else (False,)):
            r = run(h, msg_launch(layer, inp, f16=f16, aw16=aw16, agg_zero=zero))
            ref, bound, _, _ = ref_agg16(layer, inp, all_nodes(B, N), f16, aw16)
            check(f"msg[{f16}{aw16} K{K} B{B} {form} zero{int(zero)}]", r["agg"].reshape(-1, H), ref, bound)


def test_task_forms_agree(h, shim, cus, layer, tmp_path):
    """Static node tasks, dynamic node tasks (the per-workgroup counters), tile tasks with agg_is_zero and with the memset: each
    matches float64 on a sample of nodes, all give bitwise the same agg (forced forms in child processes), the counters are zero after
    every launch and a second launch on the same counters gives bitwise the same agg."""
    B, K = 8, 60
    N = 2 * cus                              # B N = 2 x the waves of the device: node tasks (two whole rounds), dynamic with AW16
    inp = make_inputs(layer, B, N, K, 0, seed=11)
    assert eh.task_form(B, N, K, cus) == "dynamic" and not h.tile_tasks(B, N, K)
    L1 = msg_launch(layer, inp, f16=0, aw16=1, agg_zero=False)
    r1 = run(h, L1)
    r2 = run(h, msg_launch(layer, inp, f16=0, aw16=1, agg_zero=False, repeat=2))
    assert np.array_equal(r1["agg"].view(np.uint32), r2["agg"].view(np.uint32)), "second launch on the same counters differs"
    rng = np.random.default_rng(3)
    nodes = np.stack([rng.integers(0, B, 48), rng.integers(0, N, 48)], 1)
    ref, bound, _, _ = ref_agg16(layer, inp, nodes, 0, 1)
    got = r1["agg"].reshape(B, N, H)[nodes[:, 0], nodes[:, 1]]
    check("forms[dynamic]", got, ref, bound)
    forced = [("static", {"DFM_EDGE_DYNAMIC": "0"}, False), ("tile_zero", {"DFM_EDGE_SPLIT": "1"}, True),
              ("tile_memset", {"DFM_EDGE_SPLIT": "1"}, False)]
    for name, env, zero in forced:
        Lc = msg_launch(layer, inp, f16=0, aw16=1, agg_zero=zero)
        fin, fout = str(tmp_path / f"{name}_in.npz"), str(tmp_path / f"{name}_out.npz")
        eh.save_launches(fin, [Lc])
        p = subprocess.run([sys.executable, eh.__file__, "child", shim, fin, fout], env={**os.environ, **env}, capture_output=True,
                           text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-2000:]
        o = np.load(fout)
        assert bool(o["0/agg_guard_ok"]) and not o["0/task_ctr"].any(), name
        assert np.array_equal(o["0/agg"].view(np.uint32), r1["agg"].view(np.uint32)), f"{name}: agg differs from the dynamic form"


def every_code_inputs(layer, seed):
    """One launch that reaches every code: all 23 x 23 x 11 first-table rows and all 40 x 66 second-table rows, radial 0 .. 1e4."""
    N, K = 101, 60
    n = N * K
    e = np.arange(n)
    f = e % (23 * 23 * 11)
    s = e % (40 * 66)
    codes = eh.pack_code(s % 40, f // (23 * 11), (f // 11) % 23, f % 11, s // 40).reshape(1, N, K)
    rad = (1e4 * (e / (n - 1)) ** 2).astype(np.float32).reshape(1, N, K)
    return make_inputs(layer, 1, N, K, 0, seed=seed, codes=codes, rad=rad)


@pytest.mark.parametrize("f16,aw16", [(0, 1), (1, 1), (1, 0)], ids=["bf16_A16", "f16_A16", "f16_A32"])
def test_every_reachable_code(h, layer, f16, aw16):
    inp = every_code_inputs(layer, 5)
    r = run(h, msg_launch(layer, inp, f16=f16, aw16=aw16, agg_zero=False))
    ref, bound, _, _ = ref_agg16(layer, inp, all_nodes(1, inp["N"]), f16, aw16)
    check(f"codes[{f16}{aw16}]", r["agg"].reshape(-1, H), ref, bound)


def test_every_reachable_code_f32(h, layer):
    inp = every_code_inputs(layer, 6)
    r = run(h, f32_launch(layer, inp))
    nodes = all_nodes(1, inp["N"])
    ab, i, j, code, rad = node_rows(inp, nodes)
    rr = eh.f32m_rows(layer, inp["A"][ab, i], inp["Bm"][ab, j], j, code, rad)
    ref, bound = eh.f32m_agg(rr["gm"], rr["e_gm"], inp["K"])
    check("f32m_codes", r["agg"].reshape(-1, H), ref, bound)


def rows_launch(h, layer, inp, rows, cnt, fp32):
    """launch_edge_rows (fp16) / launch_edge_rows32 over the list `rows` (capacity len(rows), device count cnt) -> [ceil32(cap)][256]."""
    cap = len(rows)
    cap32 = (cap + 31) // 32 * 32
    bufs = {"A": inp["A"] if fp32 else inp["A_s"], "Bm": inp["Bm"], "Bmb": dh.f2h(inp["Bm_s"]), "Ah": dh.f2h(inp["A_s"]),
            "rows": rows, "n_rows": np.array([cnt], np.uint32)}
    bufs.update(layer["slots"])
    bufs["rows_out"] = Out(np.float32 if fp32 else np.uint16, cap32 * H)
    Lc = {"op": "edge_rows32" if fp32 else "edge_rows", "bufs": bufs,
          "scalars": dict(B=1, N=inp["N"], R=0, K=1, f16=1, n_rows_cap=cap, ab_bstride=0, att_b=layer["att_b"])}
    return run(h, Lc)["rows_out"].reshape(cap32, H)


@pytest.mark.parametrize("fp32", [0, 1])
def test_every_reachable_code_row_by_row(h, layer, fp32):
    """The same sweep of every code through the row-list form, checked row by row: a code mapped to a wrong but similar table row
    (an adjacent bin) moves single rows, which a 60-row sum can hide."""
    inp = every_code_inputs(layer, 7)
    n = inp["N"] * inp["K"]
    rng = np.random.default_rng(8)
    i = rng.integers(0, inp["N"], n)
    j = rng.integers(0, inp["N"], n)
    code, rad = inp["codes"].ravel(), inp["rad"].ravel()
    rows = np.ascontiguousarray(np.stack([i.astype(np.uint32), j.astype(np.uint32), code, rad.view(np.uint32)], 1))
    out = rows_launch(h, layer, inp, rows, n, fp32)[:n]
    if fp32:
        rr = eh.f32m_rows(layer, inp["A"][0, i], inp["Bm"][0, j], j, code, rad)
        check("codes_rows32", out, rr["gm"], rr["e_gm"])
    else:
        rr = eh.edge_rows(layer, inp["A_s"][0, i], inp["Bm_s"][0, j], j, code, rad, f16=1, aw16=1)
        check("codes_rows16", dh.h_to_f64(out), rr["gm"], eh.store_bound(rr["gm"], rr["e_gm"], 1))


# ---- last layer: stored messages, coordinate update, ligand-only launches -------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("K", [60, 20, 1])
def test_last_layer(h, cus, layer, f16, K):
    """mbuf decoded against float64 S g m2 in its rounding, masked rows hold gate-0 zeros; full and ligand-only launches store bitwise the
    same mbuf and the ligand-only one leaves agg byte-for-byte sentinel, in node-task and tile-task form; k_edge_coord's fout against
    float64 on the stored messages (wc2 x 8: w clamps on both sides), bitwise the same from either buffer.  K <= 32: mbuf starts as NaN
    and fout stays finite - the coordinate kernel reads only the tiles that were written."""
    B, N, R = 3, 41, 16
    Lig = N - R
    inp = make_inputs(layer, B, N, K, R, seed=100 + K + f16)
    Lw = dict(layer, wc2=(layer["wc2"] * 8).astype(np.float32))
    Lw["slots"] = dict(layer["slots"], wc2=Lw["wc2"], wc2_s=(Lw["wc2"] / np.float32(S)).astype(np.float32))
    nan_fill = np.full(B * Lig * 64 * H, 0xffff, np.uint16)
    res = {}
    for lig_only in (0, 1):
        nodes = Lig if lig_only else N
        assert eh.task_form(B, nodes, K, cus) == ("tile" if h.tile_tasks(B, nodes, K) else "static") != "dynamic"
        Lc = msg_launch(Lw, inp, f16=f16, aw16=1 - f16, last=1, lig_only=lig_only, agg_zero=False, mbuf=nan_fill)
        res[lig_only] = run(h, Lc)
    assert np.array_equal(res[0]["mbuf"], res[1]["mbuf"])
    assert (res[1]["agg"].view(np.uint32) == 0xffffffff).all(), "ligand-only launch touched agg"
    ref_nodes = all_nodes(B, N, R)
    _, _, gm, egm = ref_agg16(Lw, inp, ref_nodes, f16, 1 - f16)
    msg = eh.decode_mbuf(res[0]["mbuf"], B, Lig)
    val = dh.h_to_f64(msg) if f16 else dh.bf16_to_f32(msg).astype(np.float64)
    ntile = (K + 31) // 32
    got = val[:, :, :K].reshape(-1, H)
    check(f"mbuf[f16={f16} K{K}]", got, gm, eh.store_bound(gm, egm, f16))
    masked = val[:, :, K:ntile * 32]
    assert (masked == 0).all(), "masked rows of a stored tile are not zero"
    # the segment sums against the launch's own stored messages (tight: catches a dropped, duplicated or extra row at any K)
    agg_l = res[0]["agg"].reshape(B, N, H)[:, R:].reshape(-1, H)
    check(f"agg_vs_mbuf[f16={f16} K{K}]", agg_l, got.reshape(-1, K, H).sum(1) / S, eh.agg_rows_bound(got, K, f16))
    if ntile == 1:
        assert (msg[:, :, 32:] == 0xffff).all(), "tile 1 written for K <= 32"
    fouts = []
    assert eh.coord_form(B, Lig, cus) == "static"
    for lig_only in (0, 1):
        Lc = {"op": "coord_bf16",
              "bufs": {**Lw["slots"], "edges": inp["edges"], "ca4": inp["ca4"], "mbuf": io(res[lig_only]["mbuf"]),
                       "fout": Out(np.float32, B * Lig * 3), "task_ctr": io(np.zeros(2 * eh.TASK_CTR_WGS, np.uint32))},
              "scalars": ints(inp, last=1, f16=f16, lig_only=lig_only)}
        rc = run(h, Lc)
        assert np.array_equal(rc["mbuf"], res[lig_only]["mbuf"]), "the coordinate kernel wrote its input"
        fouts.append(rc["fout"])
    assert np.array_equal(fouts[0].view(np.uint32), fouts[1].view(np.uint32))
    f = fouts[0].reshape(B, Lig, 3)
    assert np.isfinite(f).all()
    clamps = [0, 0]
    for b in range(B):
        for l in range(Lig):
            i = R + l
            xj = inp["ca4"][b, inp["edges"][b, i], :3]
            fr, bd, w = eh.coord_ref(Lw, val[b, l, :K], inp["ca4"][b, i, :3], xj, K, f16)
            clamps[0] += int((w < -2).sum()); clamps[1] += int((w > 2).sum())
            check(f"coord[f16={f16} K{K}]", f[b, l], fr, bd)
    if K == 60:
        assert clamps[0] > 0 and clamps[1] > 0, clamps


@pytest.mark.parametrize("f16", [0, 1])
def test_ligand_only_tile_tasks(h, cus, layer, f16):
    """Tile-task form of the last layer (K > 32, few ligand tasks): full and ligand-only store the same messages, the ligand-only
    launch neither stores, adds to nor zeroes agg (no memset: agg_is_zero = 0 and agg stays sentinel)."""
    B, N, R, K = 2, 33, 10, 47
    inp = make_inputs(layer, B, N, K, R, seed=7 + f16)
    assert h.tile_tasks(B, N - R, K) and h.tile_tasks(B, N, K)
    r0 = run(h, msg_launch(layer, inp, f16=f16, aw16=1, last=1, lig_only=0, agg_zero=False))
    r1 = run(h, msg_launch(layer, inp, f16=f16, aw16=1, last=1, lig_only=1, agg_zero=False))
    assert np.array_equal(r0["mbuf"], r1["mbuf"])
    assert (r1["agg"].view(np.uint32) == 0xffffffff).all()
    ref, bound, _, _ = ref_agg16(layer, inp, all_nodes(B, N), f16, 1)
    check(f"msg_last_tile[f16={f16}]", r0["agg"].reshape(-1, H), ref, bound)


def test_coord_task_forms(h, shim, cus, layer, tmp_path):
    """k_edge_coord in its dynamic form (B = 8, 2 x the device's waves in ligand tasks): fout against float64 on a sample of nodes,
    the counters zero after the launch, a second launch on the same counters bitwise the same, and the static form (a child with
    DFM_EDGE_DYNAMIC=0) bitwise the same."""
    B, R, K = 8, 5, 60
    Lig = 2 * cus
    N = R + Lig
    assert eh.coord_form(B, Lig, cus) == "dynamic"
    rng = np.random.default_rng(9)
    edges = rng.integers(0, N, (B, N, K)).astype(np.int32)
    ca4 = np.zeros((B, N, 4), np.float32)
    ca4[..., :3] = rng.standard_normal((B, N, 3)).astype(np.float32) * 8
    bits = (rng.standard_normal((B, Lig, 64, H), dtype=np.float32) * 0.2).astype(np.float16).view(np.uint16)
    bits[:, :, K:] = 0                                    # masked rows as the message kernel stores them
    inp = dict(B=B, N=N, R=R, K=K, Ab=1)

    def launch(repeat):
        return {"op": "coord_bf16",
                "bufs": {**layer["slots"], "edges": edges, "ca4": ca4, "mbuf": io(eh.encode_mbuf(bits)), "fout": Out(np.float32, B * Lig * 3),
                         "task_ctr": io(np.zeros(2 * eh.TASK_CTR_WGS, np.uint32))},
                "scalars": ints(inp, last=1, f16=1, repeat=repeat)}

    r1 = run(h, launch(1))
    r2 = run(h, launch(2))
    assert np.array_equal(r1["fout"].view(np.uint32), r2["fout"].view(np.uint32)), "second launch on the same counters differs"
    f = r1["fout"].reshape(B, Lig, 3)
    for b, l in zip(rng.integers(0, B, 48), rng.integers(0, Lig, 48)):
        i = R + l
        vals = bits[b, l, :K].view(np.float16).astype(np.float64)
        fr, bd, _ = eh.coord_ref(layer, vals, ca4[b, i, :3], ca4[b, edges[b, i], :3], K, 1)
        check("coord_dynamic", f[b, l], fr, bd)
    fin, fout = str(tmp_path / "coord_in.npz"), str(tmp_path / "coord_out.npz")
    eh.save_launches(fin, [launch(1)])
    p = subprocess.run([sys.executable, eh.__file__, "child", shim, fin, fout], env={**os.environ, "DFM_EDGE_DYNAMIC": "0"},
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    o = np.load(fout)
    assert bool(o["0/fout_guard_ok"]) and not o["0/task_ctr"].any()
    assert np.array_equal(o["0/fout"].view(np.uint32), r1["fout"].view(np.uint32)), "static coordinate form differs"


@pytest.mark.parametrize("aw16", [0, 1])
def test_fp16_operand_saturation(h, layer, aw16):
    """Edges whose pre-activation lies far beyond fp16 range (radial 1e9 A^2: |w_r r^2| ~ 1e6): the fp16 operand saturates at
    +-65504 (v_cvt_pkrtz truncates), the contraction (edge_mlp.2 x 4) carries messages below -65504, and their fp16 store saturates
    at -65504 (pack_f16_sat_lo): every output finite, none -inf, and agg and the stored messages within the bound of a reference that
    models both clamps."""
    L4 = eh.make_layer(seed=0, scale=4.0)
    B, N, R, K = 1, 23, 5, 40
    inp = make_inputs(L4, B, N, K, R, seed=61)
    hot = [(R + l, (3 * l) % K) for l in range(0, N - R, 2)]
    for i, s_ in hot:
        inp["rad"][0, i, s_] = 1e9
    r = run(h, msg_launch(L4, inp, f16=1, aw16=aw16, last=1, agg_zero=False))
    ref, bound, gm, egm = ref_agg16(L4, inp, all_nodes(B, N), 1, aw16)
    assert np.isfinite(r["agg"]).all()
    check(f"saturation_agg[{aw16}]", r["agg"].reshape(-1, H), ref, bound)
    msg = eh.decode_mbuf(r["mbuf"], B, N - R)
    assert not (msg[:, :, :K] == 0xfc00).any() and np.isfinite(dh.h_to_f64(msg[:, :, :K])).all()
    gm_l = gm.reshape(B, N, K, H)[:, R:].reshape(-1, H)
    egm_l = egm.reshape(B, N, K, H)[:, R:].reshape(-1, H)
    assert (gm_l < -65504).any(), "no stored message below the fp16 range: the store clamp is not exercised"
    check(f"saturation_mbuf[{aw16}]", dh.h_to_f64(msg[:, :, :K]).reshape(-1, H), np.maximum(gm_l, -65504.0),
          eh.store_bound(gm_l, egm_l, 1))
    assert (msg[:, :, :K] == 0xfbff).any()


def test_realistic_fixture_inputs(h, layer):
    """The committed fwd_syn_64_48_p0 case: its kNN edges, bins and relpos mapped to codes, h_first as node features and radial values
    from its geometry (make_complex(R, L, cx_seed) with the fixture's ligand pose), through all four 16-bit instantiations (agg and the
    stored messages of the last layer) and the fp32 kernel."""
    from dfmdock_amd.synthetic import make_complex
    d = np.load(os.path.join(eh.ROOT, "tests", "golden", "fwd_syn_64_48_p0.npz"))
    R, Lg = int(d["R"]), int(d["L"])
    N = R + Lg
    edges = d["edges"].astype(np.int32)
    K = edges.shape[1]
    cx = make_complex(R, Lg, int(d["cx_seed"]))
    ca = np.concatenate([cx["rec_pos"][:, 1], d["lig_pos"][:, 1]]).astype(np.float32)
    dx = ca[:, None, :] - ca[edges]
    rad = ((dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + dx[..., 2] * dx[..., 2]).astype(np.float32)
    b = d["bins"].astype(np.int64)
    codes = eh.pack_code(b[..., 0], b[..., 1], b[..., 2], b[..., 3], d["relpos"].astype(np.int64))
    A, Bm, A_s, Bm_s = eh.node_operands(layer, d["h_first"][None])
    ca4 = np.zeros((1, N, 4), np.float32)
    ca4[0, :, :3] = ca
    inp = dict(B=1, N=N, K=K, R=R, Ab=1, A=A, Bm=Bm, A_s=A_s, Bm_s=Bm_s, edges=edges[None], codes=codes[None].astype(np.uint32),
               rad=rad[None], ca4=ca4)
    nodes = all_nodes(1, N)
    for f16, aw16 in FORMS16:
        r = run(h, msg_launch(layer, inp, f16=f16, aw16=aw16, last=1, agg_zero=False))
        ref, bound, gm, egm = ref_agg16(layer, inp, nodes, f16, aw16)
        check(f"fixture_msg[{f16}{aw16}]", r["agg"].reshape(-1, H), ref, bound)
        msg = eh.decode_mbuf(r["mbuf"], 1, Lg)
        val = dh.h_to_f64(msg) if f16 else dh.bf16_to_f32(msg).astype(np.float64)
        gm_l = gm.reshape(N, K, H)[R:].reshape(-1, H)
        egm_l = egm.reshape(N, K, H)[R:].reshape(-1, H)
        check(f"fixture_mbuf[{f16}{aw16}]", val[0, :, :K].reshape(-1, H), gm_l, eh.store_bound(gm_l, egm_l, f16))
    r = run(h, f32_launch(layer, inp))
    ab, i, j, code, rd = node_rows(inp, nodes)
    rr = eh.f32m_rows(layer, A[ab, i], Bm[ab, j], j, code, rd)
    ref, bound = eh.f32m_agg(rr["gm"], rr["e_gm"], K)
    check("fixture_f32m", r["agg"].reshape(-1, H), ref, bound)


# ---- k_edge_f32m ------------------------------------------------------------------------------------------------------------
def test_f32m_matches_float64(h, layer):
    """Its tight bound, an odd number of node tasks (the last workgroup's second node is absent), range against the float64 maxima,
    and the last layer with and without lig_only: fout bitwise equal, and the ligand-only launch leaves agg byte-for-byte sentinel."""
    B, N, R, K = 3, 37, 12, 60
    inp = make_inputs(layer, B, N, K, R, seed=21)
    r = run(h, f32_launch(layer, inp, last=1))
    nodes = all_nodes(B, N)
    ab, i, j, code, rad = node_rows(inp, nodes)
    rr = eh.f32m_rows(layer, inp["A"][ab, i], inp["Bm"][ab, j], j, code, rad)
    ref, bound = eh.f32m_agg(rr["gm"], rr["e_gm"], K)
    check("f32m", r["agg"].reshape(-1, H), ref, bound)
    rng_ = r["range"].view(np.float32)
    k = np.argmax(np.abs(rr["pre"]))
    assert abs(rng_[0] - np.abs(rr["pre"]).max()) <= rr["e_pre"].ravel()[k] + 1e-30
    kx = np.argmax(np.abs(rr["x"]))
    assert abs(rng_[1] - np.abs(rr["x"]).max()) <= rr["e_x"].ravel()[kx] + 1e-30
    r1 = run(h, f32_launch(layer, inp, last=1, lig_only=1))
    assert np.array_equal(r["fout"].view(np.uint32), r1["fout"].view(np.uint32))
    assert (r1["agg"].view(np.uint32) == 0xffffffff).all(), "ligand-only fp32 launch touched agg"
    Lig = N - R
    f = r["fout"].reshape(B, Lig, 3)
    gm = rr["gm"].reshape(B, N, K, H)
    egm = rr["e_gm"].reshape(B, N, K, H)
    for b in range(B):
        for l in range(Lig):
            i0 = R + l
            xj = inp["ca4"][b, inp["edges"][b, i0], :3]
            fr, bd, _ = eh.f32m_coord(layer, gm[b, i0], egm[b, i0], inp["ca4"][b, i0, :3], xj, K)
            check("f32m_coord", f[b, l], fr, bd)


# ---- row-list form and the layer-0 gather ----------------------------------------------------------------------------------
def row_list(inp, n, seed):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, inp["N"], n)
    j = rng.integers(0, inp["N"], n)
    code = random_codes(rng, n)
    rad = rng.uniform(0, 400, n).astype(np.float32)
    rows = np.stack([i.astype(np.uint32), j.astype(np.uint32), code, rad.view(np.uint32)], 1)
    return np.ascontiguousarray(rows)


@pytest.mark.parametrize("fp32", [0, 1])
def test_edge_rows(h, layer, fp32):
    """launch_edge_rows / launch_edge_rows32 against float64: capacity 203 (not a multiple of 32), device count 150 - rows past
    ceil32(150) keep their sentinel (fp32: rows past 150) - and a permuted list gives bitwise the same row values."""
    inp = make_inputs(layer, 1, 50, 1, 0, seed=31, per_traj=False)
    cap, cnt = 203, 150
    rows = row_list(inp, cap, 32)
    cap32 = (cap + 31) // 32 * 32

    def launch(rw):
        bufs = {"A": inp["A"] if fp32 else inp["A_s"], "Bm": inp["Bm"], "Bmb": dh.f2h(inp["Bm_s"]), "Ah": dh.f2h(inp["A_s"]),
                "rows": rw, "n_rows": np.array([cnt], np.uint32)}
        bufs.update(layer["slots"])
        bufs["rows_out"] = Out(np.float32 if fp32 else np.uint16, cap32 * H)
        Lc = {"op": "edge_rows32" if fp32 else "edge_rows", "bufs": bufs,
              "scalars": dict(B=1, N=inp["N"], R=0, K=1, f16=1, n_rows_cap=cap, ab_bstride=0, att_b=layer["att_b"])}
        return run(h, Lc)["rows_out"].reshape(cap32, H)

    out = launch(rows)
    i, j, code, rad = rows[:cnt, 0], rows[:cnt, 1], rows[:cnt, 2], rows[:cnt, 3].view(np.float32)
    if fp32:
        rr = eh.f32m_rows(layer, inp["A"][0, i], inp["Bm"][0, j], j, code, rad)
        check("rows32", out[:cnt], rr["gm"], rr["e_gm"])
        assert (out[cnt:].view(np.uint32) == 0xffffffff).all()
    else:
        rr = eh.edge_rows(layer, inp["A_s"][0, i], inp["Bm_s"][0, j], j, code, rad, f16=1, aw16=1)
        check("rows16", dh.h_to_f64(out[:cnt]), rr["gm"], eh.store_bound(rr["gm"], rr["e_gm"], 1))
        c32 = (cnt + 31) // 32 * 32
        assert (dh.h_to_f64(out[cnt:c32]) == 0).all(), "rows past the count inside the last tile are not zero"
        assert (out[c32:] == 0xffff).all(), "rows past ceil32(count) were written"
    perm = np.random.default_rng(4).permutation(cnt)
    rows_p = rows.copy()
    rows_p[:cnt] = rows[perm]
    out_p = launch(rows_p)
    assert np.array_equal(out_p[:cnt], out[perm])


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("K", [1, 12, 13, 59, 60])
def test_l0_gather(h, fp32, K):
    """k_l0_gather / k_l0_gather32: table hits and MISS-flagged rows against the float64 sum, bitwise batch invariance (B = 1 against
    trajectory 0 of B = 3), counter reset to 0 and miss_total += counter."""
    rng = np.random.default_rng(K + 10 * fp32)
    N, P, M = 23, 97, 41
    tab = (rng.standard_normal((P, H)) * 0.3).astype(np.float32)
    X = (rng.standard_normal((M, H)) * 0.3).astype(np.float32)
    if not fp32:
        tab, X = dh.f2h(tab), dh.f2h(X)
    tv = dh.h_to_f64(tab) if not fp32 else tab.astype(np.float64)
    xv = dh.h_to_f64(X) if not fp32 else X.astype(np.float64)

    def launch(B, src):
        Lc = {"op": "l0_gather32" if fp32 else "l0_gather",
              "bufs": {"table": tab, "X": X, "src": src, "agg": Out(np.float32, B * N * H), "counter": io(np.array([7], np.uint32)),
                       "miss_total": io(np.array([100], np.uint64))},
              "scalars": dict(B=B, N=N, K=K)}
        r = run(h, Lc)
        assert r["counter"][0] == 0 and r["miss_total"][0] == 107
        return r["agg"].reshape(B, N, H)

    B = 3
    miss = rng.random((B, N, K)) < 0.3
    src = np.where(miss, eh.L0_MISS | rng.integers(0, M, (B, N, K)), rng.integers(0, P, (B, N, K))).astype(np.uint32)
    agg = launch(B, src)
    vals = np.where(miss[..., None], xv[np.where(miss, src & 0x7fffffff, 0)], tv[np.where(miss, 0, src)])
    scale = 1.0 if fp32 else 1.0 / S
    ref = vals.sum(2) * scale
    bound = ((K // 2 + 2) if not fp32 else (K + 1)) * eh.U * np.abs(vals).sum(2) * abs(scale) + eh.U * np.abs(ref) + 1e-30
    check(f"gather[{'f32' if fp32 else 'f16'} K{K}]", agg, ref, bound)
    agg1 = launch(1, np.ascontiguousarray(src[:1]))
    assert np.array_equal(agg1[0].view(np.uint32), agg[0].view(np.uint32))


@pytest.mark.parametrize("fp32", [0, 1])
def test_l0_gather_non_finite_rows(h, fp32):
    """Rows of the row list whose message is NaN (the rows of edges with a NaN radial: a non-finite pose): exactly the nodes that own
    such a row become NaN, every other node - of the same and of the other trajectories - keeps its bits, the counter ends at zero."""
    rng = np.random.default_rng(77 + fp32)
    B, N, K, P, M = 3, 23, 13, 97, 41
    tab = (rng.standard_normal((P, H)) * 0.3).astype(np.float32)
    X = (rng.standard_normal((M, H)) * 0.3).astype(np.float32)
    Xn = X.copy()
    nanrows = np.array([0, 7, 40])
    Xn[nanrows] = np.nan
    Xn[19, 100] = np.nan      # one channel only
    nanrows = np.append(nanrows, 19)
    if not fp32:
        tab, X, Xn = dh.f2h(tab), dh.f2h(X), dh.f2h(Xn)
    miss = rng.random((B, N, K)) < 0.3
    src = np.where(miss, eh.L0_MISS | rng.integers(0, M, (B, N, K)), rng.integers(0, P, (B, N, K))).astype(np.uint32)

    def launch(x):
        r = run(h, {"op": "l0_gather32" if fp32 else "l0_gather",
                    "bufs": {"table": tab, "X": x, "src": src, "agg": Out(np.float32, B * N * H), "counter": io(np.array([7], np.uint32)),
                             "miss_total": io(np.array([100], np.uint64))}, "scalars": dict(B=B, N=N, K=K)})
        assert r["counter"][0] == 0 and r["miss_total"][0] == 107
        return r["agg"].reshape(B, N, H)

    good, bad = launch(X), launch(Xn)
    owns = (miss & np.isin(src & 0x7fffffff, nanrows)).any(2)
    assert owns.any() and (~owns).any() and np.isfinite(good).all()
    assert np.isnan(bad[owns]).any(-1).all() and np.array_equal(bad[~owns].view(np.uint32), good[~owns].view(np.uint32))
    full = (miss & np.isin(src & 0x7fffffff, nanrows[:3])).any(2)
    assert np.isnan(bad[full]).all()


# ---- special values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["bf16_A32", "bf16_A16", "f16_A32", "f16_A16", "f32"])
def test_nan_reaches_every_output(h, layer, kernel):
    """A NaN in one ligand node's A row reaches that node's agg, its stored messages (the fp16 form: pack_f16_sat_lo) and its fout (the
    coordinate clamp) as NaN; every other node stays finite."""
    B, N, R, K = 2, 29, 9, 40
    inp = make_inputs(layer, B, N, K, R, seed=55)
    i0 = R + 3
    Lig = N - R
    if kernel == "f32":
        A = inp["A"].copy()
        A[1, i0, 17] = np.nan
        r = run(h, f32_launch(layer, inp, last=1, A=A))
        fout = r["fout"].reshape(B, Lig, 3)
    else:
        f16, aw16 = int(kernel.startswith("f16")), int(kernel.endswith("A16"))
        A_s = inp["A_s"].copy()
        A_s[1, i0, 17] = np.nan
        r = run(h, msg_launch(layer, inp, f16=f16, aw16=aw16, last=1, agg_zero=False, A_s=A_s))
        msg = eh.decode_mbuf(r["mbuf"], B, Lig)
        val = dh.h_to_f64(msg) if f16 else dh.bf16_to_f32(msg).astype(np.float64)
        assert np.isnan(val[1, i0 - R, :K]).all(), "NaN lost in the stored messages"
        mask = np.ones(val.shape[:2], bool)
        mask[1, i0 - R] = False
        assert np.isfinite(val[mask][:, :K]).all()
        Lc = {"op": "coord_bf16", "bufs": {**layer["slots"], "edges": inp["edges"], "ca4": inp["ca4"], "mbuf": io(r["mbuf"]),
                                           "fout": Out(np.float32, B * Lig * 3)}, "scalars": ints(inp, last=1, f16=f16)}
        fout = run(h, Lc)["fout"].reshape(B, Lig, 3)
    agg = r["agg"].reshape(B, N, H)
    assert np.isnan(agg[1, i0]).all(), "NaN lost in agg"
    ok = np.ones((B, N), bool)
    ok[1, i0] = False
    assert np.isfinite(agg[ok]).all()
    assert np.isnan(fout[1, i0 - R]).all(), "NaN lost in the coordinate update"
    fo = np.ones((B, Lig), bool)
    fo[1, i0 - R] = False
    assert np.isfinite(fout[fo]).all()


def test_nan_reaches_row_outputs(h, layer):
    inp = make_inputs(layer, 1, 30, 1, 0, seed=77, per_traj=False)
    rows = row_list(inp, 64, 78)
    A_s = inp["A_s"].copy()
    i0 = int(rows[5, 0])
    A_s[0, i0, 3] = np.nan
    for fp32 in (0, 1):
        A = inp["A"].copy()
        A[0, i0, 3] = np.nan
        bufs = {"A": A if fp32 else A_s, "Bm": inp["Bm"], "Bmb": dh.f2h(inp["Bm_s"]), "Ah": dh.f2h(A_s), "rows": rows}
        bufs.update(layer["slots"])
        bufs["rows_out"] = Out(np.float32 if fp32 else np.uint16, 64 * H)
        Lc = {"op": "edge_rows32" if fp32 else "edge_rows", "bufs": bufs,
              "scalars": dict(B=1, N=inp["N"], R=0, K=1, f16=1, n_rows_cap=64, ab_bstride=0, att_b=layer["att_b"])}
        out = run(h, Lc)["rows_out"].reshape(64, H)
        v = out.astype(np.float64) if fp32 else dh.h_to_f64(out)
        hit = rows[:, 0] == i0
        assert np.isnan(v[hit]).all() and np.isfinite(v[~hit]).all()
