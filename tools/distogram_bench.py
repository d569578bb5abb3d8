"""The distogram head reduced on the GPU (Complex.distogram, dfm_score_distogram: k_pair_dist_sum) against the only other way to the
same numbers: `score(dist=True)` (k_pair_dist, the [B,R,L,64] logits copied to the host) followed by the float64 numpy reductions of
dfmdock_amd/distogram.py.  Writes profiles/distogram.txt.

    python tools/distogram_bench.py [--out profiles/distogram.txt] [--reps 5]

Complex: the synthetic 300 + 300 residue complex of the headline benchmark (synthetic.make_complex(300, 300, seed=1)), second model
family with the seeded weights, poses = the input pose translated by N(0, 3^2) A per axis, t = 1e-3, fp32 and mfma16 engines.

Both ways at B = 1 and B = 8 (184 MB of logits - what the logits path can hold), the new call alone at B = 256.  2 warm-up calls, then
`reps` timed calls each; wall time from a host clock; GPU time between the uploads and the downloads from the calls' own events:
dfm_distogram_last_timing (copy_ms, kernel_ms) for the new call, dfm_profile.total_ms (DFM_F_PROFILE) for score().  Both spans hold
the whole forward, so the same evaluation without any distogram work (`score(dist=False)`) is timed too and subtracted: what is left is
the head alone (projection GEMM + pair kernel + finish).  The host reductions of the logits path are timed apart.

Before any time is printed the two ways are compared at B = 1 on every engine, over the seven committed fixtures of
tests/test_gpu_distogram.py: the largest deviation of each output is what that file's gates (four times it) are made of."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ["fwd2_syn_9_7", "fwd2_syn_24_16", "fwd2_syn_64_48_p0", "fwd2_syn_64_48_p1", "fwd2_syn_64_48_p2", "fwd2_7CEI_p0", "fwd2_7CEI_p1"]
ENGINES = {"fp32": {}, "mfma16": dict(mfma16=True), "f16": dict(f16=True)}
MAPS = ("pair_nll", "pcontact", "edist")


def deviations(model, hp):
    """Largest deviation of every output of the new call from the definition applied to the same call's logits, over the fixtures."""
    from conftest import complex_for, load_golden
    from dfmdock_amd import distogram as DG
    from dfmdock_amd import engine
    worst, where, cxs = {}, {}, {}
    for case in CASES:
        key = next(k for k in ("7CEI", "syn_24_16", "syn_9_7", "syn_64_48") if k in case)
        if key not in cxs:
            cx = complex_for(case)
            cxs[key] = (engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"]), cx)
        gx, cx = cxs[key]
        g = load_golden(case + ".npz")
        D = DG.ca_distances(cx["rec_pos"], g["lig_pos"])
        keep = np.abs((D ** 2)[..., None] / DG.BOUNDS ** 2 - 1).min(-1) > 1e-5
        for prec, kw in ENGINES.items():
            d = gx.distogram(g["lig_pos"], float(g["t"]), edges=g["edges"], maps=MAPS, **kw)
            z = gx.score(g["lig_pos"], float(g["t"]), edges=g["edges"], dist=True, **kw)["dist_logits"][0]
            e = DG.pose_scores(z, D, 7, hp.cut_off)
            dev = {"pair_nll": np.abs(d["pair_nll"][0] - e["pair_nll"])[keep].max(), "nll": abs(float(d["nll"][0]) - e["nll"]),
                   "nll_near": abs(float(d["nll_near"][0]) - e["nll_near"]) if e["n_near"] == int(d["n_near"][0]) else np.nan,
                   "pcontact (relative)": (np.abs(d["pcontact"][0] - e["pcontact"]) / e["pcontact"]).max(),
                   "edist (A)": np.abs(d["edist"][0] - e["edist"]).max(),
                   "exp_contacts (relative)": abs(float(d["exp_contacts"][0]) - e["exp_contacts"]) / e["exp_contacts"]}
            for k, v in dev.items():
                if k not in worst or v > worst[k]:
                    worst[k], where[k] = float(v), f"{case} {prec}"
    for gx, _ in cxs.values():
        gx.close()
    return worst, where


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distogram.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=256, help="batch of the new call alone")
    a = ap.parse_args()
    from dfmdock_amd import _lib as L
    from dfmdock_amd import distogram as DG
    from dfmdock_amd import engine
    from dfmdock_amd.synthetic import make_complex
    from dfmdock_amd.weights import HParams, make_random_weights, pack_blob
    import ctypes as C
    hp = HParams(family=1, mask_dist=20.0)
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0, hp), hp), hp)
    lines = ["distogram head: reduced in the pair kernel (dfm_score_distogram) vs logits to the host + numpy (score(dist=True), distogram.pose_scores)",
             engine.config_string()]
    worst, where = deviations(model, hp)
    lines.append("largest deviation from the definition applied to the same call's logits, 7 fixtures x 3 engines (tests/test_gpu_distogram.py gates at 4 x):")
    lines += [f"  {k:24s} {v:.3e}   ({where[k]})" for k, v in worst.items()]
    med = lambda v: float(np.median(v))

    def last_timing():
        c, k = C.c_double(), C.c_double()
        L.check(L.lib().dfm_distogram_last_timing(C.byref(c), C.byref(k)), "dfm_distogram_last_timing")
        return c.value, k.value

    R = Lg = 300
    cx = make_complex(R, Lg, seed=1)
    gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    rng = np.random.default_rng(7)
    for prec in ("fp32", "mfma16"):
        kw = ENGINES[prec]
        for B in (1, 8, a.big):
            poses = cx["lig_pos"][None] + (3.0 * rng.standard_normal((B, 1, 1, 3))).astype(np.float32)
            t = np.full(B, 1e-3, np.float32)
            ed = gx.score(poses, t, seed=5, energy=False, return_edges=True, **kw)["edges"]      # one graph draw for every way
            row = {}
            for name, fn in (("new", lambda: gx.distogram(poses, t, edges=ed, **kw)),
                             ("new+maps", lambda: gx.distogram(poses, t, edges=ed, maps=("pcontact", "edist", "pcontact_mean"), **kw)),
                             ("forward", lambda: gx.score(poses, t, edges=ed, energy=False, profile=True, **kw)),
                             ("logits", lambda: gx.score(poses, t, edges=ed, energy=False, profile=True, dist=True, **kw))):
                if B > 8 and name == "logits":
                    continue
                for _ in range(2):
                    fn()
                wall, gpu, cp = [], [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    o = fn()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    if name.startswith("new"):
                        c, k = last_timing()
                        cp.append(c)
                        gpu.append(k)
                    else:
                        gpu.append(gx.profile()["total_ms"])
                row[name] = (med(wall), med(gpu), med(cp) if cp else float("nan"), o)
            lines.append(f"300 + 300 residues, {prec}, B = {B}  (logits: {B * R * Lg * 64 * 4 / 1e6:.0f} MB; per-pose outputs: {B * 16} bytes)")
            fwd = row["forward"][1]
            lines.append(f"  forward alone (score, no distogram)      wall {row['forward'][0]:9.2f} ms   GPU {fwd:9.3f} ms")
            for name in ("new", "new+maps"):
                w, k, c, _ = row[name]
                lines.append(f"  {'dfm_score_distogram' + (' + 3 maps' if name != 'new' else ''):40s} wall {w:9.2f} ms   GPU {k:9.3f} ms (head alone {k - fwd:8.3f} ms)   copies {c:8.3f} ms")
            if "logits" in row:
                w, k, _, o = row["logits"]
                D = DG.ca_distances(cx["rec_pos"], poses)
                t0 = time.perf_counter()
                ref = [DG.pose_scores(o["dist_logits"][b], D[b], 7, hp.cut_off) for b in range(B)]
                host = (time.perf_counter() - t0) * 1e3
                got = row["new"][3]
                dn = max(abs(float(got["nll"][b]) - ref[b]["nll"]) for b in range(B))
                lines.append(f"  {'score(dist=True): k_pair_dist + logits':40s} wall {w:9.2f} ms   GPU {k:9.3f} ms (head alone {k - fwd:8.3f} ms)   + numpy reductions {host:8.1f} ms")
                lines.append(f"  -> wall {(w + host) / row['new'][0]:.1f} x, head kernels {(k - fwd) / max(row['new'][1] - fwd, 1e-9):.2f} x in favour of the new call; largest |nll - definition| {dn:.2e}")
    gx.close()
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
