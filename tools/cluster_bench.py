"""Timing of pose clustering (dfm_pose_cluster) on one GPU: prints ONE JSON line.

    python tools/cluster_bench.py [--L 300] [--sizes 1024,4096,16384,65536] [--reps 3] [--numpy-full]

Per B and rule: the wall time of the call (host to host: upload, kernels, download) and the GPU times of k_pose_dist and of the clustering
kernels after it (device events inside the call, dfm_pose_last_timing), medians over --reps after one warm-up call.  The float64 numpy
definition (cluster.pose_rmsd + cluster_adjacency) is timed at B = 1024 in full; at B = 4096 it is timed on 256 rows of the distance matrix
and scaled to B rows (`numpy_f64_extrapolated`) unless --numpy-full.

Roofline of k_pose_dist: B (B + 1) / 2 pairs x 9 n_res coordinates, each term one v_sub_f32 + one v_fma_f32 (non-packed), so the VALU bound is
256 CUs x 128 lanes x sclk / 2 terms per second (the 157.3 TFLOP/s fp32 vector peak at 2400 MHz counts one FMA as two FLOP).  sclk is read
(read-only) from rocm-smi while the largest size runs; when it cannot be read, the fraction is quoted at 2400 MHz and says so.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUS, LANES_PER_CU, PEAK_SCLK_MHZ = 256, 128, 2400.0


def poses(B, L, seed=0):
    """B poses of one ligand backbone spread over 64 basins (rigid translations plus 1.5 A of per-pose shift)."""
    rng = np.random.default_rng(seed)
    base = rng.normal(0, 8, (L, 9)).astype(np.float32)
    centres = rng.normal(0, 15, (64, 3)).astype(np.float32)
    shift = centres[rng.integers(0, 64, B)] + rng.normal(0, 1.5, (B, 3)).astype(np.float32)
    return base[None] + np.tile(shift, 3)[:, None, :]


def read_sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        d = json.loads(out)
        card = d.get("card0") or next(iter(d.values()))
        for k, v in card.items():
            if "sclk" in k.lower():
                return float(str(v).strip("()").lower().replace("mhz", ""))
    except Exception:
        return None
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=300)
    ap.add_argument("--sizes", default="1024,4096,16384,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--numpy-full", action="store_true")
    a = ap.parse_args()
    from dfmdock_amd import cluster, engine
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    sizes = [int(s) for s in a.sizes.split(",")]
    out = {"tool": "cluster_bench", "L": a.L, "radius": a.radius, "reps": a.reps, "runs": []}
    clocks, stop = [], threading.Event()
    for B in sizes:
        x = poses(B, a.L, seed=B)
        key = np.random.default_rng(B).normal(size=B).astype(np.float32)
        poller = None
        if B == max(sizes):
            def poll():
                while not stop.is_set():
                    c = read_sclk()
                    if c:
                        clocks.append(c)
                    stop.wait(0.5)
            poller = threading.Thread(target=poll, daemon=True)
            poller.start()
        for rule in ("energy", "size"):
            model.pose_cluster(x, a.radius, key=key, rule=rule, max_clusters=10)      # warm-up
            wall, dist, clus = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = model.pose_cluster(x, a.radius, key=key, rule=rule, max_clusters=10)
                wall.append((time.perf_counter() - t0) * 1e3)
                d, c = engine.pose_last_timing()
                dist.append(d)
                clus.append(c)
            terms = B * (B + 1) / 2 * 9 * a.L
            kd = float(np.median(dist))
            out["runs"].append({"B": B, "rule": rule, "wall_ms": float(np.median(wall)), "k_pose_dist_ms": kd,
                                "cluster_kernels_ms": float(np.median(clus)), "n_clusters": r["n_clusters"],
                                "largest_cluster": int(r["size"].max()), "pair_terms": terms, "pair_terms_per_s": terms / (kd / 1e3)})
        if poller is not None:
            stop.set()
            poller.join()
        del x
    sclk = float(np.median(clocks)) if clocks else None
    at = sclk or PEAK_SCLK_MHZ
    peak_terms = CUS * LANES_PER_CU * at * 1e6 / 2
    for r in out["runs"]:
        r["frac_of_valu_peak"] = r["pair_terms_per_s"] / peak_terms
    out["valu_peak_terms_per_s"] = peak_terms
    out["sclk_mhz"] = sclk
    out["sclk_note"] = ("median shader clock read from rocm-smi during the largest size" if sclk else
                        "shader clock not readable here: the fraction is quoted at 2400 MHz")
    # the float64 numpy definition
    npt = {}
    for B in (1024, 4096):
        x = poses(B, a.L, seed=B)
        key = np.random.default_rng(B).normal(size=B).astype(np.float32)
        if B == 1024 or a.numpy_full:
            t0 = time.perf_counter()
            cluster.cluster_adjacency(cluster.pose_rmsd(x) <= a.radius, key, "energy", 10)
            npt[str(B)] = {"ms": (time.perf_counter() - t0) * 1e3, "extrapolated": False}
        else:
            rows = 256
            xx = x.reshape(B, -1, 3).astype(np.float64)
            t0 = time.perf_counter()
            for i in range(rows):
                np.sqrt(((xx - xx[i]) ** 2).sum(-1).sum(-1) / xx.shape[1])
            npt[str(B)] = {"ms": (time.perf_counter() - t0) * 1e3 * B / rows, "extrapolated": True, "rows_timed": rows}
    out["numpy_f64"] = npt
    model.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
