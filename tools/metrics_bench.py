"""Poses per second of the batched GPU docking metrics (dfm_pose_metrics) against the host loop (metrics.compute_metrics with a
NativeContext: one core, and 16 worker processes over the poses) on the same poses, at (R, L, P) = (300, 300, 10 240) - the trace of
one 256-trajectory, 40-step batch - and at one DB5 size.  Writes profiles/metrics.txt.

    python tools/metrics_bench.py [--out profiles/metrics.txt] [--reps 7] [--host-poses 2048]

GPU: warm-up calls, then `reps` timed calls; wall time of the whole call (upload, kernels, download, host finish) from a host clock,
copy and kernel time from the call's own HIP events (dfm_metrics_last_timing); median and min-max.  Roofline of the kernels: the poses
are read twice (sums, then residuals), 2 x 36 L bytes per pose with a fixed receptor, over the measured HBM copy rate 6.29 TB/s."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 6.29e12

_ctx = {}


def _host_chunk(args):
    from dfmdock_amd.metrics import compute_metrics
    lo, hi = args
    rec, lig, poses, ctx = _ctx["v"]
    return [compute_metrics((rec, poses[k]), (rec, lig), ctx)["DockQ"] for k in range(lo, hi)]


def host_rates(rec, lig, poses, workers=16):
    """(poses/s on one core, poses/s with `workers` forked processes over the poses)."""
    import multiprocessing as mp
    from dfmdock_amd.metrics import NativeContext
    _ctx["v"] = (rec, lig, poses, NativeContext((rec, lig)))
    n = len(poses)
    t0 = time.perf_counter()
    one = _host_chunk((0, max(1, n // 8)))
    t_one = (time.perf_counter() - t0) / len(one)
    cuts = np.linspace(0, n, workers + 1).astype(int)
    with mp.get_context("fork").Pool(workers) as pool:      # forked BEFORE this process touches the GPU
        pool.map(_host_chunk, [(0, 1)] * workers)      # start-up outside the timed window
        t0 = time.perf_counter()
        pool.map(_host_chunk, list(zip(cuts[:-1], cuts[1:])))
        t_many = (time.perf_counter() - t0) / n
    return 1.0 / t_one, 1.0 / t_many


def make_case(R, L, P, seed):
    from dfmdock_amd.synthetic import make_complex
    cx = make_complex(R, L, seed=seed)
    rng = np.random.default_rng(seed)
    lig = np.asarray(cx["lig_pos"], np.float32)
    poses = np.empty((P,) + lig.shape, np.float32)
    poses[:] = lig[None]
    poses += (rng.standard_normal((P, 1, 1, 3)) * np.linspace(0, 10, P)[:, None, None, None]).astype(np.float32)
    return np.asarray(cx["rec_pos"], np.float32), lig, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=2048, help="poses the host loops are timed on (their rate does not depend on P)")
    a = ap.parse_args()
    cases = [("C3 trace", 300, 300, 10240, 1), ("DB5 size (1AVX-like)", 223, 177, 10240, 2)]
    data = [(name, R, L, P) + make_case(R, L, P, seed) for name, R, L, P, seed in cases]
    host = [host_rates(rec, lig, poses[: a.host_poses]) for _, _, _, _, rec, lig, poses in data]      # before the GPU is opened
    from dfmdock_amd import engine
    from dfmdock_amd.metrics import NativeContext, compute_metrics
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["docking metrics: GPU call (dfm_pose_metrics) vs host loop (metrics.compute_metrics + NativeContext)", engine.config_string()]
    ok = True
    for (name, R, L, P, rec, lig, poses), (h1, h16) in zip(data, host):
        with model.native(rec, lig) as nat:
            for _ in range(3):
                o = nat.metrics(poses)
            wall, copy, kern = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                o = nat.metrics(poses)
                wall.append((time.perf_counter() - t0) * 1e3)
                c, k = engine.metrics_last_timing()
                copy.append(c)
                kern.append(k)
            info = nat.info()
        ctx = NativeContext((rec, lig))
        dev = max(abs(o["DockQ"][k] - compute_metrics((rec, poses[k]), (rec, lig), ctx)["DockQ"]) for k in range(0, P, P // 16))
        med = lambda v: float(np.median(v))
        floor_ms = 2 * 36.0 * L * P / HBM_BPS * 1e3
        lines += [
            f"{name}: R = {R}, L = {L}, P = {P}; {info['n_iface_rec']} + {info['n_iface_lig']} interface residues, {info['n_contacts']} contacts",
            f"  host loop, 1 core         {h1:10.0f} poses/s",
            f"  host loop, 16 processes   {h16:10.0f} poses/s   ({P / h16 * 1e3:.1f} ms for P poses)",
            f"  GPU call, wall            {P / med(wall) * 1e3:10.0f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls"
            f" = {h16 and (P / h16 * 1e3) / med(wall):.1f} x the 16-process host loop",
            f"  of which host-to-device   median {med(copy):.2f} ms ({100 * med(copy) / med(wall):.0f} % of wall; {P * L * 36 / med(copy) / 1e6:.1f} GB/s from pageable memory)",
            f"  of which kernels          median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}); byte floor 2 x 36 L P / 6.29 TB/s = {floor_ms:.3f} ms"
            f" -> {100 * floor_ms / med(kern):.0f} % of the HBM roofline",
            f"  max |DockQ gpu - host| over 16 poses: {dev:.2e}",
        ]
        ok = ok and med(wall) < P / h16 * 1e3
    lines.append("gate (whole GPU call, uploads included, faster than the 16-process host loop at every size): " + ("PASS" if ok else "FAIL"))
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
