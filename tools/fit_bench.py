"""Rigid pose fit: kernel and whole-call time of dfm_pose_fit for 10 240 decoys of a 300 + 300 complex, with and without a receptor,
next to the kernel time of dfm_pose_metrics on the same poses and the wall time of the host definition fit.fit_poses.

    python tools/fit_bench.py [--out profiles/fit.txt] [--poses 10240] [--calls 7] [--host-poses 256]

Every figure is the median over --calls calls after one warm-up call; the host definition is timed on --host-poses poses (one core) and
scaled.  Nothing here is a gate: the file records what was measured.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median(xs):
    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit.txt"))
    ap.add_argument("--poses", type=int, default=10240)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=256)
    args = ap.parse_args()
    import fit_harness as fh
    from dfmdock_amd import engine
    from dfmdock_amd.fit import fit_poses
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    R = L = 300
    P = args.poses
    cs = fh.case(1, P, L, R)
    lines = ["rigid pose fit: GPU call (dfm_pose_fit) vs the host definition (fit.fit_poses), and dfm_pose_metrics on the same poses",
             engine.config_string(), f"R = {R}, L = {L}, P = {P}; medians over {args.calls} calls after one warm-up"]
    for name, rec_ref, rec_pos in (("without a receptor", None, None), ("with a receptor", cs["rec_ref"], cs["rec_pos"])):
        wall, copy, kern = [], [], []
        for i in range(args.calls + 1):
            t0 = time.perf_counter()
            out = model.pose_fit(cs["lig_ref"], cs["lig_pos"], cs["center"], rec_ref, rec_pos)
            dt = (time.perf_counter() - t0) * 1e3
            c, k = engine.fit_last_timing()
            if i:
                wall.append(dt); copy.append(c); kern.append(k)
        n = args.host_poses
        t0 = time.perf_counter()
        d = fit_poses(cs["lig_ref"], cs["lig_pos"][:n], cs["center"], rec_ref, None if rec_pos is None else rec_pos[:n])
        host = (time.perf_counter() - t0) / n * P * 1e3
        err = float(np.abs(out["rmsd"][:n] - d[2]).max())
        nbytes = 36 * P * (L + (R if rec_ref is not None else 0))
        lines += [f"{name}",
                  "  GPU call, wall            median %.2f ms (min %.2f, max %.2f) = %.0f poses/s" % (*median(wall), P / median(wall)[0] * 1e3),
                  "  of which host-to-device   median %.2f ms (%.1f GB/s from pageable memory)" % (median(copy)[0], nbytes / median(copy)[0] / 1e6),
                  "  of which kernels          median %.3f ms (min %.3f, max %.3f); the decoys are read twice (reduce, residual): 2 x %.1f MB / kernel time = %.2f TB/s"
                  % (*median(kern), nbytes / 1e6, 2 * nbytes / median(kern)[0] / 1e9),
                  "  host definition, 1 core   %.0f ms for P poses (timed on %d), %.0f x the GPU call's wall time" % (host, n, host / median(wall)[0]),
                  "  max |rmsd gpu - host| over those poses: %.2e A" % err]
    with model.native(cs["rec_ref"], cs["lig_ref"]) as nat:
        kern = []
        for i in range(args.calls + 1):
            nat.metrics(cs["lig_pos"], cs["rec_pos"])
            if i:
                kern.append(engine.metrics_last_timing()[1])
    lines.append("dfm_pose_metrics on the same poses with their receptors (three fits and the contacts): kernels median %.3f ms (min %.3f, max %.3f)" % median(kern))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
