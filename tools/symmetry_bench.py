"""Cn symmetric docking: what the symmetry step costs and how close the kernel is to its float64 definition.

    python tools/symmetry_bench.py [--out profiles/symmetry.txt] [--calls 5] [--batch 256] [--steps 40]

At C3 (300 + 300 homodimer, B = 256, 40 steps, 16-bit engine): dfm_sample with and without DFM_F_SYMMETRY, interleaved in one process
(median over --calls calls each after one warm-up call each), the time of k_symmetry next to k_restraint's from ONE traced run of the
same call with a five-group restraint set stored as well (a child process under rocprofv3 --kernel-trace --stats), and the worst
deviation of dfm_symmetry_eval from symmetry.evaluate over the evaluation poses of tests/symmetry_fixtures.py (the GPU tests' own).  Nothing here is a gate: the file
records what was measured.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_ORDER = 3


def homodimer(B):
    import symmetry_fixtures as T
    from dfmdock_amd import engine
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    gx, y, lig0 = T.homodimer(model, 300, N_ORDER)
    gx.set_symmetry(N_ORDER)
    return model, gx, y, lig0


def five_groups(y, lig0):
    from dfmdock_amd.restraints import native_contact_groups
    for cutoff in (12.0, 16.0, 24.0, 48.0):
        groups = native_contact_groups(y, lig0, 5, cutoff=cutoff, seed=0)
        if len(groups) == 5:
            return groups
    raise RuntimeError("fewer than five CA-CA contacts below 48 A in the start pose")


def traced_run(args):
    """The child under the profiler: one warm-up and one measured call with both steps on."""
    model, gx, y, lig0 = homodimer(args.batch)
    gx.set_restraints(five_groups(y, lig0))
    for seed in (0, 1):
        gx.sample(B=args.batch, num_steps=args.steps, seed=seed, mfma16=True, symmetry=True, restraints=True)


def kernel_times(args):
    """{kernel: (calls, average us, min us, max us)} of k_symmetry and k_restraint from a traced child, or a string saying why not."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return "rocprofv3 not found: no kernel times"
    tmp = tempfile.mkdtemp(prefix="symprof_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--traced-run", "--batch", str(args.batch), "--steps", str(args.steps)]
        # the child ran on the GPU: if it did not end cleanly (a fault, an abort, a time limit), nothing more is started on that card
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            sys.exit("symmetry_bench: the traced run did not end within 600 s; stopping here, nothing else was run on the GPU")
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            sys.exit(f"symmetry_bench: the traced run ended with exit status {p.returncode}; stopping here, nothing else was run on the GPU")
        files = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if not files:
            return "the traced run left no kernel_stats.csv: no kernel times"
        out = {}
        for r in csv.DictReader(open(files[0])):
            for k in ("k_symmetry", "k_restraint"):
                if k in r["Name"]:
                    out[k] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def deviations(model):
    """Worst |device - definition| per output over the evaluation cases of the test suite (all sizes, n = 2, 3, 5, 8, B = 64)."""
    import symmetry_fixtures as T
    from dfmdock_amd import symmetry as SY
    worst = {}
    for size in (9, 24, "7CEI", 300):
        gx, y, _ = T.homodimer(model, size)
        for n in (2, 3, 5, 8):
            poses = T.poses(y, n, 64, np.random.default_rng(100 * n + len(y)))
            gx.set_symmetry(n)
            w, _ = T.check_eval(gx.symmetry_eval(poses), y, poses, n, SY.SymmetryParams())
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        gx.close()
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symmetry.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--traced-run", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.traced_run:
        return traced_run(args)
    from dfmdock_amd import engine
    kt = kernel_times(args)      # (first: the child is gone before this process opens the GPU)
    model, gx, y, lig0 = homodimer(args.batch)
    B, S = args.batch, args.steps
    wall = {False: [], True: []}
    for i in range(args.calls + 1):
        for flag in (False, True):      # interleaved: off, on, off, on, ...
            t0 = time.perf_counter()
            r = gx.sample(B=B, num_steps=S, seed=i, mfma16=True, symmetry=flag)
            dt = time.perf_counter() - t0
            if i:
                wall[flag].append(dt)
    med = {f: float(np.median(v)) for f, v in wall.items()}
    import symmetry_fixtures as T
    cl = np.array([T.closure(y, p, N_ORDER) for p in r["lig_pos"]])
    lines = ["Cn symmetry step: cost at C3 and deviation from the float64 definition (tools/symmetry_bench.py)", engine.config_string(),
             f"homodimer 300 + 300, n = {N_ORDER}, B = {B}, {S} steps, mfma16, default dfm_symmetry_params; medians over {args.calls} calls each, "
             "interleaved off / on in one process, after one warm-up call each",
             "  dfm_sample without the flag   median %.1f ms (min %.1f, max %.1f) = %.1f traj/s"
             % (med[False] * 1e3, min(wall[False]) * 1e3, max(wall[False]) * 1e3, B / med[False]),
             "  dfm_sample with DFM_F_SYMMETRY median %.1f ms (min %.1f, max %.1f) = %.1f traj/s"
             % (med[True] * 1e3, min(wall[True]) * 1e3, max(wall[True]) * 1e3, B / med[True]),
             "  the flag's cost: %+.2f %% of the unflagged call's time (%+.1f us per step)"
             % ((med[True] / med[False] - 1) * 100, (med[True] - med[False]) / S * 1e6),
             "  (the two calls do not sample the same poses: symmetric trajectories stay where the step holds them)",
             "  final poses of the last flagged call: closure max %.2e A, |theta - theta*| max %.2e rad, |screw| max %.2e A"
             % (cl[:, 0].max(), cl[:, 1].max(), cl[:, 2].max())]
    if isinstance(kt, str):
        lines.append(kt)
    else:
        lines.append("kernel times of one traced run of the same call with a five-group restraint set stored as well (rocprofv3 --kernel-trace --stats;"
                     " k_symmetry, the last kernel to move the pose, also prepares it for the next evaluation - k_restraint does not, then):")
        for k in ("k_symmetry", "k_restraint"):
            if k in kt:
                lines.append("  %-12s %4d launches, average %.1f us (min %.1f, max %.1f)" % ((k,) + kt[k]))
            else:
                lines.append(f"  {k}: not in the trace")
    gx.close()
    w = deviations(model)
    lines.append("worst |dfm_symmetry_eval - symmetry.evaluate| over M = 9, 24, 87, 300, n = 2, 3, 5, 8, 64 poses each (gates: theta 1e-11 rad, axis 1e-10, the rest 1e-8 A; step: 2 fp32 ulp of the step recomputed in float64 from the device's own theta, axis, screw - every pose counted):")
    lines.append("  theta %.2e rad, axis %.2e, screw %.2e A, axis_point %.2e A, fit_rmsd %.2e A, sym_rmsd %.2e A, step %.2f fp32 ulp"
                 % tuple(w[k] for k in ("theta", "axis", "screw", "axis_point", "fit_rmsd", "sym_rmsd", "step_ulp")))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
