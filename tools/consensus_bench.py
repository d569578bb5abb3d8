"""Poses per second of consensus contact scoring on the GPU (dfm_pose_consensus) against the float64 numpy definition
(dfmdock_amd/consensus.py) on the same host: 10 240 perturbed poses of the 300 + 300 complex and 2 048 poses of the 1000 + 1000 complex.
Writes profiles/consensus.txt.

    python tools/consensus_bench.py [--out profiles/consensus.txt] [--reps 7] [--host-poses 256]

GPU: warm-up calls, then `reps` timed calls; wall time of the whole call (upload, kernels, download, host finish) from a host clock, copy
and kernel time from the call's own HIP events (dfm_consensus_last_timing); median and min-max.  The definition is timed on the first
`host-poses` poses and scaled linearly to P (labelled as scaled).  Before any time is printed the GPU results of the timed call are
asserted against the definition on that subset (bits outside a 1e-3 A border of the cutoff, the integer outputs from the call's own bits).

Two ceilings, computed here.  Bytes: the poses are read once, the contact bits are written once and read by the count, marginal (twice)
and score kernels, over the 8 TB/s HBM figure.  Float64 work: the residue pairs that survive the cheap reject (recomputed on the host
with the kernel's rule in float32) cost 9 atom pairs x 9 operations (3 subtractions, 3 multiplications, 2 additions, 1 square root
counted as one), over the MI355X data sheet's vector fp64 peak of 78.6 TFLOP/s (half its 157.3 TFLOP/s fp32 vector figure)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12
FP64_FLOPS = 78.6e12
CUTOFF = 5.5


def make_case(R, L, P, seed):
    """P rigid perturbations of a synthetic complex: scales 0 ... 1 (rotation vector s N(0,1)^3 rad about the CA centroid, translation
    N(0, (10 s)^2) A per axis), the spread of tests/test_gpu_metrics.py."""
    from dfmdock_amd.synthetic import make_complex
    from dfmdock_amd.restraints import axis_angle_to_matrix
    cx = make_complex(R, L, seed=seed)
    rng = np.random.default_rng(seed)
    lig = np.asarray(cx["lig_pos"], np.float64)
    cen = lig[:, 1].mean(0)
    poses = np.empty((P,) + lig.shape, np.float32)
    for p in range(P):
        s = (p % 16) / 15.0
        poses[p] = ((lig - cen) @ axis_angle_to_matrix(s * rng.standard_normal(3)).T + cen + 10.0 * s * rng.standard_normal(3)).astype(np.float32)
    return np.asarray(cx["rec_pos"], np.float32), poses


def reach(x):
    """The kernel's reach of every residue of x [..., 3, 3] in float32: the larger of |N - CA| and |C - CA|."""
    x = np.asarray(x, np.float32)
    a, c = x[..., 0, :] - x[..., 1, :], x[..., 2, :] - x[..., 1, :]
    a2 = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
    c2 = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
    return np.sqrt(np.maximum(a2, c2))


def surviving_pairs(rec, poses):
    """Residue pairs of `poses` the cheap reject of k_contact_bits lets through, by the kernel's rule in float32."""
    rec, n = np.asarray(rec, np.float32).reshape(-1, 3, 3), 0
    rr = reach(rec)
    one = np.float32(1.0001), np.float32(1e-3)
    for lig in np.asarray(poses, np.float32):
        d = rec[:, None, 1, :] - lig[None, :, 1, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        thr = ((np.float32(CUTOFF) + reach(lig))[None, :] + rr[:, None]) * one[0] + one[1]
        n += int((~(d2 > thr * thr)).sum())
    return n


def check_subset(got, rec, poses, n):
    """The sanity condition: the timed call's results on the first n poses against the definition - the bits outside the border, and
    n_contacts / score_sum as the definition's formulas give them from the call's own bits and count."""
    from dfmdock_amd import consensus as CS
    mine, high = CS.unpack_bits(got["bits"][:n], poses.shape[1])
    assert high == 0
    contacts = border = 0
    for p in range(n):
        d = CS.min_dist(rec, poses[p])
        want, edge = d < CUTOFF, np.abs(d - CUTOFF) < 1e-3
        assert not ((mine[p] != want) & ~edge).any(), p
        assert int(mine[p].sum()) == int(got["n_contacts"][p]) and int(got["count"][mine[p]].sum(dtype=np.int64)) == int(got["score_sum"][p]), p
        contacts += int(want.sum())
        border += int(edge.sum())
    assert got["consensus"].tobytes() == CS.finish(got["score_sum"], got["n_contacts"], got["M"]).tobytes()
    return contacts, border


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-poses", type=int, default=256, help="poses the numpy definition is timed on (scaled linearly to P)")
    a = ap.parse_args()
    from dfmdock_amd import consensus as CS
    from dfmdock_amd import engine
    from dfmdock_amd.weights import make_random_weights, pack_blob
    cases = [("C3 ensemble", 300, 300, 10240, 1), ("C5 ensemble", 1000, 1000, 2048, 1)]
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    lines = ["consensus contact scoring: GPU call (dfm_pose_consensus) vs the float64 numpy definition (consensus.consensus)", engine.config_string()]
    med = lambda v: float(np.median(v))
    for name, R, L, P, seed in cases:
        rec, poses = make_case(R, L, P, seed)
        n = min(a.host_poses, P)
        t0 = time.perf_counter()
        CS.consensus(rec, poses[:n])
        host_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(2):
            model.consensus(rec, poses)
        wall, copy, kern = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            o = model.consensus(rec, poses)
            wall.append((time.perf_counter() - t0) * 1e3)
            c, k = engine.consensus_last_timing()
            copy.append(c)
            kern.append(k)
        got = model.consensus(rec, poses, bits=True)      # the same call with the bits handed out, for the check
        for k in ("count", "n_contacts", "score_sum"):
            assert np.array_equal(got[k], o[k]), k
        contacts, border = check_subset(got, rec, poses, n)
        chunks = -(-P // engine.consensus_chunk_poses(R, L))
        W = (L + 63) // 64
        pairs = P * R * L
        alive = surviving_pairs(rec, poses[:n]) * (P / n)
        passes = 2 if chunks > 1 else 1      # a call of several chunks evaluates the bits twice
        byte_ms = (passes * P * L * 36 + (passes + 4) * P * R * W * 8) / HBM_BPS * 1e3
        flop_ms = passes * alive * 81 / FP64_FLOPS * 1e3
        lines += [
            f"{name}: R = {R}, L = {L}, P = {P} ({chunks} chunk{'s' if chunks > 1 else ''}); {int(got['n_contacts'].sum())} contacts in {pairs} residue pairs, "
            f"{int((got['n_contacts'] == 0).sum())} poses without a contact; checked against the definition on {n} poses ({contacts} contacts, {border} border pairs)",
            f"  numpy definition, 1 core  {n / host_ms * 1e3:10.1f} poses/s   {host_ms:.0f} ms for {n} poses = {host_ms * P / n:.0f} ms for P poses (scaled)",
            f"  GPU call, wall            {P / med(wall) * 1e3:10.1f} poses/s   median {med(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f}) over {a.reps} calls"
            f" = {host_ms * P / n / med(wall):.0f} x the scaled definition",
            f"  of which host-to-device   median {med(copy):.2f} ms ({100 * med(copy) / med(wall):.0f} % of wall; {passes * P * L * 36 / med(copy) / 1e6:.1f} GB/s from pageable memory)",
            f"  of which kernels          median {med(kern):.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}) = {pairs * 9 / med(kern) / 1e6:.1f} G atom-pair "
            f"distances/s nominal ({pairs / med(kern) / 1e6:.1f} G residue pairs/s)",
            f"  cheap reject              {100 * alive / pairs:.3f} % of the residue pairs survive (host, the kernel's float32 rule, on {n} poses): "
            f"{alive * 9 * passes / 1e6:.1f} M float64 atom-pair distances evaluated",
            f"  ceilings                  bytes {byte_ms:.3f} ms at 8 TB/s ({100 * byte_ms / med(kern):.1f} % of the kernel time); float64 "
            f"{flop_ms:.4f} ms at 78.6 TFLOP/s ({100 * flop_ms / med(kern):.2f} %): the kernels are bound by "
            f"{'neither: the float32 reject over all residue pairs and launch granularity dominate' if max(byte_ms, flop_ms) < 0.5 * med(kern) else ('bytes' if byte_ms > flop_ms else 'float64 work')}",
        ]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
