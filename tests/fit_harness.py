"""Kernel-level harness of the rigid-pose-fit kernels (tests/kernels/fit_harness.hip): k_fit_reduce, k_fit_solve and k_fit_resid of
kernels_fit.hip, launch by launch, under the guard-band protocol of tests/kernel_harness.py.  This module binds the shim and holds the
seeded inputs and the float64 comparisons that tests/test_gpu_fit.py uses (tests/test_fit_cpu.py runs the generators and the
comparisons against the definition on the host).

Gates (the project's own for an fp64 kernel against float64, tests/metrics_harness.py):
  rotations   |R R^T - I| <= 1e-13, |det R - 1| <= 1e-13, tr(R M) >= s1 + s2 + sign(det M) s3 - 1e-12 s1 (the SVD optimum of a proper
              rotation) for the fp64 rotation before rounding;
  RMSDs       1e-9 A + 1e-9 rmsd against fit.fit_poses on the same fp32 inputs;
  rot, tr     the public call's fp32 values within 2 ulp of the definition's values rounded to fp32.
"""
import ctypes as C
import functools

import numpy as np

import kernel_harness as kh
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, Out, guards_intact      # noqa: F401 (re-exported)

ORTHO_TOL, DET_TOL, OPT_TOL = 1e-13, 1e-13, 1e-12
RMSD_ABS, RMSD_REL = 1e-9, 1e-9
ULPS = 2
SLOTS = ("lig_ref", "lig_pos", "rec_ref", "rec_pos", "sums", "xf", "rot", "tr", "rmsd", "rec_rmsd")
OPS = ("reduce", "solve", "resid", "full")
f32 = np.float32


class Call(C.Structure):
    _fields_ = [("buf", kh.Buf * len(SLOTS)), ("o", C.c_double * 3), ("P", C.c_int), ("L", C.c_int), ("R", C.c_int)]


compile_shim = functools.partial(kh.compile_shim, "fit")


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------
def chain(rng, n, where, spread=30.0):
    """[n,3,3] float32 backbone-like points: residues uniform within `spread` A of `where`, the three atoms within 1.5 A of each other."""
    ca = where + rng.uniform(-spread, spread, (n, 1, 3))
    return (ca + rng.uniform(-1.5, 1.5, (n, 3, 3))).astype(f32)


def center_of(lig_ref, family):
    """The centre cluster.rebuild_backbone rotates about, as the fp32 triple the call takes."""
    x = np.asarray(lig_ref, f32).astype(np.float64)
    return (x.reshape(-1, 3).mean(0) if family == 1 else x[:, 1].mean(0)).astype(f32)


def random_poses(rng, P, max_tr=50.0):
    """rot [P,3] (angle uniform in [0.05, pi - 0.05]), tr [P,3] float64."""
    axis = rng.standard_normal((P, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    return axis * rng.uniform(0.05, np.pi - 0.05, (P, 1)), rng.uniform(-max_tr, max_tr, (P, 3))


def apply(x0, rot, tr, c):
    """x = (x0 - c) R(rot)^T + c + tr in float64, rounded to fp32: [P,n,3,3]."""
    from dfmdock_amd.pdbio import axis_angle_to_matrix
    x0 = np.asarray(x0, f32).astype(np.float64)
    c = np.asarray(c, np.float64)
    return np.stack([((x0 - c) @ axis_angle_to_matrix(r).T + c + t).astype(f32) for r, t in zip(rot, tr)])


def case(seed, P, L, R=0, family=0):
    """A seeded case within the round trip's premises (coordinates within 256 A, lever arms within 64 A): lig_ref, P rigid images of it
    and, with R > 0, a receptor and every decoy (receptor and ligand) carried into a frame of its own by a second rigid motion."""
    rng = np.random.default_rng(seed)
    where = rng.uniform(-60.0, 60.0, 3)
    lig_ref = chain(rng, L, where)
    c = center_of(lig_ref, family)
    rot, tr = random_poses(rng, P)
    lig_pos = apply(lig_ref, rot, tr, c)
    out = dict(P=P, L=L, R=R, family=family, lig_ref=lig_ref, lig_pos=lig_pos, center=c, rot=rot, tr=tr, rec_ref=None, rec_pos=None)
    if R:
        rec_ref = chain(rng, R, where + rng.uniform(-20.0, 20.0, 3))
        g_rot, g_tr = random_poses(rng, P, 40.0)
        pivot = where
        out["rec_ref"], out["rec_pos"] = rec_ref, np.stack([apply(rec_ref, g_rot[p:p + 1], g_tr[p:p + 1], pivot)[0] for p in range(P)])
        out["lig_pos"] = np.stack([apply(lig_pos[p], g_rot[p:p + 1], g_tr[p:p + 1], pivot)[0] for p in range(P)])
    return out


def definition(cs):
    from dfmdock_amd.fit import fit_poses
    return fit_poses(cs["lig_ref"], cs["lig_pos"], cs["center"], cs["rec_ref"], cs["rec_pos"])


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def rotation_defects(Rm):
    """(|R R^T - I|, |det R - 1|) of a 3 x 3 matrix."""
    Rm = np.asarray(Rm, np.float64).reshape(3, 3)
    return float(np.abs(Rm @ Rm.T - np.eye(3)).max()), float(abs(np.linalg.det(Rm) - 1.0))


def optimality_gap(Rm, p, q):
    """(SVD optimum - tr(R M)) / s1 for M = sum (p - pm)(q - qm)^T: how far R is from the best proper rotation of p onto q."""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    M = (p - p.mean(0)).T @ (q - q.mean(0))
    s = np.linalg.svd(M, compute_uv=False)
    best = s[0] + s[1] + (1.0 if np.linalg.det(M) >= 0 else -1.0) * s[2]
    got = float(np.trace(np.asarray(Rm, np.float64).reshape(3, 3) @ M))
    return (best - got) / max(s[0], 1e-300)


def check_xf(xf, cs):
    """Every finite pose's two rotations of xf [P,24] are proper and optimal: Q for the receptor, R for the ligand against x' = Q x + s
    with the kernel's own (Q, s).  Returns the largest defect / gate of each kind."""
    worst = {"ortho": 0.0, "det": 0.0, "optimality": 0.0}
    x0 = cs["lig_ref"].astype(np.float64).reshape(-1, 3) - cs["center"].astype(np.float64)
    for p in range(cs["P"]):
        f = xf[p]
        if not np.isfinite(f).all():
            continue
        Rm, Q, s = f[:9].reshape(3, 3), f[12:21].reshape(3, 3), f[21:24]
        x = (cs["lig_pos"][p].astype(np.float64).reshape(-1, 3) - cs["center"].astype(np.float64)) @ Q.T + s
        fits = [(Rm, x0, x)]
        if cs["R"]:
            o = cs["center"].astype(np.float64)
            fits.append((Q, cs["rec_pos"][p].astype(np.float64).reshape(-1, 3) - o, cs["rec_ref"].astype(np.float64).reshape(-1, 3) - o))
        else:
            assert np.array_equal(Q, np.eye(3)) and not s.any(), "without a receptor (Q, s) is the identity"
        for M, a, b in fits:
            d_o, d_d = rotation_defects(M)
            worst["ortho"] = max(worst["ortho"], d_o / ORTHO_TOL)
            worst["det"] = max(worst["det"], d_d / DET_TOL)
            worst["optimality"] = max(worst["optimality"], optimality_gap(M, a, b) / OPT_TOL)
    assert max(worst.values()) <= 1.0, worst
    return worst


def check_rmsd(got, want):
    """max |got - want| / (1e-9 + 1e-9 want) over the finite entries; NaN where and only where the definition has NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    r = float((np.abs(got[ok] - want[ok]) / (RMSD_ABS + RMSD_REL * want[ok])).max()) if ok.any() else 0.0
    assert r <= 1.0, r
    return r


def check_ulps(got, want64):
    """The fp32 outputs against the definition's float64 values rounded to fp32: within ULPS ulp of that value, entry by entry."""
    want = np.asarray(want64, np.float64).astype(f32)
    got = np.asarray(got, f32)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    r = float((np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) / np.spacing(np.abs(want[ok])).astype(np.float64)).max()) if ok.any() else 0.0
    assert r <= ULPS, r
    return r


HALF_ULP = 1.5e-5      # A: the half-ulp of an fp32 coordinate below 256 A, as the round trip's bound counts it
ROUND_TRIP = 1e-4      # A: two coordinate roundings, rot (2^-24 pi 64 A) and tr


def frame_bound(cs, p):
    """The round trip's bound for decoy p of a case whose decoys sit in frames of their own: ROUND_TRIP, plus HALF_ULP for the second
    rounding of the moved ligand, plus what the rounded receptor leaves of the frame.  Each receptor atom is off by at most e =
    sqrt(3) HALF_ULP.  To first order the fitted rotation is off by the vector w with (tr(S) I - S) w = sum y_i x e_i, S = sum y_i y_i^T
    over the centred receptor atoms, so |w| <= e sum |y_i| / (s2^2 + s3^2) with the singular values s1 >= s2 >= s3 of the centred atoms;
    the fitted translation is off by at most e; a ligand atom at distance D from the receptor's centroid moves by at most |w| D + e."""
    y = cs["rec_pos"][p].astype(np.float64).reshape(-1, 3)
    yc = y - y.mean(0)
    sv = np.linalg.svd(yc, compute_uv=False)
    e = np.sqrt(3.0) * HALF_ULP
    D = np.linalg.norm(cs["lig_pos"][p].astype(np.float64).reshape(-1, 3) - y.mean(0), axis=1).max()
    return ROUND_TRIP + HALF_ULP + e * (1.0 + D * np.linalg.norm(yc, axis=1).sum() / (sv[1] ** 2 + sv[2] ** 2))


# ---- binding ----------------------------------------------------------------------------------------------------------------------------
class Harness(kh.KernelHarness):
    check = True      # run() asserts success unless told check=False

    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)

    def _in(self, cs):
        return dict(lig_ref=cs["lig_ref"], lig_pos=cs["lig_pos"], rec_ref=cs["rec_ref"], rec_pos=cs["rec_pos"])

    def _scalars(self, cs):
        return dict(P=cs["P"], L=cs["L"], R=cs["R"], o=cs["center"].astype(np.float64))

    def _outs(self, cs, names):
        P, ch = cs["P"], 2 if cs["R"] else 1
        sizes = dict(sums=(np.float64, P * ch * 15), xf=(np.float64, P * 24), rot=(f32, P * 3), tr=(f32, P * 3), rmsd=(np.float64, P),
                     rec_rmsd=(np.float64, P))
        return {k: Out(*sizes[k]) for k in names if k != "rec_rmsd" or cs["R"]}

    def _shape(self, cs, r):
        P, ch = cs["P"], 2 if cs["R"] else 1
        shapes = dict(sums=(P, ch, 15), xf=(P, 24), rot=(P, 3), tr=(P, 3), rmsd=(P,), rec_rmsd=(P,))
        return {k: (v.reshape(shapes[k]) if k in shapes else v) for k, v in r.items()}

    def full(self, cs):
        r = self.run("full", dict(self._in(cs), **self._outs(cs, ("sums", "xf", "rot", "tr", "rmsd", "rec_rmsd"))), **self._scalars(cs))
        return self._shape(cs, r)

    def reduce(self, cs):
        return self._shape(cs, self.run("reduce", dict(self._in(cs), **self._outs(cs, ("sums",))), **self._scalars(cs)))

    def solve(self, cs, sums):
        return self._shape(cs, self.run("solve", dict(sums=sums, **self._outs(cs, ("xf", "rot", "tr"))), **self._scalars(cs)))

    def resid(self, cs, xf):
        r = self.run("resid", dict(self._in(cs), xf=xf, **self._outs(cs, ("rmsd", "rec_rmsd"))), **self._scalars(cs))
        return self._shape(cs, r)


if __name__ == "__main__":
    import sys
    kh.child_main(Harness, sys.argv)
