"""Cn symmetric docking (host side): the float64 numpy definition the GPU kernel k_symmetry is tested against, the parameters, the
copies of an n-mer in the engine's pose convention and the assembly of its chains.

Definition (include/dfmdock_amd.h: dfm_complex_set_symmetry).  y [M,3,3] is the stored receptor backbone, x [M,3,3] a ligand pose of the
SAME chain, n the order of the cyclic group:

    (Q, tau)   = the Kabsch fit of y onto x over all 3 M backbone atoms, equal weights, a proper rotation: the monomer-to-monomer
                 transform T of the pose.  fit_rmsd = sqrt(mean |Q y + tau - x|^2)
    (w, v)     = the unit quaternion of Q with w >= 0;  theta = 2 atan2(|v|, w) in [0, pi],  u = v / |v|
                 |v| <= 1e-9: no axis - the step is zero, m = 0, theta = 0, every other diagnostic but fit_rmsd is NaN
    c          = the centre the sampler rotates the ligand about (CA centroid of x; all backbone atoms for the second family)
    g          = Q^T (c - tau)      the receptor-frame point T sends to c
    s          = u . (c - g)        the translation along the axis (the screw component)
    theta*     = 2 pi m / n,  m in 1 .. floor(n / 2) with gcd(m, n) = 1 closest to theta, ties to the smaller m
    projection : rotate x about c by (theta* - theta) u, shift it by -s u.  The new transform T' is a pure rotation by theta* about an
                 axis parallel to u: T'^n = identity.  sym_rmsd = the rms displacement of the 3 M atoms under the projection
    axis_point = (g + c - s u) / 2 + cot(theta* / 2) / 2 * u x (c - g - s u)      a point of the assembly's axis
    step       : domega = clip(gain_rot (theta* - theta) u, max_rot),  dtau = clip(-gain_tr s u, max_tr),  clip(v, m) = v min(1, m / |v|);
                 on the last step with snap_last the gains are 1 and nothing is clipped

and the step moves the ligand as the restraint step does (restraints.apply_step).  A pose with a non-finite coordinate has NaN
diagnostics, m = 0 and a NaN step.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass

import numpy as np

from .metrics import find_rigid_alignment
from .restraints import _centroid, _clip, axis_angle_to_matrix
from .restraints import apply_step as _apply_step

MIN_ORDER, MAX_ORDER = 2, 24
NO_AXIS = 1e-9      # |v| of the fit's quaternion at or below which the pose has no rotation axis


@dataclass(frozen=True)
class SymmetryParams:
    """dfm_symmetry_params.  The defaults are starting values: nobody has measured them against a trained checkpoint."""
    gain_rot: float = 0.5    # fraction of the angle error theta* - theta one step removes, in (0, 1]
    gain_tr: float = 0.5     # fraction of the screw translation one step removes, in (0, 1]
    max_rot: float = 0.3     # rad per step
    max_tr: float = 10.0     # Angstrom per step
    t_start: float = 1.0     # the step runs when t_i <= t_start
    snap_last: int = 1       # the last step projects exactly (gains 1, no clipping)

    def __post_init__(self):
        for name in ("gain_rot", "gain_tr"):
            v = getattr(self, name)
            if not (0.0 < v <= 1.0):
                raise ValueError(f"symmetry: {name} must lie in (0, 1], got {v}")
        for name in ("max_rot", "max_tr"):
            v = getattr(self, name)
            if not (v > 0.0 and math.isfinite(v)):
                raise ValueError(f"symmetry: {name} must be finite and > 0, got {v}")
        if self.t_start != self.t_start:
            raise ValueError("symmetry: t_start must be a number")

    def to_c(self):
        from ._lib import SymmetryParamsC
        return SymmetryParamsC(self.gain_rot, self.gain_tr, self.max_rot, self.max_tr, self.t_start, int(bool(self.snap_last)))


def parse_symmetry(text):
    """"C3", "c3" or "3" -> 3; the order must lie in 2 .. 24."""
    m = re.fullmatch(r"\s*[Cc]?(\d+)\s*", str(text))
    if not m:
        raise ValueError(f"symmetry: cannot read {text!r} (expected Cn or n, e.g. C3)")
    n = int(m.group(1))
    check_order(n)
    return n


def check_order(n):
    if not (isinstance(n, (int, np.integer)) and MIN_ORDER <= n <= MAX_ORDER):
        raise ValueError(f"symmetry: the order must be an integer in {MIN_ORDER} .. {MAX_ORDER}, got {n!r}")
    return int(n)


def select_m(theta, n):
    """(m, theta*) of the definition: m in 1 .. n // 2 coprime to n with |theta - 2 pi m / n| minimal, ties to the smaller m."""
    best_m, best_t, best_d = 0, 0.0, math.inf
    for m in range(1, n // 2 + 1):
        if math.gcd(m, n) != 1:
            continue
        ts = 2.0 * math.pi * m / n
        d = abs(theta - ts)
        if d < best_d:
            best_m, best_t, best_d = m, ts, d
    return best_m, best_t


def _quaternion(Q):
    """The unit quaternion (w, v) with w >= 0 of a proper rotation matrix; the largest candidate component is the pivot."""
    m00, m11, m22 = Q[0, 0], Q[1, 1], Q[2, 2]
    cand = np.array([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22])
    k = int(np.argmax(cand))
    d = 2.0 * np.sqrt(cand[k])
    if k == 0:
        q = np.array([0.25 * d, (Q[2, 1] - Q[1, 2]) / d, (Q[0, 2] - Q[2, 0]) / d, (Q[1, 0] - Q[0, 1]) / d])
    elif k == 1:
        q = np.array([(Q[2, 1] - Q[1, 2]) / d, 0.25 * d, (Q[0, 1] + Q[1, 0]) / d, (Q[0, 2] + Q[2, 0]) / d])
    elif k == 2:
        q = np.array([(Q[0, 2] - Q[2, 0]) / d, (Q[0, 1] + Q[1, 0]) / d, 0.25 * d, (Q[1, 2] + Q[2, 1]) / d])
    else:
        q = np.array([(Q[1, 0] - Q[0, 1]) / d, (Q[0, 2] + Q[2, 0]) / d, (Q[1, 2] + Q[2, 1]) / d, 0.25 * d])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def fit_transform(rec_pos, lig_pos):
    """(Q, tau, fit_rmsd) of the definition: Q y + tau ~ x over all backbone atoms."""
    y = np.asarray(rec_pos, np.float64).reshape(-1, 3)
    x = np.asarray(lig_pos, np.float64).reshape(-1, 3)
    if y.shape != x.shape:
        raise ValueError(f"symmetry: receptor and ligand must have the same length, got {y.shape[0] // 3} and {x.shape[0] // 3} residues")
    Q, tau = find_rigid_alignment(y, x)
    Q, tau = np.asarray(Q, np.float64), np.asarray(tau, np.float64)
    return Q, tau, float(np.sqrt(np.mean(np.sum((y @ Q.T + tau - x) ** 2, -1))))


def evaluate(rec_pos, lig_pos, n, params: SymmetryParams | None = None, center="ca", last=False):
    """The definition at ONE pose (rec_pos, lig_pos [M,3,3]), float64 throughout: a dict of theta, screw, axis [3], axis_point [3],
    fit_rmsd, sym_rmsd, m, theta_star, step [6] = (dtau, domega), Q, tau and `projected`, the pose after the full projection.
    last: this is the sampler's last step (with snap_last the step is the projection itself)."""
    p = params or SymmetryParams()
    n = check_order(n)
    lig = np.asarray(lig_pos, np.float64).reshape(-1, 3, 3)
    y = np.asarray(rec_pos, np.float64).reshape(-1, 3, 3)
    nan3 = np.full(3, np.nan)
    out = {"n": n, "m": 0, "theta": np.nan, "theta_star": np.nan, "screw": np.nan, "axis": nan3.copy(), "axis_point": nan3.copy(),
           "fit_rmsd": np.nan, "sym_rmsd": np.nan, "step": np.full(6, np.nan), "Q": None, "tau": None, "projected": None}
    if y.shape != lig.shape:
        raise ValueError(f"symmetry: receptor and ligand must have the same length, got {y.shape[0]} and {lig.shape[0]} residues")
    if not (np.isfinite(lig).all() and np.isfinite(y).all()):
        return out
    Q, tau, fit_rmsd = fit_transform(y, lig)
    q = _quaternion(Q)
    w, v = q[0], q[1:]
    vn = float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    out.update(Q=Q, tau=tau, fit_rmsd=fit_rmsd)
    if vn <= NO_AXIS:
        out.update(theta=0.0, step=np.zeros(6))
        return out
    theta = 2.0 * math.atan2(vn, w)
    u = v / vn
    c = _centroid(lig, center)
    g = Q.T @ (c - tau)
    s = float(u @ (c - g))
    m, ts = select_m(theta, n)
    full = np.concatenate([-s * u, (ts - theta) * u])
    x = lig.reshape(-1, 3)
    proj = (x - c) @ axis_angle_to_matrix(full[3:]).T + c + full[:3]
    d = c - g - s * u
    axis_point = 0.5 * (g + c - s * u) + 0.5 / math.tan(0.5 * ts) * np.cross(u, d)
    if last and p.snap_last:
        step = full
    else:
        step = np.concatenate([_clip(-p.gain_tr * s * u, p.max_tr), _clip(p.gain_rot * (ts - theta) * u, p.max_rot)])
    out.update(m=m, theta=theta, theta_star=ts, screw=s, axis=u, axis_point=axis_point,
               sym_rmsd=float(np.sqrt(np.mean(np.sum((proj - x) ** 2, -1)))), step=step, projected=proj.reshape(-1, 3, 3))
    return out


def apply_step(lig_pos, step, rot_update=None, tr_update=None, center="ca"):
    """The rigid move of a step (dtau, domega) about the sampler's centroid, float64: (pose, rot_update, tr_update) - the restraint
    step's move (restraints.apply_step).  `step` may be the dict evaluate returns."""
    if isinstance(step, dict):
        step = step["step"]
    return _apply_step(lig_pos, step, rot_update, tr_update, center)


def transform_power(Q, tau, k):
    """T^k of T = (Q, tau), x -> Q x + tau, for k >= 0."""
    Qk, tk = np.eye(3), np.zeros(3)
    for _ in range(int(k)):
        Qk, tk = Q @ Qk, Q @ tk + tau
    return Qk, tk


def closure(rec_pos, Q, tau, n):
    """The largest displacement of a receptor backbone atom under T^n: 0 for an exactly closed n-mer."""
    y = np.asarray(rec_pos, np.float64).reshape(-1, 3)
    Qn, tn = transform_power(np.asarray(Q, np.float64), np.asarray(tau, np.float64), n)
    return float(np.sqrt(np.sum((y @ Qn.T + tn - y) ** 2, -1)).max())


def _pose_backbone(lig_ref_bb, rot, tr, center):
    x0 = np.asarray(lig_ref_bb, np.float64).reshape(-1, 3, 3)
    c = np.asarray(center, np.float64).reshape(3)
    return (x0 - c) @ axis_angle_to_matrix(rot).T + c + np.asarray(tr, np.float64).reshape(3)


def copy_poses(rec_bb, lig_ref_bb, rot, tr, center, n, center_mode="ca"):
    """The poses (rot_k [n-1,3], tr_k [n-1,3]) of copies k = 1 .. n-1 of an n-mer in the engine's pose convention
    x = (x0 - c) R(rot)^T + c + tr acting on the LIGAND's coordinates x0 (lig_ref_bb [M,3,3], `center` c [3]): every dfm_pose_* call and
    pdbio.apply_pose_all_atom place copy k with them.  Copy 1 is the pose (rot, tr) itself; copy k is T'^(k-1) of it, T' the projection
    (pure rotation by theta* about the assembly's axis) of the Kabsch fit of the receptor rec_bb onto the pose - so copy n would be the
    receptor again.  A pose without an axis (or a non-finite one) repeats the fit's own transform.  center_mode ("ca" / "all_atoms"): the
    centre the SAMPLER rotates about for the model's family (evaluate's `center`): the projection T' is taken about it, so the copies are
    those of the written files for a pose that is not yet symmetric too."""
    from .fit import matrix_to_axis_angle
    n = check_order(n)
    c = np.asarray(center, np.float64).reshape(3)
    rot, tr = np.asarray(rot, np.float64).reshape(3), np.asarray(tr, np.float64).reshape(3)
    x = _pose_backbone(lig_ref_bb, rot, tr, c)
    ev = evaluate(rec_bb, x, n, center=center_mode)
    if ev["m"] > 0:
        Qp = axis_angle_to_matrix(ev["theta_star"] * ev["axis"])
        a = ev["axis_point"]
        taup = a - Qp @ a
    elif ev["Q"] is not None:
        Qp, taup = ev["Q"], ev["tau"]
    else:
        Qp, taup = np.full((3, 3), np.nan), np.full(3, np.nan)
    Rm = axis_angle_to_matrix(rot)
    rots, trs = [rot.copy()], [tr.copy()]
    for k in range(2, n):
        Qk, tk = transform_power(Qp, taup, k - 1)
        rots.append(matrix_to_axis_angle(Qk @ Rm) if np.isfinite(Qk).all() else np.full(3, np.nan))
        trs.append(Qk @ (c + tr) + tk - c)
    return np.asarray(rots), np.asarray(trs)


def assemble(rec_bb, lig_ref_bb, rot, tr, center, n, center_mode="ca"):
    """The backbone [n,M,3,3] of the n-mer: the receptor, then copies 1 .. n-1 (copy_poses)."""
    rots, trs = copy_poses(rec_bb, lig_ref_bb, rot, tr, center, n, center_mode)
    chains = [np.asarray(rec_bb, np.float64).reshape(-1, 3, 3)]
    chains += [_pose_backbone(lig_ref_bb, rots[k], trs[k], center) for k in range(n - 1)]
    return np.stack(chains)


def record(rec_bb, lig_bb, n, center="ca"):
    """The `symmetry` record of one final pose (lig_bb [M,3,3]) in the drivers' results: n, m, theta, screw, sym_rmsd, closure, axis,
    axis_point; closure is the largest displacement of a receptor atom under T^n of the pose's own (unprojected) fit."""
    ev = evaluate(rec_bb, lig_bb, n, center=center)
    cl = closure(rec_bb, ev["Q"], ev["tau"], n) if ev["Q"] is not None else float("nan")
    return {"n": int(n), "m": int(ev["m"]), "theta": float(ev["theta"]), "screw": float(ev["screw"]), "sym_rmsd": float(ev["sym_rmsd"]),
            "closure": cl, "axis": [float(v) for v in ev["axis"]], "axis_point": [float(v) for v in ev["axis_point"]]}
