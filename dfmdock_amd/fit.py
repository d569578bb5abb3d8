"""Rigid pose fit (host side): the float64 numpy definition the GPU call engine.Model.pose_fit (dfm_pose_fit, kernels_fit.hip) is tested
against - from the backbone coordinates of a rigidly placed ligand back to the sampler's (rot_update, tr_update).

Definition.  lig_ref [L,3,3] is the input ligand x0, lig_pos [P,L,3,3] the decoys' ligands x, `center` c the point the sampler rotates
the ligand about (cluster.rebuild_backbone: the CA centroid for family 0, the backbone centroid for family 1).  The points of a fit are
all 3 L (3 R) backbone atoms N, CA, C with equal weights; a fit is Kabsch's, by SVD with the reflection fix (metrics.find_rigid_alignment).

    with a receptor (rec_ref y_ref [R,3,3], rec_pos y [P,R,3,3]: decoys in a frame of their own)
        (Q, s)   = the fit of y onto y_ref                         rec_rmsd = sqrt(mean |Q y + s - y_ref|^2)
        x'       = Q x + s                                         (without a receptor x' = x)
    (R, t)       = the fit of x0 onto x'                           rmsd = sqrt(mean |R x0 + t - x'|^2), the explicit residuals
    rot          = the axis-angle of R, angle in [0, pi]; exactly the zero vector when R is the identity
    tr           = t + R c - c                                     so that x' = (x0 - c) R(rot)^T + c + tr

which is the convention of cluster.rebuild_backbone, pdbio.apply_pose_all_atom and every dfm_pose_* call.  A decoy whose rmsd (or
rec_rmsd) is above a tolerance is no rigid image of the input.  A pose with any non-finite input coordinate has rot, tr, rmsd (and
rec_rmsd) all NaN.
"""
from __future__ import annotations

import numpy as np

from .metrics import find_rigid_alignment


def matrix_to_axis_angle(R):
    """The axis-angle [3] of a proper rotation matrix, angle in [0, pi], through the unit quaternion with w >= 0 (the largest of the four
    candidate components is the pivot, so no branch divides by a small number); exactly zero when R is the identity."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    if np.array_equal(R, np.eye(3)):
        return np.zeros(3)
    m00, m11, m22 = R[0, 0], R[1, 1], R[2, 2]
    cand = np.array([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22])
    k = int(np.argmax(cand))
    d = 2.0 * np.sqrt(cand[k])
    if k == 0:
        q = np.array([0.25 * d, (R[2, 1] - R[1, 2]) / d, (R[0, 2] - R[2, 0]) / d, (R[1, 0] - R[0, 1]) / d])
    elif k == 1:
        q = np.array([(R[2, 1] - R[1, 2]) / d, 0.25 * d, (R[0, 1] + R[1, 0]) / d, (R[0, 2] + R[2, 0]) / d])
    elif k == 2:
        q = np.array([(R[0, 2] - R[2, 0]) / d, (R[0, 1] + R[1, 0]) / d, 0.25 * d, (R[1, 2] + R[2, 1]) / d])
    else:
        q = np.array([(R[1, 0] - R[0, 1]) / d, (R[0, 2] + R[2, 0]) / d, (R[1, 2] + R[2, 1]) / d, 0.25 * d])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    vn = np.linalg.norm(q[1:])
    if not vn > 0:
        return np.zeros(3)
    return q[1:] * (2.0 * np.arctan2(vn, q[0]) / vn)


def _points(x, what):
    a = np.asarray(x, np.float64)
    if a.size == 0 or a.size % 9:
        raise ValueError(f"{what} must be [n,3,3], got {np.shape(x)}")
    return a.reshape(-1, 3)


def fit_poses(lig_ref, lig_pos, center, rec_ref=None, rec_pos=None):
    """lig_ref [L,3,3], lig_pos [P,L,3,3], center [3], rec_ref [R,3,3] / rec_pos [P,R,3,3] both or neither ->
    (rot [P,3], tr [P,3], rmsd [P], rec_rmsd [P] or None), float64 (the module's docstring is the definition)."""
    if (rec_ref is None) != (rec_pos is None):
        raise ValueError("rec_ref and rec_pos must be given together")
    x0 = _points(lig_ref, "lig_ref")
    lp = np.asarray(lig_pos, np.float64)
    if lp.size == 0 or lp.size % x0.size:
        raise ValueError(f"lig_pos must be [P,{x0.shape[0] // 3},3,3], got {np.shape(lig_pos)}")
    P = lp.size // x0.size
    X = lp.reshape(P, -1, 3)
    c = np.asarray(center, np.float64).reshape(3)
    y_ref = Y = None
    if rec_ref is not None:
        y_ref = _points(rec_ref, "rec_ref")
        rp = np.asarray(rec_pos, np.float64)
        if rp.size != P * y_ref.size:
            raise ValueError(f"rec_pos must be [{P},{y_ref.shape[0] // 3},3,3], got {np.shape(rec_pos)}")
        Y = rp.reshape(P, -1, 3)
    rot, tr = np.full((P, 3), np.nan), np.full((P, 3), np.nan)
    rmsd = np.full(P, np.nan)
    rec_rmsd = None if Y is None else np.full(P, np.nan)
    fixed = np.isfinite(x0).all() and np.isfinite(c).all() and (y_ref is None or np.isfinite(y_ref).all())
    for p in range(P):
        if not (fixed and np.isfinite(X[p]).all() and (Y is None or np.isfinite(Y[p]).all())):
            continue
        x = X[p]
        if Y is not None:
            Q, s = find_rigid_alignment(Y[p], y_ref)
            rec_rmsd[p] = np.sqrt(np.mean(np.sum((Y[p] @ Q.T + s - y_ref) ** 2, -1)))
            x = x @ Q.T + s
        # identical point sets: the optimum is the identity itself, not the SVD's identity to rounding
        R, t = (np.eye(3), np.zeros(3)) if np.array_equal(x, x0) else find_rigid_alignment(x0, x)
        rmsd[p] = np.sqrt(np.mean(np.sum((x0 @ R.T + t - x) ** 2, -1)))
        rot[p] = matrix_to_axis_angle(R)
        tr[p] = t + R @ c - c
    return rot, tr, rmsd, rec_rmsd
