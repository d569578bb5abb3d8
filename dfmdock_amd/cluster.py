"""Pose clustering (host side): the float64 numpy definition the GPU kernels of dfm_pose_rmsd / dfm_pose_cluster are tested against, the
backbone every trajectory is clustered on, and the ranking keys of the drivers.

Definition (include/dfmdock_amd.h: dfm_pose_cluster).  Poses lig_pos [B, L, 9] (N, CA, C per residue, the sampler's layout) and a
ligand-residue subset S (default: all L residues):

    rmsd_ab = sqrt( mean over the 3 |S| atoms of S of |x_a - x_b|^2 )      (no superposition: the receptor frame is the same in every
                                                                           trajectory, so this is the pairwise L-RMSD of CAPRI / DockQ)
    a ~ b  <=>  rmsd_ab <= radius                                         (a pose is its own neighbour)
A pose with a non-finite coordinate among the compared residues has a non-finite rmsd to every pose, itself included (NaN for a NaN
coordinate): it is no pose's neighbour, not even its own, never opens a cluster under either rule and keeps cluster_of = -1.

Ranking: a per-pose key, lower is better, ties to the lower index, NaN last (`rank_order`).
  rule "energy" (leader clustering): walk the poses in key order; an unassigned pose opens a cluster that its unassigned neighbours join.
  rule "size" (ClusPro-style greedy): repeatedly the unassigned pose with the most unassigned neighbours (ties: better key, then lower
      index) and its unassigned neighbours form the next cluster.
Both stop after max_clusters clusters, or when no pose that is its own neighbour is left (every cluster has size >= 1); poses still
unassigned then belong to cluster -1.  Clusters are numbered in the order they formed.
"""
from __future__ import annotations

import numpy as np

RULES = ("energy", "size")
MAX_POSES = 65536


def _poses(lig_pos):
    x = np.asarray(lig_pos)
    if x.ndim == 4:
        x = x.reshape(x.shape[0], x.shape[1], 9)
    if x.ndim != 3 or x.shape[2] != 9:
        raise ValueError(f"lig_pos must be [B, L, 9] or [B, L, 3, 3], got {np.shape(lig_pos)}")
    return x


def check_residues(residues, L):
    """The residue subset as int32 indices (None: all L); raises ValueError for an empty, out-of-range or duplicated subset."""
    if residues is None:
        return None
    r = np.asarray(residues).reshape(-1)
    if r.size == 0 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("residues must be a non-empty list of ligand residue indices")
    if r.min() < 0 or r.max() >= L:
        raise ValueError(f"residues must lie in [0, {L})")
    if np.unique(r).size != r.size:
        raise ValueError("residues must not repeat")
    return r.astype(np.int32)


def pose_rmsd(lig_pos, residues=None):
    """[B, B] float64 pairwise RMSD over the backbone atoms of `residues`, no superposition."""
    x = _poses(lig_pos)
    r = check_residues(residues, x.shape[1])
    if r is not None:
        x = x[:, r]
    x = x.reshape(x.shape[0], -1, 3).astype(np.float64)
    B, n = x.shape[0], x.shape[1]
    out = np.empty((B, B), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):      # a non-finite coordinate makes its pose's row and column non-finite
        for a in range(B):      # direct differences (the Gram form cancels: |x|^2 ~ 1e6 A^2 against 1e1 for a close pair)
            out[a] = np.sqrt(((x - x[a]) ** 2).sum(-1).sum(-1) / n)
    return out


def rank_order(key, B):
    """Pose indices in key order: lower key first, ties to the lower index, NaN last.  key None: index order."""
    if key is None:
        return np.arange(B)
    k = np.asarray(key, np.float64).reshape(-1)
    if k.size != B:
        raise ValueError(f"key must have {B} entries, got {k.size}")
    nan = np.isnan(k)
    return np.lexsort((np.arange(B), np.where(nan, 0.0, k), nan))


def cluster_adjacency(adj, key=None, rule="energy", max_clusters=None):
    """The two rules on a boolean neighbour matrix adj [B, B] (symmetric; the diagonal True but for poses with a non-finite coordinate).
    Returns {n_clusters, center, size, cluster_of} as int32 arrays (center / size have n_clusters entries)."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
    adj = np.asarray(adj, bool)
    B = adj.shape[0]
    maxc = B if max_clusters is None else int(max_clusters)
    if maxc < 1:
        raise ValueError("max_clusters must be >= 1")
    order = rank_order(key, B)
    pos = np.empty(B, np.int64)
    pos[order] = np.arange(B)
    free = adj.diagonal().copy()      # a pose that is not its own neighbour (a non-finite coordinate) opens no cluster and joins none
    cluster_of = np.full(B, -1, np.int32)
    center, size = [], []
    if rule == "energy":
        for p in order:
            if len(center) == maxc:
                break
            if not free[p]:
                continue
            m = adj[p] & free
            cluster_of[m] = len(center)
            free &= ~m
            center.append(int(p))
            size.append(int(m.sum()))
    else:
        count = adj.sum(1).astype(np.int64)
        while len(center) < maxc and free.any():
            cand = np.nonzero(free)[0]
            best = cand[np.lexsort((pos[cand], -count[cand]))[0]]      # most unassigned neighbours, then the better key / lower index
            m = adj[best] & free
            cluster_of[m] = len(center)
            free &= ~m
            count -= adj[:, m].sum(1)      # unassigned neighbours of every pose (the assigned ones no longer matter)
            center.append(int(best))
            size.append(int(m.sum()))
    return {"n_clusters": len(center), "center": np.asarray(center, np.int32), "size": np.asarray(size, np.int32),
            "cluster_of": cluster_of}


def cluster_poses(lig_pos, radius, key=None, rule="energy", max_clusters=None, residues=None):
    """The definition end to end: float64 RMSD, neighbours within `radius`, then the rule."""
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and > 0")
    return cluster_adjacency(pose_rmsd(lig_pos, residues) <= radius, key, rule, max_clusters)


def rebuild_backbone(lig_pos0, rot_update, tr_update, family=0):
    """The ligand backbone [B, L, 3, 3] float32 of trajectories with final (rot_update, tr_update) [B, 3], rebuilt in float64 from the
    input backbone lig_pos0 [L, 3, 3] about the centre the sampler rotates about (CA centroid for family 0, backbone centroid for family 1):
    x = (x0 - c) R(rot_update)^T + c + tr_update - the composition of every step of modify_coords (src/inference_base.py:342-352)."""
    from .pdbio import axis_angle_to_matrix
    x0 = np.asarray(lig_pos0, np.float32).reshape(-1, 3, 3).astype(np.float64)
    c = x0.reshape(-1, 3).mean(0) if family == 1 else x0[:, 1].mean(0)
    rot, tr = np.asarray(rot_update, np.float64).reshape(-1, 3), np.asarray(tr_update, np.float64).reshape(-1, 3)
    out = np.empty((rot.shape[0],) + x0.shape, np.float32)
    for b in range(rot.shape[0]):
        out[b] = ((x0 - c) @ axis_angle_to_matrix(rot[b]).T + c + tr[b]).astype(np.float32)
    return out


def satisfied_key(energy, n_satisfied):
    """Key of the "satisfied, then energy" rule of restraint ranking: rank positions of (most groups satisfied, lower energy, lower index),
    so that the first pose in key order is the one restraints.rank_key keeps."""
    e, s = np.asarray(energy, np.float64).reshape(-1), np.asarray(n_satisfied, np.int64).reshape(-1)
    order = np.lexsort((np.arange(e.size), e, -s))
    key = np.empty(e.size, np.float32)
    key[order] = np.arange(e.size, dtype=np.float32)
    return key
