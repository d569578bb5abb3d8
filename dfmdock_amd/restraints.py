"""Interface distance restraints (host side): the restraint type, its packing into the arrays of dfm_complex_set_restraints, the float64
numpy definition the GPU kernel is tested against, the restraint-file parser and native-contact restraints for benchmarks.

Definition (include/dfmdock_amd.h: dfm_complex_set_restraints).  Group g = residue pairs P_g of (receptor i, ligand j), upper bound
u_g > 0 (Angstrom), weight w_g >= 0.  With receptor CA y_i and ligand CA x_j of one pose:

    d_g = min over P_g of |x_j - y_i|      (arg-min (i*, j*): the first minimal pair in list order)
    v_g = max(0, d_g - u_g),   U = sum_g w_g v_g^2,   grad_g = 2 w_g v_g (x_j* - y_i*) / d_g   (on x_j* only)
    F = -sum_g grad_g,   T = sum_g (x_j* - c) x (-grad_g)      (c: the centroid the sampler rotates about)
    dtau = clip(k_tr F, max_tr),   domega = clip(k_rot T, max_rot),   clip(v, m) = v min(1, m / |v|)

and the step moves the ligand as the Euler-Maruyama step does (inference_base.py:453-456): X <- (X - c) R(domega)^T + c + dtau,
rot_update <- axis_angle(R(domega) R(rot_update)), tr_update <- tr_update + dtau.

Restraint file: one group per line, `REC_RESIDUES  LIG_RESIDUES  UPPER [WEIGHT]`; residues as `chain:resnum[icode]`, comma lists and
ranges `A:100-A:105` (every residue of the structure from the first to the second, in file order); `#` starts a comment.
"""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class RestraintGroup:
    """One (possibly ambiguous) distance restraint: some pair of `pairs` (receptor index, ligand index) within `upper` Angstrom."""
    pairs: tuple
    upper: float
    weight: float = 1.0

    def __post_init__(self):
        object.__setattr__(self, "pairs", tuple((int(i), int(j)) for i, j in self.pairs))


@dataclass(frozen=True)
class RestraintParams:
    """dfm_restraint_params.  Defaults: DESIGN.md "Interface restraints"."""
    k_tr: float = 0.25      # Angstrom per unit force (U in Angstrom^2: force in Angstrom)
    k_rot: float = 3e-3     # rad per unit torque
    max_tr: float = 10.0    # Angstrom per step
    max_rot: float = 0.3    # rad per step
    t_start: float = 1.0    # the step runs when t_i <= t_start

    def to_c(self):
        from ._lib import RestraintParamsC
        return RestraintParamsC(self.k_tr, self.k_rot, self.max_tr, self.max_rot, self.t_start)


def pack(groups, R=None, L=None):
    """Groups -> (group_start int32 [G+1], pairs int32 [P,2], upper float32 [G], weight float32 [G]), the arrays of
    dfm_complex_set_restraints.  Checks what the C entry point checks (with the group's index in the message)."""
    groups = list(groups)
    gs = np.zeros(len(groups) + 1, np.int32)
    pairs, up, w = [], np.zeros(len(groups), np.float32), np.zeros(len(groups), np.float32)
    for g, grp in enumerate(groups):
        if not grp.pairs:
            raise ValueError(f"restraint group {g} has no residue pair")
        if not (grp.upper > 0 and np.isfinite(grp.upper)):
            raise ValueError(f"restraint group {g}: upper bound must be > 0, got {grp.upper}")
        if not (grp.weight >= 0 and np.isfinite(grp.weight)):
            raise ValueError(f"restraint group {g}: weight must be >= 0, got {grp.weight}")
        for i, j in grp.pairs:
            if (R is not None and not 0 <= i < R) or (L is not None and not 0 <= j < L):
                raise ValueError(f"restraint group {g}: pair ({i}, {j}) outside the complex (R = {R}, L = {L})")
        pairs += grp.pairs
        gs[g + 1] = len(pairs)
        up[g], w[g] = grp.upper, grp.weight
    return gs, np.asarray(pairs, np.int32).reshape(-1, 2), up, w


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference
def _centroid(lig, center):
    lig = np.asarray(lig, np.float64)
    return lig.reshape(-1, 3).mean(0) if center == "all_atoms" else lig[:, 1].mean(0)


def _clip(v, m):
    n = float(np.linalg.norm(v))
    return v * min(1.0, m / n) if n > 0 else v


def evaluate(groups, rec_pos, lig_pos, params: RestraintParams | None = None, center="ca"):
    """U, the number of satisfied groups (v_g = 0), force F, torque T and the step (dtau, domega) at ONE pose (lig_pos [L,3,3]);
    float64 throughout.  center: "ca" (first family) or "all_atoms" (second family) - the centroid the sampler rotates about."""
    p = params or RestraintParams()
    y = np.asarray(rec_pos, np.float64).reshape(-1, 3, 3)[:, 1]
    lig = np.asarray(lig_pos, np.float64).reshape(-1, 3, 3)
    x = lig[:, 1]
    c = _centroid(lig, center)
    U, n_sat = 0.0, 0
    F, T = np.zeros(3), np.zeros(3)
    d_all, arg_all = [], []
    for grp in groups:
        pr = np.asarray(grp.pairs, np.int64).reshape(-1, 2)
        diff = x[pr[:, 1]] - y[pr[:, 0]]
        d2 = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
        k = int(np.argmin(d2))      # first minimal pair; a NaN distance wins (the first one): the group's d, U and the step are then NaN
        d = float(np.sqrt(d2[k]))
        d_all.append(d)
        arg_all.append(k)
        v = d - grp.upper
        if v <= 0:
            n_sat += 1
            continue
        U += grp.weight * v * v
        if grp.weight == 0:
            continue
        f = -2.0 * grp.weight * v * diff[k] / d
        F += f
        T += np.cross(x[pr[k, 1]] - c, f)
    step = np.concatenate([_clip(p.k_tr * F, p.max_tr), _clip(p.k_rot * T, p.max_rot)])
    return {"energy": U, "n_satisfied": n_sat, "force": F, "torque": T, "step": step, "d": np.asarray(d_all), "arg": np.asarray(arg_all)}


def energy(groups, rec_pos, lig_pos):
    return evaluate(groups, rec_pos, lig_pos)["energy"]


def axis_angle_to_matrix(aa):
    aa = np.asarray(aa, np.float64).reshape(3)
    ang = np.linalg.norm(aa)
    if ang < 1e-12:
        return np.eye(3)
    k = aa / ang
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def matrix_to_axis_angle(Rm):
    """Axis-angle of a rotation matrix (angle in [0, pi]) via the quaternion of the largest diagonal term."""
    m = np.asarray(Rm, np.float64)
    tr = np.trace(m)
    cand = [1 + tr, 1 + 2 * m[0, 0] - tr, 1 + 2 * m[1, 1] - tr, 1 + 2 * m[2, 2] - tr]
    b = int(np.argmax(cand))
    s = 2.0 * np.sqrt(cand[b])
    if b == 0:
        q = [s / 4, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    elif b == 1:
        q = [(m[2, 1] - m[1, 2]) / s, s / 4, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
    elif b == 2:
        q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, s / 4, (m[1, 2] + m[2, 1]) / s]
    else:
        q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, s / 4]
    q = np.asarray(q)
    if q[0] < 0:
        q = -q
    n = np.linalg.norm(q[1:])
    if n < 1e-15:
        return 2.0 * q[1:]
    return q[1:] / n * (2.0 * np.arctan2(n, q[0]))


def rot_compose(r1, r2):
    """inference_base.py:311-316: axis_angle(R(r2) @ R(r1))."""
    return matrix_to_axis_angle(axis_angle_to_matrix(r2) @ axis_angle_to_matrix(r1))


def apply_step(lig_pos, step, rot_update=None, tr_update=None, center="ca"):
    """The rigid move of a step (dtau, domega) about the sampler's centroid, float64: returns (pose, rot_update, tr_update)."""
    lig = np.asarray(lig_pos, np.float64).reshape(-1, 3, 3)
    step = np.asarray(step, np.float64).reshape(6)
    c = _centroid(lig, center)
    new = (lig - c) @ axis_angle_to_matrix(step[3:]).T + c + step[:3]
    ru = None if rot_update is None else rot_compose(np.asarray(rot_update, np.float64), step[3:])
    tu = None if tr_update is None else np.asarray(tr_update, np.float64) + step[:3]
    return new, ru, tu


def replay_pose(lig0, rot_update, tr_update, center="ca"):
    """The pose (rot_update, tr_update) describe, from the complex's start pose lig0 (modify_aa_coords, inference_base.py:354-364)."""
    lig0 = np.asarray(lig0, np.float64).reshape(-1, 3, 3)
    c = _centroid(lig0, center)
    return (lig0 - c) @ axis_angle_to_matrix(rot_update).T + c + np.asarray(tr_update, np.float64).reshape(3)


# ---------------------------------------------------------------------------------------------------------------------------------
# restraint files
_RES = re.compile(r"^([A-Za-z0-9]):(-?\d+)([A-Za-z]?)$")


def _residue_index(bb):
    return {(k[0], int(k[1]), (k[2] if k[2] != " " else "")): n for n, k in enumerate(bb["residues"])}


def _incomplete(bb):
    """Residues of the structure (ATOM records) that backbone_from_atoms dropped: no complete N, CA, C backbone."""
    kept = {(k[0], int(k[1]), (k[2] if k[2] != " " else "")) for k in bb["residues"]}
    return {(a["chain"], int(a["res_id"]), (a["ins"] if a["ins"] != " " else "")) for a in bb["atoms"]} - kept


def _spec_name(key):
    return f"{key[0]}:{key[1]}{key[2]}"


def _parse_residue(tok, idx, bad, side, lineno):
    m = _RES.match(tok)
    if not m:
        raise ValueError(f"restraints line {lineno}: cannot read {side} residue {tok!r} (expected chain:resnum[icode])")
    key = (m.group(1), int(m.group(2)), m.group(3))
    if key in idx:
        return idx[key]
    why = "has no complete backbone (N, CA, C)" if key in bad else "is not in the structure"
    raise ValueError(f"restraints line {lineno}: {side} residue {_spec_name(key)} {why}")


def _parse_set(field, bb, side, lineno):
    idx, bad = _residue_index(bb), _incomplete(bb)
    out = []
    for item in field.split(","):
        item = item.strip()
        if not item:
            continue
        m = re.match(r"^(\S+?:-?\d+[A-Za-z]?)-(\S+:-?\d+[A-Za-z]?)$", item)
        if m:
            a = _parse_residue(m.group(1), idx, bad, side, lineno)
            b = _parse_residue(m.group(2), idx, bad, side, lineno)
            if b < a or bb["residues"][a][0] != bb["residues"][b][0]:
                raise ValueError(f"restraints line {lineno}: {side} range {item!r} must run forward within one chain")
            out += list(range(a, b + 1))
        else:
            out.append(_parse_residue(item, idx, bad, side, lineno))
    if not out:
        raise ValueError(f"restraints line {lineno}: no {side} residue")
    return list(dict.fromkeys(out))      # each residue once, first mention order


def parse_restraints(text, rec, lig):
    """Restraint-file text -> [RestraintGroup].  rec / lig: pdbio.backbone_from_atoms dicts (indices follow their `residues`).
    Pairs of a group run receptor-major in the order the residues are written."""
    groups = []
    for lineno, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        if not line:
            continue
        f = line.split()
        if len(f) not in (3, 4):
            raise ValueError(f"restraints line {lineno}: expected REC_RESIDUES LIG_RESIDUES UPPER [WEIGHT], got {raw.strip()!r}")
        ri = _parse_set(f[0], rec, "receptor", lineno)
        li = _parse_set(f[1], lig, "ligand", lineno)
        try:
            upper = float(f[2])
            weight = float(f[3]) if len(f) == 4 else 1.0
        except ValueError:
            raise ValueError(f"restraints line {lineno}: UPPER / WEIGHT must be numbers, got {f[2:]}") from None
        if not (upper > 0 and np.isfinite(upper)):
            raise ValueError(f"restraints line {lineno}: upper bound must be > 0, got {f[2]}")
        if not (weight >= 0 and np.isfinite(weight)):
            raise ValueError(f"restraints line {lineno}: weight must be >= 0, got {f[3]}")
        groups.append(RestraintGroup(tuple((i, j) for i in ri for j in li), upper, weight))
    return groups


def read_restraints(path, rec, lig):
    with open(path) as fh:
        return parse_restraints(fh.read(), rec, lig)


def native_contact_groups(rec_pos, lig_pos, k, cutoff=8.0, seed=0):
    """k seeded single-pair restraints (u = cutoff) on CA-CA contacts closer than `cutoff` in the native pose - the usual way to
    evaluate guided docking.  Fewer contacts than k: all of them.  Pairs in (receptor, ligand) order."""
    y = np.asarray(rec_pos, np.float64).reshape(-1, 3, 3)[:, 1]
    x = np.asarray(lig_pos, np.float64).reshape(-1, 3, 3)[:, 1]
    d = np.sqrt(((y[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    ii, jj = np.nonzero(d < cutoff)
    if len(ii) == 0:
        return []
    pick = np.sort(np.random.default_rng(seed).choice(len(ii), size=min(int(k), len(ii)), replace=False))
    return [RestraintGroup(((int(ii[q]), int(jj[q])),), float(cutoff)) for q in pick]


def rank_key(energy, n_satisfied):
    """Index of the kept trajectory under the "satisfied, then energy" rule: the minimum energy among those satisfying the most
    groups (the first such, as the reference keeps the first minimum)."""
    energy, n_satisfied = np.asarray(energy), np.asarray(n_satisfied)
    cand = np.nonzero(n_satisfied == n_satisfied.max())[0]
    return int(cand[np.argmin(energy[cand])])
