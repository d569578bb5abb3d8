"""Consensus contact scoring (host side): the float64 numpy definition the GPU kernels of dfm_pose_consensus are tested against, the
host finish the definition and the engine wrapper share, the ranking key of the drivers and the consensus contacts as restraints.

Definition (include/dfmdock_amd.h: dfm_pose_consensus).  Receptor backbone rec_pos [R, 9] (N, CA, C per residue, the sampler's layout;
the same in every pose), ligand poses lig_pos [P, L, 9], a cutoff (Angstrom, 5.5: the contact cutoff of metrics.py and
dfm_native_create), members [P] bool (default: every pose; M = number of members >= 1).  Coordinates and the cutoff are taken as float32
and widened to float64.

    d(p,i,j)   = min over the 9 backbone-atom pairs of sqrt((dx*dx + dy*dy) + dz*dz)      (the arithmetic of metrics._min_dist)
    c(p,i,j)   = d(p,i,j) < cutoff                                  (strict; NaN is no contact and disturbs no other pose)
    count[i,j] = number of MEMBER poses with c(p,i,j);  freq = count / M
    rec_count[i] / lig_count[j] = number of member poses in which the residue has at least one contact
    per pose, member or not:  n_contacts[p] = number of contacts,  score_sum[p] = sum of count[i,j] over the contacts of p
    consensus[p] = score_sum[p] / (M n_contacts[p]),  NaN when the pose has no contact                        (`finish`)

Ranking: key -consensus under cluster.rank_order (higher consensus first, ties to the lower index, NaN last).  This is CONSRANK's
score: the mean frequency, in the ensemble, of the contacts of a model (a member's own contacts are part of the frequencies).
"""
from __future__ import annotations

import numpy as np

from .restraints import RestraintGroup

CUTOFF = 5.5
MAX_POSES = 65536


def _inputs(rec_pos, lig_pos):
    rec = np.asarray(rec_pos, np.float32).reshape(-1, 9)
    lig = np.asarray(lig_pos, np.float32)
    if lig.ndim == 4:
        lig = lig.reshape(lig.shape[0], lig.shape[1], 9)
    if lig.ndim != 3 or lig.shape[2] != 9 or lig.shape[0] < 1 or lig.shape[1] < 1 or rec.shape[0] < 1:
        raise ValueError(f"lig_pos must be [P, L, 9] or [P, L, 3, 3] with P, L >= 1 and rec_pos [R, 9] with R >= 1, got "
                         f"{np.shape(lig_pos)} and {np.shape(rec_pos)}")
    return rec, lig


def check_cutoff(cutoff):
    c = float(np.float32(cutoff))
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"cutoff must be finite and > 0, got {cutoff}")
    return c


def check_members(members, P):
    """members as bool [P] (None: every pose); raises ValueError when no pose is a member."""
    m = np.ones(P, bool) if members is None else np.asarray(members).reshape(-1).astype(bool)
    if m.size != P:
        raise ValueError(f"members must have {P} entries, got {m.size}")
    if not m.any():
        raise ValueError("members: no pose is a member")
    return m


def min_dist(rec_pos, lig_pose):
    """[R, L] float64: d(i,j) of ONE pose, rec_pos [R, 9], lig_pose [L, 9]."""
    a = np.asarray(rec_pos, np.float32).reshape(-1, 3, 3).astype(np.float64)
    b = np.asarray(lig_pose, np.float32).reshape(-1, 3, 3).astype(np.float64)
    best = None
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(3):
            for t in range(3):
                dx = a[:, None, s, 0] - b[None, :, t, 0]
                dy = a[:, None, s, 1] - b[None, :, t, 1]
                dz = a[:, None, s, 2] - b[None, :, t, 2]
                d = np.sqrt((dx * dx + dy * dy) + dz * dz)
                best = d if best is None else np.minimum(best, d)      # np.minimum propagates NaN, like numpy's min
    return best


def contacts(rec_pos, lig_pos, cutoff=CUTOFF):
    """bool [P, R, L]: c(p,i,j)."""
    rec, lig = _inputs(rec_pos, lig_pos)
    cut = check_cutoff(cutoff)
    out = np.zeros((lig.shape[0], rec.shape[0], lig.shape[1]), bool)
    for p in range(lig.shape[0]):
        with np.errstate(invalid="ignore"):
            out[p] = min_dist(rec, lig[p]) < cut
    return out


def finish(score_sum, n_contacts, M):
    """consensus [P] float64 = score_sum / (M n_contacts), NaN where n_contacts == 0: the host finish shared by the definition and
    engine.Model.consensus."""
    s, n = np.asarray(score_sum, np.int64).reshape(-1), np.asarray(n_contacts, np.int64).reshape(-1)
    out = np.full(s.size, np.nan, np.float64)
    has = n > 0
    out[has] = s[has].astype(np.float64) / (float(int(M)) * n[has].astype(np.float64))
    return out


def from_contacts(c, members=None):
    """The definition's formulas on given contacts c bool [P, R, L]: {count, rec_count, lig_count (int32), n_contacts (int32 [P]),
    score_sum (int64 [P]), M, freq, consensus}."""
    c = np.asarray(c, bool)
    m = check_members(members, c.shape[0])
    M = int(m.sum())
    cm = c[m]
    count = cm.sum(0, dtype=np.int64).astype(np.int32)
    n_contacts = c.reshape(c.shape[0], -1).sum(1, dtype=np.int64).astype(np.int32)
    score_sum = np.array([int(count[c[p]].sum(dtype=np.int64)) for p in range(c.shape[0])], np.int64)
    return {"count": count, "rec_count": cm.any(2).sum(0, dtype=np.int64).astype(np.int32),
            "lig_count": cm.any(1).sum(0, dtype=np.int64).astype(np.int32), "n_contacts": n_contacts, "score_sum": score_sum, "M": M,
            "freq": count.astype(np.float64) / M, "consensus": finish(score_sum, n_contacts, M)}


def consensus(rec_pos, lig_pos, cutoff=CUTOFF, members=None):
    """The definition end to end (float64 numpy): the dict of from_contacts plus `cutoff`."""
    out = from_contacts(contacts(rec_pos, lig_pos, cutoff), members)
    out["cutoff"] = check_cutoff(cutoff)
    return out


def pack_bits(c):
    """bool [P, R, L] -> uint64 [P, R, ceil(L / 64)]: bit j % 64 of word j / 64 = c[p, i, j] (the layout of dfm_consensus_out.bits)."""
    c = np.asarray(c, bool)
    P, R, L = c.shape
    W = (L + 63) // 64
    pad = np.zeros((P, R, W * 64), np.uint8)
    pad[:, :, :L] = c
    by = np.packbits(pad.reshape(P, R, W, 8, 8), axis=-1, bitorder="little").reshape(P, R, W, 8)
    return np.ascontiguousarray(by).view("<u8").reshape(P, R, W).astype(np.uint64)


def unpack_bits(bits, L):
    """uint64 [P, R, W] -> (bool [P, R, L], the number of set bits beyond L, which must be 0)."""
    b = np.ascontiguousarray(np.asarray(bits, np.uint64).astype("<u8"))
    P, R, W = b.shape
    flat = np.unpackbits(b.view(np.uint8).reshape(P, R, W * 8), axis=-1, bitorder="little")
    return flat[:, :, :L].astype(bool), int(flat[:, :, L:].sum())


def energy_members(energy, frac=1.0):
    """members = the best `frac` of the poses by energy (lower first, ties to the lower index, NaN last), at least one."""
    from .cluster import rank_order
    e = np.asarray(energy, np.float64).reshape(-1)
    if not (0.0 < float(frac) <= 1.0):
        raise ValueError(f"the member fraction must be in (0, 1], got {frac}")
    n = max(1, min(e.size, int(np.floor(float(frac) * e.size + 1e-9))))
    m = np.zeros(e.size, bool)
    m[rank_order(e, e.size)[:n]] = True
    return m


def pick(consensus_score, energy):
    """Index of the pose consensus ranking keeps: the highest consensus, ties to the lower energy, then to the lower index.  None when no
    pose has a contact (every score NaN): the caller falls back to the energy."""
    s, e = np.asarray(consensus_score, np.float64).reshape(-1), np.asarray(energy, np.float64).reshape(-1)
    if np.isnan(s).all():
        return None
    return int(rank_positions(s, e).argmin())


def rank_positions(consensus_score, energy):
    """float32 [P]: every pose's position under (higher consensus, lower energy, lower index), NaN consensus last - a key for
    dfm_pose_cluster (lower = better) whose first pose is the one `pick` keeps."""
    s, e = np.asarray(consensus_score, np.float64).reshape(-1), np.asarray(energy, np.float64).reshape(-1)
    nan, enan = np.isnan(s), np.isnan(e)
    order = np.lexsort((np.arange(s.size), np.where(enan, 0.0, e), enan, np.where(nan, 0.0, -s), nan))
    key = np.empty(s.size, np.float32)
    key[order] = np.arange(s.size, dtype=np.float32)
    return key


def top_contacts(count, n, min_count=1):
    """The n residue pairs with the largest count (at least min_count), ties in row-major order of the R x L matrix: int32 [k, 2] =
    (receptor residue, ligand residue), k <= n."""
    c = np.asarray(count)
    if c.ndim != 2:
        raise ValueError("count must be [R, L]")
    flat = c.reshape(-1).astype(np.int64)
    keep = np.nonzero(flat >= max(int(min_count), 1))[0]
    keep = keep[np.argsort(-flat[keep], kind="stable")][: max(int(n), 0)]
    return np.stack([keep // c.shape[1], keep % c.shape[1]], 1).astype(np.int32).reshape(-1, 2)


def contact_groups(count, M, n, upper=8.0, min_count=1):
    """top_contacts as restraints: one pair per group, upper bound `upper` A on the CA-CA distance (what restraints.native_contact_groups
    uses), weight = the contact's frequency count / M."""
    c = np.asarray(count)
    return [RestraintGroup(((int(i), int(j)),), float(upper), float(c[i, j]) / float(M)) for i, j in top_contacts(c, n, min_count)]


def _name(key):
    return f"{key[0]}:{int(key[1])}{key[2] if key[2] != ' ' else ''}"


def format_restraints(groups, rec, lig, header=None):
    """Restraint-file text (the format restraints.parse_restraints reads) of single-pair or multi-pair groups; rec / lig are
    pdbio.backbone_from_atoms dicts.  Pairs of a group must form a product set (receptor residues x ligand residues), which is what the
    format can say; weights are written with repr precision so that write -> parse gives back the same groups."""
    lines = [] if header is None else ["# " + h for h in str(header).splitlines()]
    for g in groups:
        ri, li = list(dict.fromkeys(i for i, _ in g.pairs)), list(dict.fromkeys(j for _, j in g.pairs))
        if tuple((i, j) for i in ri for j in li) != tuple(g.pairs):
            raise ValueError("a restraint group must pair every listed receptor residue with every listed ligand residue to be written")
        lines.append(f"{','.join(_name(rec['residues'][i]) for i in ri)} {','.join(_name(lig['residues'][j]) for j in li)} "
                     f"{float(g.upper)!r} {float(g.weight)!r}")
    return "\n".join(lines) + "\n"


def write_restraints(path, groups, rec, lig, header=None):
    with open(path, "w") as f:
        f.write(format_restraints(groups, rec, lig, header))
