"""The distogram head's reductions, in float64 numpy: the definition `Complex.distogram` (dfm_score_distogram) is tested against.

The second model family predicts, for every receptor / ligand residue pair, the native CA-CA distance in 64 bins (EGNN_Net.to_dist,
egnn_net.py:347-352,:447).  Three reductions over the bins make that prediction usable after sampling:

  nll       -log_softmax(z)[bin(D)] with D the POSE's own CA-CA distance: averaged over all pairs it is the reference's
            ``distogram_loss(dist_logits, D)`` (utils/loss.py:65-93) - how well the pose agrees with what the model predicts at it
  pcontact  the probability mass of the first `contact_bins` bins (7: d <= 7.85 A)
  edist     the expected distance, sum_k p_k centre_k

bins: bounds = linspace(3.25, 50.75, 63), bin(d) = #{k : d^2 > bounds[k]^2} in 0..63, centre[k] = 3.25 + (k - 0.5) step.
"""
from __future__ import annotations

import numpy as np

N_BINS = 64
MIN_BIN, MAX_BIN = 3.25, 50.75
BOUNDS = np.linspace(MIN_BIN, MAX_BIN, N_BINS - 1)
STEP = (MAX_BIN - MIN_BIN) / (N_BINS - 2)
CENTRES = MIN_BIN + (np.arange(N_BINS) - 0.5) * STEP


def bin_of(d):
    """bin(d) = #{k : d^2 > bounds[k]^2}, elementwise; d = 3.25 is bin 0, anything above 50.75 is bin 63."""
    d = np.asarray(d, np.float64)
    return (d[..., None] ** 2 > BOUNDS ** 2).sum(-1)


def log_softmax(z):
    z = np.asarray(z, np.float64)
    zs = z - z.max(-1, keepdims=True)
    return zs - np.log(np.exp(zs).sum(-1, keepdims=True))


def ca_distances(rec_pos, lig_pos):
    """D [R,L] (or [B,R,L] for lig_pos [B,L,3,3]) between the CA atoms (atom 1) of the receptor and of the ligand pose(s)."""
    rc = np.asarray(rec_pos, np.float64)[:, 1]
    lc = np.asarray(lig_pos, np.float64)[..., 1, :]
    return np.sqrt(((rc[:, None, :] - lc[..., None, :, :]) ** 2).sum(-1))


def pair_maps(logits, D, contact_bins=7):
    """Per-pair reductions of logits [...,64] at distances D [...]: {pair_nll, pcontact, edist}."""
    if not 1 <= int(contact_bins) <= N_BINS - 1:
        raise ValueError("contact_bins must be in 1..63")
    logp = log_softmax(logits)
    p = np.exp(logp)
    b = bin_of(D)
    return dict(pair_nll=-np.take_along_axis(logp, b[..., None], -1)[..., 0], pcontact=p[..., :int(contact_bins)].sum(-1),
                edist=(p * CENTRES).sum(-1))


def pose_scores(logits, D, contact_bins=7, near_cutoff=12.0):
    """One pose: logits [R,L,64], D [R,L] -> the maps of pair_maps plus nll (mean over all pairs: the reference's distogram_loss),
    nll_near / n_near (mean / count over D < near_cutoff; NaN without any) and exp_contacts (sum of pcontact)."""
    m = pair_maps(logits, D, contact_bins)
    near = np.asarray(D, np.float64) < float(near_cutoff)
    n = int(near.sum())
    m.update(nll=float(m["pair_nll"].mean()), n_near=n, nll_near=float(m["pair_nll"][near].sum() / n) if n else float("nan"),
             exp_contacts=float(m["pcontact"].sum()))
    return m


def pcontact_mean(pcontact):
    """Mean over the B poses of pcontact [B,R,L], added in index order in double."""
    pc = np.asarray(pcontact, np.float64)
    s = np.zeros(pc.shape[1:], np.float64)
    for b in range(pc.shape[0]):
        s += pc[b]
    return s / pc.shape[0]


def top_contacts(pmean, n):
    """The n most probable pairs of pmean [R,L] as [(r, l, p)], highest first; ties go to the lower (r, l)."""
    pm = np.asarray(pmean, np.float64)
    if pm.ndim != 2:
        raise ValueError("pmean must be [R,L]")
    n = max(0, min(int(n), pm.size))
    order = np.argsort(-pm.ravel(), kind="stable")[:n]      # stable: equal values keep the row-major (r, l) order
    return [(int(q // pm.shape[1]), int(q % pm.shape[1]), float(pm.ravel()[q])) for q in order]


def contact_groups(pmean, n, upper=8.0):
    """top_contacts as restraints (what consensus.write_restraints writes and restraints.parse_restraints reads): one pair per group,
    upper bound `upper` A on the CA-CA distance, weight = the predicted contact probability."""
    from .restraints import RestraintGroup
    return [RestraintGroup(((r, l),), float(upper), p) for r, l, p in top_contacts(pmean, n)]
