#!/usr/bin/env python3
"""Reference numbers for the distogram reductions (dfmdock_amd/distogram.py) by RUNNING THE REFERENCE's own loss:
``distogram_loss(logits, dists)`` (src/utils/loss.py:65-93) and a torch softmax on the reference's dist_logits committed in
fwd2_dist.npz (make_golden_pair.py dist): syn_24_16 whole, 7CEI pose 1 on its stride-8 residue grid, each at the CA-CA distances
of its own pose.

Same rules as make_golden_pair.py: runs only in the build container; only distogram_ref.npz (recorded numbers) travels.

Usage:  python tests/golden/make_golden_distogram.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on sys.path)

from utils.loss import distogram_loss  # noqa: E402

from conftest import complex_for, load_golden  # noqa: E402

CONTACT_BINS = 7
CASES = (("fwd2_syn_24_16", "syn_24_16", 1), ("fwd2_7CEI_p1", "cei_p1_stride8", 8))


def case_distances(case, stride):
    """CA-CA distances [R,L] of the golden case's pose (float64), on the stride grid of its logits."""
    g, cx = load_golden(case + ".npz"), complex_for(case)
    rc = cx["rec_pos"][:, 1].astype(np.float64)
    lc = g["lig_pos"][:, 1].astype(np.float64)
    return np.sqrt(((rc[:, None] - lc[None]) ** 2).sum(-1))[::stride, ::stride]


def main():
    logits = load_golden("fwd2_dist.npz")
    out = {"contact_bins": np.int64(CONTACT_BINS)}
    for case, key, stride in CASES:
        z = torch.from_numpy(logits[key].astype(np.float64))
        D = torch.from_numpy(case_distances(case, stride))
        assert z.shape[:2] == D.shape
        out[key + "_nll"] = np.float64(distogram_loss(z, D[..., None]).item())
        p = torch.softmax(z, -1)
        pc = p[..., :CONTACT_BINS].sum(-1).numpy()
        out[key + "_pcontact_range"] = np.array([pc.min(), pc.max()])
        out[key + "_pcontact_4x4"] = pc[:4, :4].copy()
        # per-pair loss of the same corner, one pair at a time through the same function
        out[key + "_pair_nll_4x4"] = np.array([[distogram_loss(z[i, j][None], D[i, j].reshape(1, 1)).item() for j in range(4)] for i in range(4)])
        print(key, out[key + "_nll"], out[key + "_pcontact_range"])
    mg.save("distogram_ref.npz", **out)


if __name__ == "__main__":
    main()
