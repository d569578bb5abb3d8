#!/usr/bin/env python3
"""Generate tests/golden/igso3_ref.npz by RUNNING THE REFERENCE's forward process (local refinement, dfmdock_amd/refine.py).

The reference is imported unmodified (utils/so3_diffuser.py, utils/r3_diffuser.py, models/score_model_mlsb.py::modify_coords) with
the stand-ins of make_golden.py for the third-party modules that are absent; the checkout is looked for where make_golden.py looks
for it (DFMDOCK_REFERENCE overrides).  The SO3Diffuser constructor builds its 1000 x 1000 tables in a temporary cache directory
(about a minute).

For t in T: sigma_idx, the grid sigma, the 1000-entry cdf (float64), the angles SO3Diffuser.sample_igso3 returns for 64 recorded
uniforms, and for the syn_24_16 complex the reference's own noising: forward_marginal of both diffusers under a seeded np.random
(draws recorded by replaying the seed), pose after modify_coords.

Usage:  python tests/golden/make_golden_igso3.py
"""
import os
import sys
import tempfile
import types
from types import SimpleNamespace as NS
from unittest.mock import MagicMock

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DFMDOCK_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "src"))

T = (0.001, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 1.0)
N_U = 64
U_LO, U_HI = 0.01, 0.99      # the recorded uniforms: inside the strictly increasing part of every table (asserted below)
PDF_MIN = 1e-3               # ... and where the density is at least this (tests/test_gpu_refine.py derives its cdf bound from it)


def install_stubs():
    """make_golden.py's stand-ins; nothing of them is on the path this script records."""
    tg = types.ModuleType("torch_geometric")
    tgnn = types.ModuleType("torch_geometric.nn")
    tgn = types.ModuleType("torch_geometric.nn.norm")
    tgl = types.ModuleType("torch_geometric.loader")
    tgn.GraphNorm = type("GraphNorm", (nn.Module,), {})
    tgl.DataLoader = object
    tgd = types.ModuleType("torch_geometric.data")
    tgd.HeteroData = type("HeteroData", (), {})
    tg.data, tgnn.norm, tg.nn, tg.loader = tgd, tgn, tgnn, tgl
    sys.modules.update({"torch_geometric": tg, "torch_geometric.nn": tgnn, "torch_geometric.nn.norm": tgn,
                        "torch_geometric.loader": tgl, "torch_geometric.data": tgd})
    for name in ["esm", "biotite", "biotite.structure", "biotite.structure.io", "biotite.structure.io.pdb", "tree", "hydra",
                 "omegaconf", "wandb"]:
        sys.modules.setdefault(name, MagicMock())
    sys.modules["hydra"].main = lambda **kw: (lambda f: f)
    pl = types.ModuleType("pytorch_lightning")

    class LightningModule(nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass

    pl.LightningModule = LightningModule
    pl.LightningDataModule = object
    sys.modules["pytorch_lightning"] = pl


def main():
    install_stubs()
    from utils.so3_diffuser import SO3Diffuser
    from utils.r3_diffuser import R3Diffuser
    from models.score_model_mlsb import Score_Model
    from dfmdock_amd.synthetic import make_complex

    # configs/model/score_model_mlsb.yaml:15-26
    r3 = R3Diffuser(NS(min_sigma=0.1, max_sigma=30.0, schedule="VE"))
    with tempfile.TemporaryDirectory() as cache:
        so3 = SO3Diffuser(NS(num_omega=1000, num_sigma=1000, min_sigma=0.1, max_sigma=1.5, schedule="logarithmic",
                             cache_dir=cache, use_cached_score=False))
    cx = make_complex(24, 16, seed=5)      # syn_24_16 (tests/conftest.py: complex_for)
    lig = torch.from_numpy(cx["lig_pos"])
    out = {"t": np.asarray(T, np.float64), "omega": so3.discrete_omega.astype(np.float64), "lig_pos": cx["lig_pos"]}
    for n, t in enumerate(T):
        idx = int(so3.t_to_idx(t))
        cdf, pdf = so3._cdf[idx], so3._pdf[idx]
        # sample_igso3 draws its uniforms itself: run it under a seed, replay the seed to record them, keep the first N_U in range
        np.random.seed(1000 + n)
        ang = so3.sample_igso3(t, n_samples=4 * N_U)
        np.random.seed(1000 + n)
        u = np.random.rand(4 * N_U)
        keep = np.nonzero((u >= U_LO) & (u <= U_HI))[0][:N_U]
        assert keep.size == N_U
        u, ang = u[keep], ang[keep]
        k_hi = int(np.searchsorted(cdf, U_HI)) + 1
        assert cdf[0] < U_LO and cdf[-1] > U_HI and np.all(np.diff(cdf[: k_hi + 1]) > 0), f"t={t}: recorded uniforms leave the monotone part"
        assert np.all(np.interp(ang, so3.discrete_omega, pdf) >= PDF_MIN), f"t={t}: a recorded angle lies where pdf < {PDF_MIN}"
        # the reference's training-step noising (score_model_mlsb.py:65-94): translation first, then rotation
        seed = 2000 + n
        while True:
            np.random.seed(seed)
            z = np.random.randn(1, 3)
            axis = np.random.randn(1, 3)
            u1 = np.random.rand(1)
            if U_LO <= u1[0] <= U_HI:
                break
            seed += 100
        np.random.seed(seed)
        tr_t, _ = r3.forward_marginal(t)
        rot_t, _ = so3.forward_marginal(t)
        tr_u, rot_u = torch.from_numpy(tr_t).float(), torch.from_numpy(rot_t).float()
        pose = Score_Model.modify_coords(None, lig, rot_u, tr_u).numpy()
        k = f"t{n}/"
        out.update({k + "sigma_idx": np.int64(idx), k + "sigma": np.float64(so3.discrete_sigma[idx]), k + "cdf": cdf.astype(np.float64),
                    k + "u": u, k + "angle": ang.astype(np.float64), k + "fm_seed": np.int64(seed), k + "fm_z": z[0], k + "fm_axis": axis[0],
                    k + "fm_u": np.float64(u1[0]), k + "fm_rot": rot_t.reshape(3).astype(np.float64), k + "fm_tr": tr_t.reshape(3).astype(np.float64),
                    k + "fm_pose": pose.astype(np.float32), k + "sigma_r3": np.float64(r3.sigma(t))})
        print(f"t={t}: idx {idx} sigma {so3.discrete_sigma[idx]:.6f} cdf[-1] {cdf[-1]:.12f} min pdf {pdf.min():.2e} "
              f"first non-increasing k {int(np.argmax(np.diff(cdf) <= 0)) if np.any(np.diff(cdf) <= 0) else -1} |rot| {np.linalg.norm(rot_t):.4f}")
    path = os.path.join(HERE, "igso3_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
