"""Local refinement (host side): the float64 numpy definition of the forward process that dfm_refine starts from, which the kernels
k_igso3_cdf / k_start_pose (csrc/kernels_geom.hip) are tested against.

Partial diffusion: a pose the caller already has is noised with the reference's forward process up to a time t_begin < 1 and the reverse
SDE of dfm_sample runs from there over linspace(t_begin, eps, num_steps).  The forward process is what the reference's training step
applies (src/models/score_model_mlsb.py:65-94): R3Diffuser.forward_marginal (r3_diffuser.py:33-39), SO3Diffuser.forward_marginal ->
sample -> sample_igso3 (so3_diffuser.py:232-343), then modify_coords.

  sigma grid    discrete_sigma = sigma_so3(linspace(0, 1, 1000)); the reference samples at the grid value BELOW sigma_so3(t):
                idx = digitize(sigma_so3(t), discrete_sigma) - 1                                          (so3_diffuser.py:199-206,:228)
  table         omega_k = k pi / 1000, k = 1..1000; expansion(omega) = sum_{l<1000} (2l+1) exp(-l(l+1) sigma^2 / 2) sin((l+1/2) omega)
                / sin(omega / 2); pdf = expansion (1 - cos omega) / pi; cdf = cumsum(pdf) pi / 1000        (:24-85,:165-177)
  inverse       angle(u): k = the first index with cdf[k] >= u; k = 0 -> omega_1; none -> pi; otherwise linear between
                (cdf[k-1], omega_{k-1}) and (cdf[k], omega_k).  Equal to the reference's np.interp(u, cdf, omega) wherever the table is
                strictly increasing; at small sigma its tail is not (rounding noise of a pdf that is 0 there), where np.interp is undefined.
  pose          rotation vector = normalised N(0, I) draw x angle; translation = sigma_r3(t) z, z ~ N(0, I); applied as modify_coords
                applies a step: x = (x - c) R^T + c + tr about the ligand CA centroid (family 1: the centroid of all backbone atoms).
  time grid     linspace(t_begin, eps, num_steps) in float32 by dfm_sample's two-sided formula; t_begin = 1 gives dfm_sample's grid.
"""
from __future__ import annotations

import numpy as np

from .weights import HParams

NUM_SIGMA = 1000      # configs/model/score_model_mlsb.yaml:21-22
NUM_OMEGA = 1000
L_TRUNC = 1000        # igso3_expansion's default L

OMEGA = np.linspace(0.0, np.pi, NUM_OMEGA + 1)[1:]


def so3_sigma(t, hp: HParams | None = None):
    hp = hp or HParams()
    t = np.asarray(t, np.float64)
    if np.any(t < 0) or np.any(t > 1) or np.any(np.isnan(t)):
        raise ValueError(f"Invalid t={t}")
    return np.log(t * np.exp(hp.so3_max_sigma) + (1 - t) * np.exp(hp.so3_min_sigma))


def r3_sigma(t, hp: HParams | None = None):
    hp = hp or HParams()
    return hp.r3_min_sigma * (hp.r3_max_sigma / hp.r3_min_sigma) ** np.float64(t)


def discrete_sigma(hp: HParams | None = None):
    return so3_sigma(np.linspace(0.0, 1.0, NUM_SIGMA), hp)


def sigma_index(t, hp: HParams | None = None):
    """(idx, discrete_sigma[idx]): the grid value the reference's tables are looked up at for time t."""
    ds = discrete_sigma(hp)
    idx = int(np.digitize(so3_sigma(float(t), hp), ds) - 1)
    return idx, float(ds[idx])


def igso3_cdf(sigma):
    """The 1000-entry cdf of the rotation angle at one sigma, float64; terms summed over l in ascending order (the device kernel's
    order - the reference's np.sum is pairwise; the difference is below 1e-15, tests/test_refine_cpu.py)."""
    ls = np.arange(L_TRUNC, dtype=np.float64)
    coef = (2 * ls + 1) * np.exp(-ls * (ls + 1) * float(sigma) ** 2 / 2)
    terms = coef[None, :] * np.sin(OMEGA[:, None] * (ls[None, :] + 0.5)) / np.sin(OMEGA[:, None] / 2)
    expansion = np.zeros(NUM_OMEGA)
    for l in range(L_TRUNC):
        expansion += terms[:, l]
    pdf = expansion * (1 - np.cos(OMEGA)) / np.pi
    return np.cumsum(pdf) / NUM_OMEGA * np.pi


def inverse_cdf(u, cdf, omega=OMEGA):
    """Angles for uniforms u by the first-crossing rule of the module docstring."""
    u = np.atleast_1d(np.asarray(u, np.float64))
    cdf = np.asarray(cdf, np.float64)
    out = np.empty(u.shape, np.float64)
    for n, x in enumerate(u.reshape(-1)):
        hit = np.nonzero(cdf >= x)[0]
        if hit.size == 0:
            a = omega[-1]
        elif hit[0] == 0:
            a = omega[0]
        else:
            k = int(hit[0])
            a = (omega[k] - omega[k - 1]) / (cdf[k] - cdf[k - 1]) * (x - cdf[k - 1]) + omega[k - 1]
        out.reshape(-1)[n] = a
    return out


def time_grid(t_begin, eps, num_steps):
    """float32 linspace(t_begin, eps, num_steps) as dfm_refine builds it (torch.linspace's two-sided formula) and dt = ts[0] - ts[1]."""
    tb, eps = np.float32(t_begin), np.float32(eps)
    step = np.float32(eps - tb) / np.float32(num_steps - 1)
    ts = np.empty(num_steps, np.float32)
    for i in range(num_steps):      # one rounding per entry (a fused multiply-add, as torch.linspace computes it: tests/golden/scalar_kats.npz)
        ts[i] = np.float32(np.float64(tb) + np.float64(step) * i if i < num_steps // 2 else np.float64(eps) - np.float64(step) * (num_steps - 1 - i))
    return ts, np.float32(ts[0] - ts[1])


def forward_marginal(t, u_angle, axis_draw, tr_draw, hp: HParams | None = None, cdf=None):
    """(rot [B,3], tr [B,3]) float64 of the forward process at time t from its draws: u_angle [B] uniform, axis_draw [B,3] and
    tr_draw [B,3] N(0,1).  `cdf`: the table of sigma_index(t) (computed when None)."""
    if cdf is None:
        cdf = igso3_cdf(sigma_index(t, hp)[1])
    ax = np.asarray(axis_draw, np.float64).reshape(-1, 3)
    ax = ax / np.linalg.norm(ax, axis=-1, keepdims=True)
    ang = inverse_cdf(np.asarray(u_angle, np.float64).reshape(-1), cdf)
    return ax * ang[:, None], r3_sigma(t, hp) * np.asarray(tr_draw, np.float64).reshape(-1, 3)


def noise_pose(start, rot, tr, family=0):
    """modify_coords (score_model_mlsb.py:193-199) of one pose [L,3,3] in float32: rotation `rot` (axis-angle) about the CA centroid
    (family 1: the centroid of all backbone atoms), then translation `tr`."""
    from .pdbio import axis_angle_to_matrix
    x = np.asarray(start, np.float32).reshape(-1, 3, 3)
    c = (x.reshape(-1, 3).astype(np.float64).mean(0) if family == 1 else x[:, 1].astype(np.float64).mean(0)).astype(np.float32)
    Rm = axis_angle_to_matrix(np.asarray(rot, np.float32).astype(np.float64)).astype(np.float32)
    return ((x - c) @ Rm.T + c) + np.asarray(tr, np.float32)
