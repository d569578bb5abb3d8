// dfm_schedule.h - the host arithmetic of the sampler and the decoding of the engine flags: diffusion coefficients, the time grid, the
// per-step scalars of the Euler-Maruyama update, the engine selection and the key of the captured step graph.  No HIP: the public C
// header and the standard library only, so tests/schedule_main.cpp runs it under g++ and its sanitizers (tests/test_schedule_cpu.py).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/dfmdock_amd.h"

namespace dfm {

// index of the first value of x[0 .. n) that is NaN or infinite; n when all are numbers (the stored pose of a complex must be:
// dfm_complex_create / dfm_complex_set_pose refuse it otherwise, include/dfmdock_amd.h "non-finite poses").  No part of the schedule:
// it lives here because this is the engine's one header of plain host C++ (no HIP), which tests/schedule_main.cpp already builds under
// the sanitizers - the scan of a caller's array is what such a build is for
inline size_t first_nonfinite(const float *x, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(x[k])) return k;
    return n;
}

// g(t) and sigma(t) of the R^3 (which 0) or SO(3) (which 1) diffuser; DFM_E_INVALID for another `which`, or t outside [0,1] on SO(3)
inline int diffusion_coef(const dfm_hparams &hp, int which, double t, double *g_out, double *sigma_out)
{
    double sigma, g;
    if (which == 0) {          // r3_diffuser.py:20-24
        sigma = hp.r3_min_sigma * std::pow(hp.r3_max_sigma / hp.r3_min_sigma, t);
        g = sigma * std::sqrt(2.0 * (std::log(hp.r3_max_sigma) - std::log(hp.r3_min_sigma)));
    } else if (which == 1) {   // so3_diffuser.py:210-227
        if (t < 0.0 || t > 1.0 || t != t) return DFM_E_INVALID;
        sigma = std::log(t * std::exp(hp.so3_max_sigma) + (1.0 - t) * std::exp(hp.so3_min_sigma));
        g = std::sqrt(2.0 * (std::exp(hp.so3_max_sigma) - std::exp(hp.so3_min_sigma)) * sigma / std::exp(sigma));
    } else {
        return DFM_E_INVALID;
    }
    if (g_out) *g_out = g;
    if (sigma_out) *sigma_out = sigma;
    return DFM_OK;
}

// The time grid of a sampler call: torch.linspace(t_first, eps, num_steps) in float32, dt = t[0] - t[1] (inference_base.py:404-405
// with t_first = 1) and g(t) of both diffusers at every entry.  An entry is the float32 product step * i rounded, then the float32
// sum rounded: two roundings, where torch.linspace and refine.time_grid round once - so single entries differ from theirs by one ulp
// (7 of 40 on the default grid).  Changing that changes trajectory bits; tests/test_schedule_cpu.py pins the arithmetic as it is.
struct TimeGrid {
    std::vector<float> ts;
    float dt = 0.f;
    std::vector<double> gr, gt;      // g of SO(3) / of R^3 at ts[i]
};
// DFM_E_INVALID (ValueError parity, so3_diffuser.py:210) when an entry lies outside [0,1]; needs num_steps >= 2
inline int time_grid(const dfm_hparams &hp, float t_first, float eps, int num_steps, TimeGrid *out)
{
    const size_t S = (size_t)num_steps;
    out->ts.resize(S); out->gr.resize(S); out->gt.resize(S);
    const float step = (eps - t_first) / (float)(num_steps - 1);
    for (int i = 0; i < num_steps; ++i)
        out->ts[i] = i < num_steps / 2 ? t_first + step * (float)i : eps - step * (float)(num_steps - 1 - i);
    out->dt = out->ts[0] - out->ts[1];
    for (int i = 0; i < num_steps; ++i) {
        const int rc = diffusion_coef(hp, 1, (double)out->ts[i], &out->gr[i], nullptr);
        if (rc) return rc;
        diffusion_coef(hp, 0, (double)out->ts[i], &out->gt[i], nullptr);
    }
    return DFM_OK;
}

// per-step scalars of the Euler-Maruyama update: by value in the arguments of step i's k_heads launch, or read by k_heads from
// device memory when the step loop is a replayed graph
struct StepParams { float g2_r, g_r, hg2_r, g2_t, g_t, hg2_t, dt, sqrt_dt, rot_noise, tr_noise; uint32_t step, pad; };

inline StepParams step_params(const TimeGrid &g, int i, uint32_t flags, float tr_noise_scale, float rot_noise_scale, int num_steps)
{
    const bool is_last = (i == num_steps - 1);
    const double gr = g.gr[i], gt = g.gt[i];
    StepParams p;
    p.g2_r = (float)(gr * gr); p.g_r = (float)gr; p.hg2_r = (float)(0.5 * (gr * gr));
    p.g2_t = (float)(gt * gt); p.g_t = (float)gt; p.hg2_t = (float)(0.5 * (gt * gt));
    p.dt = g.dt; p.sqrt_dt = std::sqrt(g.dt);
    if (flags & DFM_F_NOISE_ANNEALING) { p.tr_noise = g.ts[i]; p.rot_noise = g.ts[i]; }       // inference_base.py:428-430
    else { p.tr_noise = is_last ? 0.0f : tr_noise_scale; p.rot_noise = is_last ? 0.0f : rot_noise_scale; }
    p.step = (uint32_t)i; p.pad = 0u;
    return p;
}

// The engine `flags` select.  bf16: a 16-bit MFMA engine; f16: ... with fp32 A_i; bf16_ops: bf16 MFMA operands in every layer but the
// last; has_table: the engine has a layer-0 message table - the fp32 engine and the shipped 16-bit plan (DFM_F_MFMA16 alone) do
struct EngineSel { bool bf16, f16, bf16_ops, has_table; };
inline EngineSel engine_sel(uint32_t flags)
{
    EngineSel s;
    s.f16 = (flags & DFM_F_F16) != 0;
    s.bf16 = (flags & DFM_F_MFMA16) || s.f16;
    s.bf16_ops = s.bf16 && !s.f16 && (flags & DFM_F_BF16_OPS);
    s.has_table = (s.bf16 && !s.f16 && !(flags & DFM_F_BF16_OPS)) || !s.bf16;
    return s;
}
// dfm_sample, dfm_refine and dfm_complex_selfcheck go through the table unless told otherwise (and where the complex is eligible)
inline bool table_by_default(const EngineSel &s, uint32_t flags) { return s.has_table && !(flags & DFM_F_NO_L0_TABLE); }

// what the captured step graph of a handle was captured for: the batch, the flags that change its nodes, whether layer 0 goes through
// the table and whether the restraint step and the symmetry step are part of it
inline uint64_t graph_key(int B, uint32_t flags, bool l0, bool restr, bool sym = false)
{
    return ((uint64_t)(uint32_t)B << 32) | (uint64_t)(flags & (DFM_F_MFMA16 | DFM_F_F16 | DFM_F_BF16_OPS | DFM_F_CLASH_FORCE | DFM_F_ODE | DFM_F_NO_L0_TABLE))
           | (l0 ? 1ull << 31 : 0ull) | (restr ? (uint64_t)DFM_F_RESTRAINTS : 0ull) | (sym ? (uint64_t)DFM_F_SYMMETRY : 0ull);
}

}  // namespace dfm
