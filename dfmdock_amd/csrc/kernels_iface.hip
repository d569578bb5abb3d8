// kernels_iface.hip - interface energy of P rigid ligand poses: soft Lennard-Jones plus Coulomb with a distance-dependent dielectric
// over the heavy-atom pairs within a cutoff (include/dfmdock_amd.h: dfm_iface_create / dfm_pose_iface_energy; the float64 numpy
// definition is dfmdock_amd/ifenergy.py).
//
// A pair (receptor atom b, ligand atom a of a pose) counts when r2 = (dx*dx + dy*dy) + dz*dz, fp64 on the widened fp32 receptor atom and
// the fp64 ligand atom, is below cutoff^2.  Its three terms are functions of r2 alone - eps = slope r makes Coulomb q q / r2 - so there is
// no square root: fp64 + - * / in the definition's order, nothing contracted, are correctly rounded here and on the host.  Each term
// is rounded to an integer number of quanta of 2^-20 kcal/mol (round to nearest even) and everything after that is an integer sum, so
// no result depends on the order of the poses, on the blocks or on the chunks of a call.  dfm_poseprep.h (iface_sum_bound) shows that
// the sums can not wrap.
//
//   k_iface_pose   one lane per pose: the pose as 12 doubles (dfm_posewalk.h: pose_transform); zeroes the pose's four totals.
//   k_iface        one wave per (pose, block of 64 ligand atoms): the early exits and the staged receptor cell walk of dfm_posewalk.h,
//                  the receptor's (rmin_half, sqrt_eps, charge) staged next to its coordinates.  Per receptor atom the shared fp32
//                  reject; at 8 A a good share of the lanes pass it, so the fp64 recipe is not a per-lane branch: when any lane
//                  passes (one wave-uniform test) every lane evaluates it and a lane without a pair adds zeros.  int64 sums in
//                  registers, one plain store per lane and per-atom output, an integer wave reduction, one 64-bit integer atomic per
//                  block and total.  No floating-point atomic.  A wave that leaves early leaves the pose's totals at 0.
#include "dfm_internal.h"
#include "dfm_posewalk.h"

namespace dfm {

namespace {

constexpr double QUANTA = 1048576.0;      // 2^20 per kcal/mol

__device__ __forceinline__ long long wave_sum(long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

__global__ __launch_bounds__(64) void k_iface_pose(const float *__restrict__ rot, const float *__restrict__ tr, int n, double *__restrict__ T,
                                                   long long *__restrict__ tot)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    pose_transform(rot, tr, p, T);
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[(int64_t)p * 4 + k] = 0;
}

// grid (blocks of 64 ligand atoms, poses of the chunk)
__global__ __launch_bounds__(64) void k_iface(const float4 *__restrict__ rec, const float4 *__restrict__ rec_par,
                                              const int32_t *__restrict__ cell_start, const float4 *__restrict__ lig,
                                              const float4 *__restrict__ lig_par, const float4 *__restrict__ sphere,
                                              const int32_t *__restrict__ lig_index, const double *__restrict__ T, IfaceConst sc, int Al,
                                              unsigned long long *__restrict__ tot, long long *__restrict__ lig_vdw,
                                              long long *__restrict__ lig_elec)
{
    __shared__ float4 s_rec[64], s_par[64];
    const int lane = threadIdx.x, p = blockIdx.y, a = blockIdx.x * 64 + lane;
    WalkBlock w;
    if (!walk_front(sc.g, T, sphere, lig, Al, nullptr, w)) return;
    const bool valid = w.valid;
    const double X = w.X, Y = w.Y, Z = w.Z;
    const float xf = (float)X, yf = (float)Y, zf = (float)Z;
    const float4 lp = lig_par[valid ? a : Al - 1];
    const double rh_a = (double)lp.x, se_a = (double)lp.y, q_a = (double)lp.z;
    long long rep = 0, att = 0, elec = 0;
    int np = 0;
    walk_rows(sc.g, w, cell_start, rec, rec_par, s_rec, s_par, [&](int, const float4 r, const float4 rp) {
        const float dx = r.x - xf, dy = r.y - yf, dz = r.z - zf;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const bool near = valid && !(d2 > sc.reject2);
        if (__any(near)) {
            const double ex = X - (double)r.x, ey = Y - (double)r.y, ez = Z - (double)r.z;
            const double r2 = (ex * ex + ey * ey) + ez * ez;
            const bool pair = near && r2 < sc.cut2;
            const double Rm = rh_a + (double)rp.x, f = sc.soft * Rm, ff = f * f;
            const double r2v = r2 < ff ? ff : r2;
            const double s2 = (Rm * Rm) / r2v, s6 = (s2 * s2) * s2, e = se_a * (double)rp.y;
            const double t_rep = e * (s6 * s6), t_att = -2.0 * (e * s6);
            const double r2c = r2 < sc.min2 ? sc.min2 : r2;
            const double t_elec = (sc.kc * (q_a * (double)rp.z)) / r2c;
            const long long i_rep = __double2ll_rn(t_rep * QUANTA), i_att = __double2ll_rn(t_att * QUANTA);
            const long long i_elec = __double2ll_rn(t_elec * QUANTA);
            rep += pair ? i_rep : 0;
            att += pair ? i_att : 0;
            elec += pair ? i_elec : 0;
            np += pair ? 1 : 0;
        }
    });
    if (valid) {
        const int64_t o = (int64_t)p * Al + lig_index[a];
        if (lig_vdw) lig_vdw[o] = rep + att;
        if (lig_elec) lig_elec[o] = elec;
    }
    long long n = wave_sum((long long)np);
    if (n == 0) return;      // wave-uniform: no pair, the three sums are 0
    rep = wave_sum(rep);
    att = wave_sum(att);
    elec = wave_sum(elec);
    if (lane == 0) {
        unsigned long long *t = tot + (int64_t)p * 4;
        atomicAdd(t, (unsigned long long)rep);
        atomicAdd(t + 1, (unsigned long long)att);
        atomicAdd(t + 2, (unsigned long long)elec);
        atomicAdd(t + 3, (unsigned long long)n);
    }
}

hipError_t launch_iface_pose(const float *rot, const float *tr, int n, double *T, int64_t *tot, hipStream_t s)
{
    hipLaunchKernelGGL(k_iface_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), token_lds(), s, rot, tr, n, T,
                       reinterpret_cast<long long *>(tot));
    return hipGetLastError();
}

hipError_t launch_iface(const IfaceAtoms &at, const double *T, int n, int64_t *tot, int64_t *lig_vdw, int64_t *lig_elec, hipStream_t s)
{
    if (n < 1 || n > 65535) return hipErrorInvalidValue;      // poses are gridDim.y
    hipLaunchKernelGGL(k_iface, dim3((unsigned)((at.Al + 63) / 64), (unsigned)n), dim3(64), token_lds(), s,
                       reinterpret_cast<const float4 *>(at.rec), reinterpret_cast<const float4 *>(at.rec_par), at.cell_start,
                       reinterpret_cast<const float4 *>(at.lig), reinterpret_cast<const float4 *>(at.lig_par),
                       reinterpret_cast<const float4 *>(at.sphere), at.lig_index, T, at.sc, at.Al,
                       reinterpret_cast<unsigned long long *>(tot), reinterpret_cast<long long *>(lig_vdw),
                       reinterpret_cast<long long *>(lig_elec));
    return hipGetLastError();
}

}  // namespace dfm
