// kernels_pairpot.hip - tabulated pair potential and pair counts of P rigid ligand poses: the sum of table[type_a][type_b][bin(r)] over
// the heavy-atom pairs within the last bin edge, and optionally the histogram of those pairs by (ligand type, receptor type, bin)
// (include/dfmdock_amd.h: dfm_pairpot_create / dfm_pose_pairpot; the float64 numpy definition is dfmdock_amd/pairpot.py).
//
// A pair (receptor atom b, ligand atom a of a pose) counts when r2 = (dx*dx + dy*dy) + dz*dz, fp64 on the widened fp32 receptor atom and
// the fp64 ligand atom, has e2[0] <= r2 < e2[NB], e2[k] = the exact square of edge k.  Its bin is k = #{j : e2[j] <= r2} - 1: no square
// root anywhere, the only rounding is r2's own, the same IEEE operations as the host's (nothing contracted).  The table was rounded to
// quanta of 2^-20 kcal/mol on the host (dfm_poseprep.h: quantise_pairpot) and everything here is an integer sum, so no result depends on
// the order of the poses, on the blocks or on the chunks of a call.  dfm_poseprep.h (pairpot_pair_bound) shows that nothing can wrap.
//
//   k_pairpot_pose     one lane per pose: the pose as 12 doubles (dfm_posewalk.h: pose_transform); zeroes the pose's two totals.
//   k_pairpot<COUNTS>  one wave per (pose, block of 64 ligand atoms): the early exits and the staged receptor cell walk of
//                      dfm_posewalk.h, the receptor's type (and its slab's offset in the table) staged next to its coordinates.  Per
//                      receptor atom the shared fp32 reject; when any lane passes (one wave-uniform test, as in k_iface) every lane takes
//                      the fp64 r2 and finds its bin by a branchless binary search over e2 in LDS, padded with +inf so that no step
//                      needs a bound (NB = 30: five steps of one ds_read_b64 each); a lane with a pair then loads
//                      table_q[(tb T + ta) NB + k] from global memory through the vector cache.  tb is the staged atom's, so it is
//                      wave-uniform: the 64 gathers of an iteration fall inside one slab of T NB 4 bytes.  int64 sums in registers, one
//                      plain store per lane for the per-atom output, an integer wave reduction, one 64-bit integer atomic per block
//                      and total.  No floating-point atomic.  A wave that leaves early leaves the pose's totals at 0.
//                      COUNTS: also one global int32 atomic per pair into counts[p][ta][tb][k] - 64 lanes into up to 64 lines, the
//                      slow, optional path; the COUNTS = false instantiation holds no code of it.
#include "dfm_internal.h"
#include "dfm_posewalk.h"

namespace dfm {

namespace {

__device__ __forceinline__ long long wave_sum(long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

__global__ __launch_bounds__(64) void k_pairpot_pose(const float *__restrict__ rot, const float *__restrict__ tr, int n, double *__restrict__ T,
                                                     long long *__restrict__ tot)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    pose_transform(rot, tr, p, T);
    tot[(int64_t)p * 2] = 0;
    tot[(int64_t)p * 2 + 1] = 0;
}

// grid (blocks of 64 ligand atoms, poses of the chunk)
template <bool COUNTS>
__global__ __launch_bounds__(64) void k_pairpot(const float4 *__restrict__ rec, const float4 *__restrict__ rec_par,
                                                const int32_t *__restrict__ cell_start, const float4 *__restrict__ lig,
                                                const int32_t *__restrict__ lig_type, const float4 *__restrict__ sphere,
                                                const int32_t *__restrict__ lig_index, const double *__restrict__ e2,
                                                const int32_t *__restrict__ table_q, const double *__restrict__ T, PairpotConst sc, int Al,
                                                unsigned long long *__restrict__ tot, long long *__restrict__ lig_q,
                                                int32_t *__restrict__ counts)
{
    __shared__ float4 s_rec[64], s_par[64];
    __shared__ double s_e2[PAIRPOT_E2_SLOTS];
    const int lane = threadIdx.x, p = blockIdx.y, a = blockIdx.x * 64 + lane;
    WalkBlock w;
    if (!walk_front(sc.g, T, sphere, lig, Al, nullptr, w)) return;
    s_e2[lane] = e2[lane];
    s_e2[lane + 64] = e2[lane + 64];      // read after the first barrier of walk_rows
    const bool valid = w.valid;
    const double X = w.X, Y = w.Y, Z = w.Z;
    const float xf = (float)X, yf = (float)Y, zf = (float)Z;
    const int ta = lig_type[valid ? a : Al - 1], row = ta * sc.NB;
    long long e = 0;
    int np = 0;
    int32_t *cnt = nullptr;
    if constexpr (COUNTS) cnt = counts + ((int64_t)p * sc.T + ta) * ((int64_t)sc.T * sc.NB);
    walk_rows(sc.g, w, cell_start, rec, rec_par, s_rec, s_par, [&](int, const float4 r, const float4 rp) {
        const float dx = r.x - xf, dy = r.y - yf, dz = r.z - zf;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const bool near = valid && !(d2 > sc.reject2);
        if (__any(near)) {
            const double ex = X - (double)r.x, ey = Y - (double)r.y, ez = Z - (double)r.z;
            const double r2 = (ex * ex + ey * ey) + ez * ez;
            const bool pair = near && r2 >= sc.lo2 && r2 < sc.cut2;
            // the largest k with e2[k] <= r2 (e2[0] <= r2 for a pair); the slots past NB hold +inf, a NaN stays at 0
            int k = 0;
            for (int step = sc.top; step > 0; step >>= 1) k += s_e2[k + step] <= r2 ? step : 0;
            if (pair) {
                const int slab = __builtin_amdgcn_readfirstlane(__float_as_int(rp.y));      // the staged atom's: wave-uniform
                e += (long long)table_q[slab + row + k];
                ++np;
                if constexpr (COUNTS) atomicAdd(cnt + __float_as_int(rp.x) * sc.NB + k, 1);
            }
        }
    });
    if (valid && lig_q) lig_q[(int64_t)p * Al + lig_index[a]] = e;
    long long n = wave_sum((long long)np);
    if (n == 0) return;      // wave-uniform: no pair, the sum is 0
    e = wave_sum(e);
    if (lane == 0) {
        unsigned long long *t = tot + (int64_t)p * 2;
        atomicAdd(t, (unsigned long long)e);
        atomicAdd(t + 1, (unsigned long long)n);
    }
}

hipError_t launch_pairpot_pose(const float *rot, const float *tr, int n, double *T, int64_t *tot, hipStream_t s)
{
    hipLaunchKernelGGL(k_pairpot_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), token_lds(), s, rot, tr, n, T,
                       reinterpret_cast<long long *>(tot));
    return hipGetLastError();
}

hipError_t launch_pairpot(const PairpotAtoms &at, const double *T, int n, int64_t *tot, int64_t *lig_q, int32_t *counts, hipStream_t s)
{
    if (n < 1 || n > 65535) return hipErrorInvalidValue;      // poses are gridDim.y
    const dim3 grid((unsigned)((at.Al + 63) / 64), (unsigned)n);
    const float4 *rec = reinterpret_cast<const float4 *>(at.rec), *rec_par = reinterpret_cast<const float4 *>(at.rec_par);
    const float4 *lig = reinterpret_cast<const float4 *>(at.lig), *sphere = reinterpret_cast<const float4 *>(at.sphere);
    unsigned long long *t = reinterpret_cast<unsigned long long *>(tot);
    long long *lq = reinterpret_cast<long long *>(lig_q);
    if (counts)
        hipLaunchKernelGGL((k_pairpot<true>), grid, dim3(64), token_lds(), s, rec, rec_par, at.cell_start, lig, at.lig_type, sphere, at.lig_index,
                           at.e2, at.table_q, T, at.sc, at.Al, t, lq, counts);
    else
        hipLaunchKernelGGL((k_pairpot<false>), grid, dim3(64), token_lds(), s, rec, rec_par, at.cell_start, lig, at.lig_type, sphere, at.lig_index,
                           at.e2, at.table_q, T, at.sc, at.Al, t, lq, counts);
    return hipGetLastError();
}

}  // namespace dfm
