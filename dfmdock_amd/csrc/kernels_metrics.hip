// kernels_metrics.hip - docking metrics of P poses against one native (include/dfmdock_amd.h: dfm_native_create / dfm_pose_metrics; the
// float64 numpy definition is dfmdock_amd/metrics.py: compute_metrics).
//
// Per pose three Kabsch fits (all atoms: c_rmsd; interface atoms: i_rmsd; receptor atoms, applied to the ligand: l_rmsd) and the
// recovered native contacts.  Everything is carried in fp64 on the fp32 inputs, in coordinates shifted by `o` (the native's all-atom
// centroid rounded to fp32, so the shift is exact): p' = p - o, q' = q - o; a Kabsch fit is translation covariant.
//
//   k_metrics_reduce  one wave per (pose, chain): S = sum p', C = sum p' q'^T over all residues of the chain and over its interface
//                     residues (24 doubles).  Lanes take residues lane, lane + 64, ...; a xor butterfly finishes: the order of every
//                     sum depends on the chain length alone, never on P or on the pose's place in the batch.  The same kernel run on
//                     the native receptor as its own model gives the per-native constants used when the receptor does not move.
//   k_metrics_solve   one lane per pose: for each fit M = C - S qm^T, the proper rotation maximising sum q . (R p) as the dominant
//                     eigenvector of Horn's 4 x 4 quaternion matrix (cyclic Jacobi, fully unrolled index pattern: no private array
//                     is indexed dynamically) - the rotation Kabsch's SVD gives with its reflection fix - and t = qm - R pm.
//   k_metrics_resid   one wave per pose: the residuals of the EXPLICITLY transformed points (no E0 - 2 sum(sigma): that cancels to
//                     noise at native-like poses), and the native contact pairs whose minimum backbone-atom distance (9 atom pairs, the
//                     arithmetic of metrics._min_dist_pairs operation by operation) is below the cutoff.
//   k_native_pairs    dfm_native_create: per residue pair of the native, bit 0 = min distance < interface cutoff, bit 1 = < contact cutoff.
//
// Built with -ffp-contract=off: the distance arithmetic rounds like numpy's; the sums use explicit fma.
#include "dfm_contact.h"      // min_dist9
#include "dfm_horn.h"         // wave_sum, horn_rotation
#include "dfm_internal.h"

namespace dfm {

namespace {

constexpr int MW = 4;      // waves (poses) per workgroup

}  // namespace

__global__ __launch_bounds__(256) void k_native_pairs(const float *__restrict__ rec, const float *__restrict__ lig, int R, int L,
                                                      double iface_cutoff, double contact_cutoff, uint8_t *__restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)R * L) return;
    const int i = (int)(idx / L), j = (int)(idx % L);
    const double d = min_dist9(rec + (int64_t)i * 9, lig + (int64_t)j * 9);
    out[idx] = (uint8_t)((d < iface_cutoff ? 1 : 0) | (d < contact_cutoff ? 2 : 0));
}

// sums [P][chains][24]: S all [3] | C all [9] | S interface [3] | C interface [9]
__global__ __launch_bounds__(64 * MW) void k_metrics_reduce(MetricsChain c0, MetricsChain c1, int P, double ox, double oy, double oz,
                                                            double *__restrict__ sums)
{
    const int lane = threadIdx.x & 63, pose = blockIdx.x * MW + (threadIdx.x >> 6);
    if (pose >= P) return;
    const MetricsChain ch = blockIdx.y ? c1 : c0;
    const float *__restrict__ X = ch.model + (int64_t)pose * ch.n * 9;
    const double o[3] = {ox, oy, oz};
    double acc[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) acc[k] = 0.0;
    for (int r = lane; r < ch.n; r += 64) {
        double p[9], q[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            p[k] = (double)X[(int64_t)r * 9 + k] - o[k % 3];
            q[k] = (double)ch.native[(int64_t)r * 9 + k] - o[k % 3];
        }
        const bool in = ch.iface[r] != 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {      // atom
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                acc[i] += p[3 * a + i];
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[3 + 3 * i + j] = fma(p[3 * a + i], q[3 * a + j], acc[3 + 3 * i + j]);
            }
            if (in) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    acc[12 + i] += p[3 * a + i];
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[15 + 3 * i + j] = fma(p[3 * a + i], q[3 * a + j], acc[15 + 3 * i + j]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 24; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
        double *dst = sums + ((int64_t)pose * gridDim.y + blockIdx.y) * 24;
#pragma unroll
        for (int k = 0; k < 24; ++k) dst[k] = acc[k];
    }
}

// xf [P][3][12]: rotation (row-major) and translation of the fits all | interface | receptor, in the shifted coordinates
__global__ __launch_bounds__(64) void k_metrics_solve(const double *__restrict__ sums, int chains, const double *__restrict__ rec_const,
                                                      MetricsConst mc, int P, double *__restrict__ xf)
{
    const int pose = blockIdx.x * blockDim.x + threadIdx.x;
    if (pose >= P) return;
    const double *__restrict__ sl = sums + (int64_t)pose * chains * 24;
    const double *__restrict__ sr = chains == 2 ? sl + 24 : rec_const;
#pragma unroll 1
    for (int fit = 0; fit < 3; ++fit) {
        // fit 0: receptor + ligand, all | 1: receptor + ligand, interface | 2: receptor, all
        const int g = fit == 1 ? 12 : 0;
        const int n = (fit == 1 ? mc.n_rec_iface : mc.n_rec) + (fit == 2 ? 0 : (fit == 1 ? mc.n_lig_iface : mc.n_lig));
        double *dst = xf + ((int64_t)pose * 3 + fit) * 12;
        if (n == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) dst[k] = __longlong_as_double(0x7ff8000000000000LL);
            continue;
        }
        const double inv = 1.0 / (3.0 * (double)n);
        double S[3], T[3], M[3][3], r[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            S[i] = fit == 2 ? sr[g + i] : sr[g + i] + sl[g + i];
            const double tr = fit == 1 ? mc.T_rec_iface[i] : mc.T_rec[i], tl = fit == 1 ? mc.T_lig_iface[i] : mc.T_lig[i];
            T[i] = fit == 2 ? tr : tr + tl;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double c = fit == 2 ? sr[g + 3 + 3 * i + j] : sr[g + 3 + 3 * i + j] + sl[g + 3 + 3 * i + j];
                M[i][j] = c - S[i] * (T[j] * inv);
            }
        horn_rotation(M, r);
        // a NaN or an infinity in M: the Jacobi sweeps skip what they cannot order and would hand back a finite rotation; the fit is
        // undefined, so all of it is NaN (0 x M is 0 for every finite entry: finite fits keep their bits)
        double undefined = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) undefined += 0.0 * M[i][j];
        if (!(undefined == 0.0)) {
#pragma unroll
            for (int k = 0; k < 9; ++k) r[k] = __longlong_as_double(0x7ff8000000000000LL);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[k] = r[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            dst[9 + i] = T[i] * inv - (r[3 * i] * (S[0] * inv) + r[3 * i + 1] * (S[1] * inv) + r[3 * i + 2] * (S[2] * inv));
    }
}

namespace {

// |R p' + t - q'|^2 of one atom
__device__ inline double resid(const double *__restrict__ f, const double (&p)[3], const double (&q)[3])
{
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double d = fma(f[3 * i], p[0], fma(f[3 * i + 1], p[1], fma(f[3 * i + 2], p[2], f[9 + i]))) - q[i];
        e = fma(d, d, e);
    }
    return e;
}

}  // namespace

// rmsd [P][3] = c_rmsd, i_rmsd, l_rmsd; recovered [P]
__global__ __launch_bounds__(64 * MW) void k_metrics_resid(MetricsChain lig, MetricsChain rec, const double *__restrict__ xf, MetricsConst mc,
                                                           const int32_t *__restrict__ contacts, int P, double *__restrict__ rmsd,
                                                           int32_t *__restrict__ recovered)
{
    const int lane = threadIdx.x & 63, pose = blockIdx.x * MW + (threadIdx.x >> 6);
    if (pose >= P) return;
    const double *__restrict__ f = xf + (int64_t)pose * 36;
    const float *__restrict__ XL = lig.model + (int64_t)pose * lig.n * 9;
    const float *__restrict__ XR = rec.model + (int64_t)pose * rec.n * 9 * mc.rec_moves;      // rec_moves 0: the native receptor itself
    const double o[3] = {mc.o[0], mc.o[1], mc.o[2]};
    double eA = 0.0, eB = 0.0, eC = 0.0;
#pragma unroll 1
    for (int chain = 0; chain < 2; ++chain) {
        const MetricsChain ch = chain ? rec : lig;
        const float *__restrict__ X = chain ? XR : XL;
        for (int r = lane; r < ch.n; r += 64) {
            const bool in = ch.iface[r] != 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double p[3], q[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    p[i] = (double)X[(int64_t)r * 9 + 3 * a + i] - o[i];
                    q[i] = (double)ch.native[(int64_t)r * 9 + 3 * a + i] - o[i];
                }
                eA += resid(f, p, q);
                if (in) eB += resid(f + 12, p, q);
                if (chain == 0) eC += resid(f + 24, p, q);
            }
        }
    }
    int cnt = 0;
    for (int k = lane; k < mc.n_contacts; k += 64) {
        const int i = contacts[2 * k], j = contacts[2 * k + 1];
        cnt += min_dist9(XR + (int64_t)i * 9, XL + (int64_t)j * 9) < mc.contact_cutoff ? 1 : 0;
    }
    eA = wave_sum(eA); eB = wave_sum(eB); eC = wave_sum(eC);
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (lane == 0) {
        const int nb = mc.n_rec_iface + mc.n_lig_iface;
        rmsd[(int64_t)pose * 3 + 0] = sqrt(eA / (3.0 * (double)(mc.n_rec + mc.n_lig)));
        rmsd[(int64_t)pose * 3 + 1] = nb ? sqrt(eB / (3.0 * (double)nb)) : __longlong_as_double(0x7ff8000000000000LL);
        rmsd[(int64_t)pose * 3 + 2] = sqrt(eC / (3.0 * (double)mc.n_lig));
        recovered[pose] = cnt;
    }
}

hipError_t launch_native_pairs(const float *rec, const float *lig, int R, int L, double iface_cutoff, double contact_cutoff, uint8_t *out,
                               hipStream_t s)
{
    const int64_t n = (int64_t)R * L;
    hipLaunchKernelGGL(k_native_pairs, dim3((unsigned)((n + 255) / 256)), dim3(256), token_lds(), s, rec, lig, R, L, iface_cutoff,
                       contact_cutoff, out);
    return hipGetLastError();
}

hipError_t launch_metrics_reduce(const MetricsChain &c0, const MetricsChain &c1, int chains, int P, const MetricsConst &mc, double *sums,
                                 hipStream_t s)
{
    hipLaunchKernelGGL(k_metrics_reduce, dim3((unsigned)((P + MW - 1) / MW), (unsigned)chains), dim3(64 * MW), token_lds(), s, c0, c1, P,
                       mc.o[0], mc.o[1], mc.o[2], sums);
    return hipGetLastError();
}

hipError_t launch_metrics_finish(const MetricsChain &lig, const MetricsChain &rec, const double *sums, int chains, const double *rec_const,
                                 const MetricsConst &mc, const int32_t *contacts, int P, double *xf, double *rmsd, int32_t *recovered,
                                 hipStream_t s)
{
    hipLaunchKernelGGL(k_metrics_solve, dim3((unsigned)((P + 63) / 64)), dim3(64), token_lds(), s, sums, chains, rec_const, mc, P, xf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_metrics_resid, dim3((unsigned)((P + MW - 1) / MW)), dim3(64 * MW), token_lds(), s, lig, rec, xf, mc, contacts, P,
                       rmsd, recovered);
    return hipGetLastError();
}

}  // namespace dfm
