// kernels_fit.hip - rigid pose fit of P decoys of one complex (include/dfmdock_amd.h: dfm_pose_fit; the float64 numpy definition is
// dfmdock_amd/fit.py: fit_poses): from the coordinates of a rigidly placed ligand back to the sampler's (rot_update, tr_update).
//
// Per pose up to two Kabsch fits over backbone atoms with equal weights, everything in fp64 on the fp32 inputs, in coordinates shifted
// by `o` (the rotation centre, an fp32 triple, so the shift is exact; a Kabsch fit is translation covariant):
//   receptor (optional)  (Q, s) carries the decoy's receptor y onto the input's receptor y_ref: the decoy's frame into the input's;
//   ligand               (R, t) carries the input's ligand x0 onto x' = Q x + s (x' = x without a receptor).
//
//   k_fit_reduce  one wave per (pose, chain): S_pos = sum pos', S_ref = sum ref', C = sum pos' ref'^T (15 doubles).  Lanes take residues
//                 lane, lane + 64, ...; a xor butterfly finishes: the order of every sum depends on the chain length alone, never on P
//                 or on the pose's place in the batch.
//   k_fit_solve   one lane per pose: Q from M = C_rec - S_pos S_ref^T / n (Horn's quaternion, dfm_horn.h), s = ym_ref - Q ym; the
//                 ligand's covariance against x' follows algebraically, M = (C_lig^T - S_ref S_pos^T / n) Q^T - no second pass over
//                 the atoms; R from its quaternion q, and the axis-angle straight from q: sign fixed to w >= 0, angle 2 atan2(|v|, w),
//                 exactly zero for the identity.  With o = the centre c, tr = t + R c - c is the shifted frame's t itself.
//   k_fit_resid   one wave per pose: the residuals of the EXPLICITLY transformed points, |R x0' + t - (Q x' + s)| over the ligand
//                 and |Q y' + s - y_ref'| over the receptor (no E0 - 2 sum(sigma): that cancels to noise for a rigid image).
//
// A pose whose sums hold a NaN or an infinity is NaN in all its outputs and leaves its neighbours' bits alone.
// Built with -ffp-contract=off; the sums use explicit fma.
#include "dfm_horn.h"
#include "dfm_internal.h"

namespace dfm {

namespace {

constexpr int FW = 4;      // waves (poses) per workgroup
constexpr int FS = 15;     // doubles per (pose, chain): S_pos [3] | C [9] | S_ref [3]

__device__ inline double fit_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

}  // namespace

__global__ __launch_bounds__(64 * FW) void k_fit_reduce(FitChain c0, FitChain c1, int P, double ox, double oy, double oz,
                                                        double *__restrict__ sums)
{
    const int lane = threadIdx.x & 63, pose = blockIdx.x * FW + (threadIdx.x >> 6);
    if (pose >= P) return;
    const FitChain ch = blockIdx.y ? c1 : c0;
    const float *__restrict__ X = ch.pos + (int64_t)pose * ch.n * 9;
    const double o[3] = {ox, oy, oz};
    double acc[FS];
#pragma unroll
    for (int k = 0; k < FS; ++k) acc[k] = 0.0;
    for (int r = lane; r < ch.n; r += 64) {
        double p[9], q[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            p[k] = (double)X[(int64_t)r * 9 + k] - o[k % 3];
            q[k] = (double)ch.ref[(int64_t)r * 9 + k] - o[k % 3];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {      // atom
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                acc[i] += p[3 * a + i];
                acc[12 + i] += q[3 * a + i];
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[3 + 3 * i + j] = fma(p[3 * a + i], q[3 * a + j], acc[3 + 3 * i + j]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < FS; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
        double *dst = sums + ((int64_t)pose * gridDim.y + blockIdx.y) * FS;
#pragma unroll
        for (int k = 0; k < FS; ++k) dst[k] = acc[k];
    }
}

// xf [P][24]: R (row-major) and t of the ligand fit | Q and s of the receptor fit (the identity and zero without a receptor), in the
// shifted coordinates; rot [P][3], tr [P][3]: the pose in the sampler's convention about the centre o (the shift IS the centre, so tr = t)
__global__ __launch_bounds__(64) void k_fit_solve(const double *__restrict__ sums, int chains, int n_lig, int n_rec, int P,
                                                  double *__restrict__ xf, float *__restrict__ rot, float *__restrict__ tr)
{
    const int pose = blockIdx.x * blockDim.x + threadIdx.x;
    if (pose >= P) return;
    const double *__restrict__ sl = sums + (int64_t)pose * chains * FS;
    double Q[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, s[3] = {0.0, 0.0, 0.0};
    double undefined = 0.0;      // 0 x (every sum): 0 for finite sums, NaN otherwise - finite poses keep their bits
    if (chains == 2) {
        const double *__restrict__ sr = sl + FS;
        const double inv = 1.0 / (3.0 * (double)n_rec);
        double M[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            undefined += 0.0 * sr[i] + 0.0 * sr[12 + i];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                M[i][j] = sr[3 + 3 * i + j] - (sr[i] * sr[12 + j]) * inv;
                undefined += 0.0 * M[i][j];
            }
        }
        horn_rotation(M, Q);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            s[i] = sr[12 + i] * inv - (Q[3 * i] * (sr[0] * inv) + Q[3 * i + 1] * (sr[1] * inv) + Q[3 * i + 2] * (sr[2] * inv));
    }
    const double inv = 1.0 / (3.0 * (double)n_lig);
    // the ligand: p = x0 (the reference), q = x' = Q x + s.  A[a][c] = sum (x0 - x0m)_a (x - xm)_c, M = A Q^T
    double A[3][3], M[3][3], r[9], t[3], w, x, y, z;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        undefined += 0.0 * sl[a] + 0.0 * sl[12 + a];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[a][c] = sl[3 + 3 * c + a] - (sl[12 + a] * sl[c]) * inv;
            undefined += 0.0 * A[a][c];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) M[a][b] = A[a][0] * Q[3 * b] + A[a][1] * Q[3 * b + 1] + A[a][2] * Q[3 * b + 2];
    horn_quaternion(M, w, x, y, z);
    quaternion_matrix(w, x, y, z, r);
    // t = x'm - R x0m with x'm = Q xm + s
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double xm = Q[3 * i] * (sl[0] * inv) + Q[3 * i + 1] * (sl[1] * inv) + Q[3 * i + 2] * (sl[2] * inv) + s[i];
        t[i] = xm - (r[3 * i] * (sl[12] * inv) + r[3 * i + 1] * (sl[13] * inv) + r[3 * i + 2] * (sl[14] * inv));
    }
    // axis-angle straight from q
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double vn = sqrt(x * x + y * y + z * z);
    const double k = vn > 0.0 ? 2.0 * atan2(vn, w) / vn : 0.0;
    const double aa[3] = {k * x, k * y, k * z};
    double *dst = xf + (int64_t)pose * 24;
    const bool bad = !(undefined == 0.0);
#pragma unroll
    for (int i = 0; i < 9; ++i) { dst[i] = bad ? fit_nan() : r[i]; dst[12 + i] = bad ? fit_nan() : Q[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        dst[9 + i] = bad ? fit_nan() : t[i];
        dst[21 + i] = bad ? fit_nan() : s[i];
        rot[(int64_t)pose * 3 + i] = bad ? (float)fit_nan() : (float)aa[i];
        tr[(int64_t)pose * 3 + i] = bad ? (float)fit_nan() : (float)t[i];
    }
}

namespace {

// f (p) = F p + f_t of one atom, F row-major [9] followed by f_t [3]
__device__ inline void fit_apply(const double *__restrict__ f, const double (&p)[3], double (&out)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = fma(f[3 * i], p[0], fma(f[3 * i + 1], p[1], fma(f[3 * i + 2], p[2], f[9 + i])));
}

}  // namespace

// rmsd [P]; rec_rmsd [P] when rec.n > 0
__global__ __launch_bounds__(64 * FW) void k_fit_resid(FitChain lig, FitChain rec, const double *__restrict__ xf, int P, double ox, double oy,
                                                       double oz, double *__restrict__ rmsd, double *__restrict__ rec_rmsd)
{
    const int lane = threadIdx.x & 63, pose = blockIdx.x * FW + (threadIdx.x >> 6);
    if (pose >= P) return;
    const double *__restrict__ f = xf + (int64_t)pose * 24;
    const float *__restrict__ XL = lig.pos + (int64_t)pose * lig.n * 9;
    const double o[3] = {ox, oy, oz};
    double eL = 0.0, eR = 0.0;
    for (int r = lane; r < lig.n; r += 64) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double p[3], q[3], u[3], v[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                p[i] = (double)lig.ref[(int64_t)r * 9 + 3 * a + i] - o[i];
                q[i] = (double)XL[(int64_t)r * 9 + 3 * a + i] - o[i];
            }
            fit_apply(f, p, u);           // R x0' + t
            fit_apply(f + 12, q, v);      // Q x' + s
#pragma unroll
            for (int i = 0; i < 3; ++i) { const double d = u[i] - v[i]; eL = fma(d, d, eL); }
        }
    }
    if (rec.n > 0) {
        const float *__restrict__ XR = rec.pos + (int64_t)pose * rec.n * 9;
        for (int r = lane; r < rec.n; r += 64) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double p[3], q[3], v[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    p[i] = (double)XR[(int64_t)r * 9 + 3 * a + i] - o[i];
                    q[i] = (double)rec.ref[(int64_t)r * 9 + 3 * a + i] - o[i];
                }
                fit_apply(f + 12, p, v);      // Q y' + s
#pragma unroll
                for (int i = 0; i < 3; ++i) { const double d = v[i] - q[i]; eR = fma(d, d, eR); }
            }
        }
    }
    eL = wave_sum(eL);
    eR = wave_sum(eR);
    if (lane == 0) {
        rmsd[pose] = sqrt(eL / (3.0 * (double)lig.n));
        if (rec.n > 0) rec_rmsd[pose] = sqrt(eR / (3.0 * (double)rec.n));
    }
}

hipError_t launch_fit_reduce(const FitChain &lig, const FitChain &rec, int P, const double o[3], double *sums, hipStream_t s)
{
    if (P < 1 || lig.n < 1 || rec.n < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fit_reduce, dim3((unsigned)((P + FW - 1) / FW), rec.n > 0 ? 2u : 1u), dim3(64 * FW), token_lds(), s, lig, rec, P,
                       o[0], o[1], o[2], sums);
    return hipGetLastError();
}

hipError_t launch_fit_solve(const double *sums, int n_lig, int n_rec, int P, double *xf, float *rot, float *tr, hipStream_t s)
{
    if (P < 1 || n_lig < 1 || n_rec < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fit_solve, dim3((unsigned)((P + 63) / 64)), dim3(64), token_lds(), s, sums, n_rec > 0 ? 2 : 1, n_lig, n_rec, P, xf, rot,
                       tr);
    return hipGetLastError();
}

hipError_t launch_fit_resid(const FitChain &lig, const FitChain &rec, const double *xf, int P, const double o[3], double *rmsd,
                            double *rec_rmsd, hipStream_t s)
{
    if (P < 1 || lig.n < 1 || rec.n < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fit_resid, dim3((unsigned)((P + FW - 1) / FW)), dim3(64 * FW), token_lds(), s, lig, rec, xf, P, o[0], o[1], o[2],
                       rmsd, rec_rmsd);
    return hipGetLastError();
}

}  // namespace dfm
