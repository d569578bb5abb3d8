// kernels_symmetry.hip - the Cn symmetry step of the sampler and its evaluation mode (include/dfmdock_amd.h: dfm_complex_set_symmetry,
// dfm_symmetry_eval; the numpy form in dfmdock_amd/symmetry.py is the spec).
// The ligand x is a pose of the receptor's own chain y.  (Q, tau) = the Horn fit of y onto x over all 3 M backbone atoms (dfm_horn.h):
// the monomer-to-monomer transform T.  theta, u = angle and axis of Q; c = the centre the sampler rotates about; g = Q^T (c - tau) the
// point T sends to c; s = u . (c - g) the screw translation; theta* = 2 pi m / n the nearest generator angle of the group.  Rotating x
// about c by (theta* - theta) u and shifting it by -s u makes T a pure rotation by theta*, T^n = identity; the step takes the fraction
// (gain_rot, gain_tr) of that, clipped like the restraint step, and all of it on the last step under snap_last.
// One 256-thread workgroup per trajectory, the shape of k_restraint (so that this kernel too can prepare the pose it produces for the
// next evaluation with prep_pose_block's bits).  Every sum is float64 in a fixed order - atoms strided over the lanes, the butterfly of
// a wave, the four waves in index order - so a trajectory's bits do not depend on B or on its place in the batch.  Two passes: the
// centroids, then the cross-covariance of the centred coordinates (a chain far from the origin loses nothing).  Lane 0 runs the 4 x 4
// Jacobi sweeps and the screw algebra (a few hundred dependent fp64 operations: latency, not throughput); the evaluation mode adds a
// third pass for the two explicit rms residuals.  The pose update is float32 with k_heads' / k_restraint's expressions.
// Built with -ffp-contract=off (dfm_horn.h needs it).
#include "dfm_device.h"
#include "dfm_horn.h"
#include "dfm_internal.h"

namespace dfm {

namespace {

// sums K values over the block: wave butterfly, then the waves in index order; every thread gets the totals.  dscr: 4 * K doubles
template <int K> __device__ inline void block_sum_k(double (&a)[K], double *dscr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = wave_sum_d(a[k]);
    __syncthreads();      // (the previous totals have been read)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) dscr[wave * K + k] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = ((dscr[k] + dscr[K + k]) + dscr[2 * K + k]) + dscr[3 * K + k];
}

__device__ inline int gcd_i(int a, int b)
{
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

}  // namespace

// s_par layout (doubles, written by lane 0 for the residual pass of the evaluation mode)
//   [0..8] Q   [9..11] tau   [12..20] rotation of the projection   [21..23] c   [24..26] c - s u
__global__ __launch_bounds__(256) void k_symmetry(SymmetryArgs p)
{
    __shared__ double dscr[4 * 9];
    __shared__ double s_par[27];
    __shared__ float s_upd[16], s_center[3];
    __shared__ int s_go, s_res;
    const int b = blockIdx.x, tid = threadIdx.x, L = p.L, A = L * 3;
    float *lig = p.lig + (size_t)b * L * 9;
    const float *rec = p.rec_pos;
    bool go = true, last = false;
    if (p.t_dev) {      // sampler: only from t_start on (step i's time; the replayed step graph reads i and the step count from its control words)
        const uint32_t idx = p.ctl ? p.ctl[0] - 1u : p.step;
        const uint32_t S = p.ctl ? p.ctl[3] : p.num_steps;
        go = p.t_dev[idx] <= p.t_start;
        last = idx + 1u == S;
    }
    if (go) {
        // pass 1: centroids of y and x over all atoms, and the centre the sampler rotates about
        double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int q = tid; q < A; q += blockDim.x) {
            a[0] += rec[q * 3]; a[1] += rec[q * 3 + 1]; a[2] += rec[q * 3 + 2];
            a[3] += lig[q * 3]; a[4] += lig[q * 3 + 1]; a[5] += lig[q * 3 + 2];
        }
        if (!p.all_atoms)
            for (int q = tid; q < L; q += blockDim.x) { a[6] += lig[q * 9 + 3]; a[7] += lig[q * 9 + 4]; a[8] += lig[q * 9 + 5]; }
        block_sum_k<9>(a, dscr);
        double ym[3], xm[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ym[k] = a[k] / A; xm[k] = a[3 + k] / A;
            c[k] = p.all_atoms ? xm[k] : a[6 + k] / L;
        }
        // pass 2: M[i][j] = sum (y - ym)_i (x - xm)_j
        double m9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int q = tid; q < A; q += blockDim.x) {
            const double y0 = (double)rec[q * 3] - ym[0], y1 = (double)rec[q * 3 + 1] - ym[1], y2 = (double)rec[q * 3 + 2] - ym[2];
            const double x0 = (double)lig[q * 3] - xm[0], x1 = (double)lig[q * 3 + 1] - xm[1], x2 = (double)lig[q * 3 + 2] - xm[2];
            m9[0] += y0 * x0; m9[1] += y0 * x1; m9[2] += y0 * x2;
            m9[3] += y1 * x0; m9[4] += y1 * x1; m9[5] += y1 * x2;
            m9[6] += y2 * x0; m9[7] += y2 * x1; m9[8] += y2 * x2;
        }
        block_sum_k<9>(m9, dscr);
        if (tid == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            double chk = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) chk += m9[k] - m9[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) chk += (ym[k] - ym[k]) + (xm[k] - xm[k]) + (c[k] - c[k]);
            const bool finite = chk == 0.0;      // (inf - inf and nan - nan are NaN)
            double theta = nan, screw = nan;
            double u[3] = {nan, nan, nan}, ap[3] = {nan, nan, nan};
            double st[6] = {nan, nan, nan, nan, nan, nan};
            int m_sel = 0, res = 0;
            if (finite) {
                const double M[3][3] = {{m9[0], m9[1], m9[2]}, {m9[3], m9[4], m9[5]}, {m9[6], m9[7], m9[8]}};
                double w, qx, qy, qz;
                horn_quaternion(M, w, qx, qy, qz);
                if (w < 0.0) { w = -w; qx = -qx; qy = -qy; qz = -qz; }
                double Q[9];
                quaternion_matrix(w, qx, qy, qz, Q);
                const double tau[3] = {xm[0] - ((Q[0] * ym[0] + Q[1] * ym[1]) + Q[2] * ym[2]),
                                       xm[1] - ((Q[3] * ym[0] + Q[4] * ym[1]) + Q[5] * ym[2]),
                                       xm[2] - ((Q[6] * ym[0] + Q[7] * ym[1]) + Q[8] * ym[2])};
                const double vn = sqrt((qx * qx + qy * qy) + qz * qz);
                res = 1;      // fit_rmsd only
#pragma unroll
                for (int k = 0; k < 9; ++k) { s_par[k] = Q[k]; s_par[12 + k] = (k % 4 == 0) ? 1.0 : 0.0; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { s_par[9 + k] = tau[k]; s_par[21 + k] = c[k]; s_par[24 + k] = c[k]; }
                if (vn <= 1e-9) {      // no axis: a zero step
                    theta = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) st[k] = 0.0;
                } else {
                    theta = 2.0 * atan2(vn, w);
                    u[0] = qx / vn; u[1] = qy / vn; u[2] = qz / vn;
                    const double d0 = c[0] - tau[0], d1 = c[1] - tau[1], d2 = c[2] - tau[2];
                    const double g[3] = {(Q[0] * d0 + Q[3] * d1) + Q[6] * d2, (Q[1] * d0 + Q[4] * d1) + Q[7] * d2,
                                         (Q[2] * d0 + Q[5] * d1) + Q[8] * d2};
                    screw = (u[0] * (c[0] - g[0]) + u[1] * (c[1] - g[1])) + u[2] * (c[2] - g[2]);
                    double ts = 0.0, bestd = 0.0;
                    for (int m = 1; m <= p.n / 2; ++m) {
                        if (gcd_i(m, p.n) != 1) continue;
                        const double t = 2.0 * 3.14159265358979323846 * (double)m / (double)p.n;
                        const double d = fabs(theta - t);
                        if (m_sel == 0 || d < bestd) { m_sel = m; ts = t; bestd = d; }
                    }
                    const double delta = ts - theta;
                    const bool snap = last && p.snap_last;
                    const double g_tr = snap ? 1.0 : (double)p.gain_tr, g_rot = snap ? 1.0 : (double)p.gain_rot;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { st[k] = -g_tr * screw * u[k]; st[3 + k] = g_rot * delta * u[k]; }
                    if (!snap) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {      // clip(v, m) = v min(1, m / |v|)
                            const double nn = sqrt(st[h * 3] * st[h * 3] + st[h * 3 + 1] * st[h * 3 + 1] + st[h * 3 + 2] * st[h * 3 + 2]);
                            const double mx = h ? p.max_rot : p.max_tr;
                            if (nn > mx) {
#pragma unroll
                                for (int k = 0; k < 3; ++k) st[h * 3 + k] *= mx / nn;
                            }
                        }
                    }
                    if (p.out) {
                        // a point of the axis, and the projection for the residual pass
                        const double e[3] = {c[0] - g[0] - screw * u[0], c[1] - g[1] - screw * u[1], c[2] - g[2] - screw * u[2]};
                        const double ct = 0.5 / tan(0.5 * ts);
                        ap[0] = 0.5 * (g[0] + c[0] - screw * u[0]) + ct * (u[1] * e[2] - u[2] * e[1]);
                        ap[1] = 0.5 * (g[1] + c[1] - screw * u[1]) + ct * (u[2] * e[0] - u[0] * e[2]);
                        ap[2] = 0.5 * (g[2] + c[2] - screw * u[2]) + ct * (u[0] * e[1] - u[1] * e[0]);
                        const double cd = cos(delta), sd = sin(delta), td = 1.0 - cd;
                        s_par[12] = cd + td * u[0] * u[0];        s_par[13] = td * u[0] * u[1] - sd * u[2]; s_par[14] = td * u[0] * u[2] + sd * u[1];
                        s_par[15] = td * u[0] * u[1] + sd * u[2]; s_par[16] = cd + td * u[1] * u[1];        s_par[17] = td * u[1] * u[2] - sd * u[0];
                        s_par[18] = td * u[0] * u[2] - sd * u[1]; s_par[19] = td * u[1] * u[2] + sd * u[0]; s_par[20] = cd + td * u[2] * u[2];
#pragma unroll
                        for (int k = 0; k < 3; ++k) s_par[24 + k] = c[k] - screw * u[k];
                        res = 2;      // fit_rmsd and sym_rmsd
                    }
                }
            }
            float tr[3], rot[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { tr[k] = (float)st[k]; rot[k] = (float)st[3 + k]; }
            if (p.out) {
                double *o = p.out + (size_t)b * SYM_OUT;
                o[0] = theta; o[1] = screw;
#pragma unroll
                for (int k = 0; k < 3; ++k) { o[2 + k] = u[k]; o[5 + k] = ap[k]; }
                o[8] = nan; o[9] = nan;      // (the residual pass fills them)
                o[10] = (double)m_sel;
            }
            if (p.step_out) {
                float *so = p.step_out + (size_t)b * 6;
#pragma unroll
                for (int k = 0; k < 3; ++k) { so[k] = tr[k]; so[3 + k] = rot[k]; }
            }
            s_res = p.out ? res : 0;
            const bool moves = p.apply && (tr[0] != 0.f || tr[1] != 0.f || tr[2] != 0.f || rot[0] != 0.f || rot[1] != 0.f || rot[2] != 0.f);
            s_go = moves;
            if (moves) {
                float Rm[9];
                aa_to_mat(rot, Rm);
#pragma unroll
                for (int k = 0; k < 9; ++k) s_upd[k] = Rm[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) { s_upd[9 + k] = tr[k]; s_upd[12 + k] = (float)c[k]; }
                float ru[3] = {p.rot_update[b * 3], p.rot_update[b * 3 + 1], p.rot_update[b * 3 + 2]}, rn[3];
                rot_compose(ru, rot, rn);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    p.tr_update[b * 3 + k] += tr[k];
                    p.rot_update[b * 3 + k] = rn[k];
                }
            }
        }
        __syncthreads();
        if (s_res) {      // evaluation mode: the explicit residuals of the fit and of the projection
            double r2[2] = {0, 0};
            for (int q = tid; q < A; q += blockDim.x) {
                const double y0 = rec[q * 3], y1 = rec[q * 3 + 1], y2 = rec[q * 3 + 2];
                const double x0 = lig[q * 3], x1 = lig[q * 3 + 1], x2 = lig[q * 3 + 2];
                const double f0 = (((s_par[0] * y0 + s_par[1] * y1) + s_par[2] * y2) + s_par[9]) - x0;
                const double f1 = (((s_par[3] * y0 + s_par[4] * y1) + s_par[5] * y2) + s_par[10]) - x1;
                const double f2 = (((s_par[6] * y0 + s_par[7] * y1) + s_par[8] * y2) + s_par[11]) - x2;
                r2[0] += (f0 * f0 + f1 * f1) + f2 * f2;
                const double v0 = x0 - s_par[21], v1 = x1 - s_par[22], v2 = x2 - s_par[23];
                const double h0 = (((s_par[12] * v0 + s_par[13] * v1) + s_par[14] * v2) + s_par[24]) - x0;
                const double h1 = (((s_par[15] * v0 + s_par[16] * v1) + s_par[17] * v2) + s_par[25]) - x1;
                const double h2 = (((s_par[18] * v0 + s_par[19] * v1) + s_par[20] * v2) + s_par[26]) - x2;
                r2[1] += (h0 * h0 + h1 * h1) + h2 * h2;
            }
            block_sum_k<2>(r2, dscr);
            if (tid == 0) {
                double *o = p.out + (size_t)b * SYM_OUT;
                o[8] = sqrt(r2[0] / A);
                if (s_res == 2) o[9] = sqrt(r2[1] / A);
            }
        }
        if (s_go) {      // modify_coords (inference_base.py:342-352) with k_heads' expressions
            for (int at = tid; at < A; at += blockDim.x) {
                const float v0 = lig[at * 3] - s_upd[12], v1 = lig[at * 3 + 1] - s_upd[13], v2 = lig[at * 3 + 2] - s_upd[14];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    float s = 0;
                    s += v0 * s_upd[r * 3]; s += v1 * s_upd[r * 3 + 1]; s += v2 * s_upd[r * 3 + 2];
                    lig[at * 3 + r] = (s + s_upd[12 + r]) + s_upd[9 + r];
                }
            }
        }
    }
    if (p.prep_next) {      // the last kernel that moves the pose prepares it for the next evaluation (k_heads / k_restraint do not, then)
        __syncthreads();
        const int N = p.R + L;
        prep_pose_block(p.rec_pos, lig, p.R, L, p.all_atoms, p.prep_pos + (size_t)b * N, p.prep_ca4 + (size_t)b * N, p.prep_cb4 + (size_t)b * N,
                        dscr, s_center);
    }
}

hipError_t launch_symmetry(const SymmetryArgs &a, int B, hipStream_t s)
{
    hipLaunchKernelGGL(k_symmetry, dim3(B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dfm
