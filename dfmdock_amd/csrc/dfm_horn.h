// dfm_horn.h - Horn's quaternion fit in fp64 on the device, shared by kernels_metrics.hip (docking metrics) and kernels_fit.hip (rigid
// pose fit): the wave sum of the reductions, the cyclic Jacobi sweeps on Horn's 4 x 4 matrix and the quaternion's rotation matrix.
// Include it from translation units built with -ffp-contract=off only: every operation rounds as it is written.
#pragma once

#include <hip/hip_runtime.h>

namespace dfm {

namespace {

__device__ inline double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one Jacobi rotation of the symmetric 4 x 4 matrix a in the (p, q) plane; v collects the eigenvectors as columns
template <int p, int q> __device__ inline void jacobi_rot(double (&a)[4][4], double (&v)[4][4])
{
    const double apq = a[p][q];
    if (!(fabs(apq) > 0.0)) return;      // also NaN: nothing to do, the solve kernels make the whole fit NaN
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[p][p] -= t * apq;
    a[q][q] += t * apq;
    a[p][q] = 0.0;
    a[q][p] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != p && k != q) {
            const double akp = a[k][p], akq = a[k][q];
            a[k][p] = c * akp - s * akq; a[p][k] = a[k][p];
            a[k][q] = s * akp + c * akq; a[q][k] = a[k][q];
        }
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
    }
}

// M[a][b] = sum (p - pm)_a (q - qm)_b  ->  the unit quaternion (w, x, y, z) of the proper rotation r with sum |r p - q|^2 minimal
// (Horn 1987): the eigenvector of the largest eigenvalue of Horn's matrix (first one on ties), sign as the sweeps leave it
__device__ inline void horn_quaternion(const double (&M)[3][3], double &w, double &x, double &y, double &z)
{
    double a[4][4], v[4][4];
    a[0][0] = M[0][0] + M[1][1] + M[2][2];
    a[1][1] = M[0][0] - M[1][1] - M[2][2];
    a[2][2] = -M[0][0] + M[1][1] - M[2][2];
    a[3][3] = -M[0][0] - M[1][1] + M[2][2];
    a[0][1] = a[1][0] = M[1][2] - M[2][1];
    a[0][2] = a[2][0] = M[2][0] - M[0][2];
    a[0][3] = a[3][0] = M[0][1] - M[1][0];
    a[1][2] = a[2][1] = M[0][1] + M[1][0];
    a[1][3] = a[3][1] = M[2][0] + M[0][2];
    a[2][3] = a[3][2] = M[1][2] + M[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        if (!(off > 0.0)) break;
        jacobi_rot<0, 1>(a, v); jacobi_rot<0, 2>(a, v); jacobi_rot<0, 3>(a, v);
        jacobi_rot<1, 2>(a, v); jacobi_rot<1, 3>(a, v); jacobi_rot<2, 3>(a, v);
    }
    double best = a[0][0];
    w = v[0][0]; x = v[1][0]; y = v[2][0]; z = v[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (a[k][k] > best) { best = a[k][k]; w = v[0][k]; x = v[1][k]; y = v[2][k]; z = v[3][k]; }
    const double n = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= n; x *= n; y *= n; z *= n;
}

// the row-major rotation matrix of a unit quaternion
__device__ inline void quaternion_matrix(double w, double x, double y, double z, double (&r)[9])
{
    r[0] = w * w + x * x - y * y - z * z; r[1] = 2.0 * (x * y - w * z);         r[2] = 2.0 * (x * z + w * y);
    r[3] = 2.0 * (x * y + w * z);         r[4] = w * w - x * x + y * y - z * z; r[5] = 2.0 * (y * z - w * x);
    r[6] = 2.0 * (x * z - w * y);         r[7] = 2.0 * (y * z + w * x);         r[8] = w * w - x * x - y * y + z * z;
}

// M as above  ->  row-major proper rotation r with sum |r p - q|^2 minimal
__device__ inline void horn_rotation(const double (&M)[3][3], double (&r)[9])
{
    double w, x, y, z;
    horn_quaternion(M, w, x, y, z);
    quaternion_matrix(w, x, y, z, r);
}

}  // namespace

}  // namespace dfm
