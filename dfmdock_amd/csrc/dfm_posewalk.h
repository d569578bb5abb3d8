// dfm_posewalk.h - what the six per-pose all-atom kernels share (kernels_sterics.hip, kernels_surface.hip, kernels_iface.hip,
// kernels_rescon.hip, kernels_hbond.hip, kernels_pairpot.hip): a rigid ligand pose against a receptor whose atoms are sorted by cell
// of a uniform grid (dfm_walkgrid.h).  Device code.  tests/test_gpu_pose_kernels.py holds every step below to a float64 restatement,
// bitwise.
//
// A pose is 24 bytes: (rot, tr) of the sampler.  Pose p of ligand atom a is (a - center) R(rot_p)^T + center + tr_p in fp64.  One wave
// takes a (pose, block of 64 ligand atoms).  In this order:
//   1. a pose whose 12 doubles are not all finite is left alone (the definitions: a NaN distance is nothing);
//   2. the block's sphere, moved by the pose, against the receptor's bounding box grown by `grow`: most blocks of most poses are nowhere
//      near the receptor and the whole wave leaves here, having loaded 16 bytes;
//   3. each lane transforms its atom in fp64; the block's exact bounding box (fp64 wave min / max) against the grown box once more, then
//      its range of cells;
//   4. for every (y, z) row of that range the row's atoms (cell = (z ny + y) nx + x, so the cells x0 .. x1 of a row are ONE contiguous
//      range) are staged in LDS, 64 at a time by one coalesced load, and read back as broadcasts (every lane reads the same address: no
//      bank conflict, one ds_read_b128 per receptor atom for 64 pairs).  Letting each lane walk its own 27 cells instead would test about
//      a sixth of the pairs, but with 64 different cell ranges per wave: every load a scattered gather, every loop as long as the wave's
//      longest lane.  The staged form keeps the wave converged up to the kernel's fp64 part: a per-lane branch that few pairs take in
//      k_sterics, k_surface, k_rescon and k_hbond, the whole wave's converged evaluation behind one wave-uniform test in k_iface and
//      k_pairpot, where many pairs pass.
//
// The fp32 reject of the kernels: a pair is dropped without the fp64 arithmetic only when d2 > (reach * 1.0001f + slack)^2 with d2 taken
// in fp32 from the fp32 copy of the ligand atom (reach: the contact cutoff, R_a + R_b, or the energy cutoff, at most 16 A); written as !(d2 > ...) for the pairs that go
// on, so a NaN goes on.  Why that is conservative: a pair within reach has its ligand atom inside the receptor's box grown by the reach,
// so every coordinate involved is at most `maxabs` = the largest |coordinate| of that grown box.  The fp32 copy is off by at most 2^-24
// maxabs per axis, the three differences and d2 add relative errors of a few 2^-24, so the fp32 distance is off by at most sqrt(3) 2^-24
// maxabs + 4e-7 d < 1.04e-7 maxabs + 6.4e-6 (d <= 16, the largest reach of any caller).  slack = max(1e-3, 2.5e-7 maxabs) A (dfm_poseprep.h: pose_slack) is above the first
// term at any scale (it stays 1e-3 A up to maxabs = 4000 A, which holds every PDB file), and the factor 1.0001 (1e-4 d: 5e-4 A at 5 A, 1.6e-3 A
// at 16 A, against 4e-7 d) is above the second at any reach.  The same threshold is `grow` of the box tests of steps 2 and 3, which are taken in fp64; the cell of a coordinate is
// cell_of (dfm_walkgrid.h) in fp64 here and on the host, a monotone function of x, so a receptor atom within reach of the block's box can not lie in
// a cell below or above the block's range.
#pragma once

#include <hip/hip_runtime.h>

#include "dfm_walkgrid.h"

namespace dfm {

__device__ inline double wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

__device__ inline double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// T [p][12] = R(rot_p) row-major in fp64 from the axis-angle, pdbio.axis_angle_to_matrix operation by operation (small-angle branch
// included), then tr_p
__device__ __forceinline__ void pose_transform(const float *__restrict__ rot, const float *__restrict__ tr, int p, double *__restrict__ T)
{
    const double x = (double)rot[3 * p], y = (double)rot[3 * p + 1], z = (double)rot[3 * p + 2];
    const double ang = sqrt((x * x + y * y) + z * z);
    const double s = fabs(ang) < 1e-6 ? 0.5 - ang * ang / 48.0 : sin(0.5 * ang) / ang;
    const double r = cos(0.5 * ang), i = x * s, j = y * s, k = z * s;
    const double two_s = 2.0 / (((r * r + i * i) + j * j) + k * k);
    double *__restrict__ t = T + (int64_t)p * 12;
    t[0] = 1.0 - two_s * (j * j + k * k); t[1] = two_s * (i * j - k * r);       t[2] = two_s * (i * k + j * r);
    t[3] = two_s * (i * j + k * r);       t[4] = 1.0 - two_s * (i * i + k * k); t[5] = two_s * (j * k - i * r);
    t[6] = two_s * (i * k - j * r);       t[7] = two_s * (j * k + i * r);       t[8] = 1.0 - two_s * (i * i + j * j);
    t[9] = (double)tr[3 * p]; t[10] = (double)tr[3 * p + 1]; t[11] = (double)tr[3 * p + 2];
}

// what steps 1 to 3 leave a wave that goes on: the pose, the lane's ligand atom as stored and as posed (the lanes past Al repeat the
// last atom: they change no minimum or maximum, and are not `valid`), the block's cell range
struct WalkBlock {
    double t[12], X, Y, Z;
    float4 l4;
    bool valid;
    int cx0, cx1, cy0, cy1, cz0, cz1;
};

// steps 1 to 3 for the wave of block blockIdx.x (of 64 threads) and pose blockIdx.y; false, wave-uniformly: the wave has nothing to do.
// exits [2] (or nullptr) counts the waves that leave at the sphere test, at the box test.  (The counters are fed here and not by the
// caller from a result code: with a code the compiler builds another prologue for k_sterics, 1.167 against 1.095 ms of kernel time in
// the back-to-back runs of profiles/sterics.txt.)
__device__ __forceinline__ bool walk_front(const WalkGrid &g, const double *__restrict__ T, const float4 *__restrict__ sphere,
                                           const float4 *__restrict__ lig, int Al, unsigned long long *__restrict__ exits, WalkBlock &w)
{
    const int lane = threadIdx.x, blk = blockIdx.x, p = blockIdx.y;
    double *t = w.t, chk = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        t[k] = T[(int64_t)p * 12 + k];
        chk += t[k] * 0.0;
    }
    if (chk != chk) return false;
    {
        const float4 bs = sphere[blk];
        const double qx = (double)bs.x, qy = (double)bs.y, qz = (double)bs.z, reach = (double)bs.w + g.grow;
        const double cx = ((qx * t[0] + qy * t[1]) + qz * t[2]) + g.center[0] + t[9];
        const double cy = ((qx * t[3] + qy * t[4]) + qz * t[5]) + g.center[1] + t[10];
        const double cz = ((qx * t[6] + qy * t[7]) + qz * t[8]) + g.center[2] + t[11];
        const double ex = cx < g.lo[0] ? g.lo[0] - cx : (cx > g.hi[0] ? cx - g.hi[0] : 0.0);
        const double ey = cy < g.lo[1] ? g.lo[1] - cy : (cy > g.hi[1] ? cy - g.hi[1] : 0.0);
        const double ez = cz < g.lo[2] ? g.lo[2] - cz : (cz > g.hi[2] ? cz - g.hi[2] : 0.0);
        if ((ex * ex + ey * ey) + ez * ez > reach * reach) {
            if (exits && lane == 0) atomicAdd(exits, 1ull);
            return false;
        }
    }
    const int a = blk * 64 + lane;
    w.valid = a < Al;
    w.l4 = lig[w.valid ? a : Al - 1];
    const double qx = (double)w.l4.x - g.center[0], qy = (double)w.l4.y - g.center[1], qz = (double)w.l4.z - g.center[2];
    const double X = ((qx * t[0] + qy * t[1]) + qz * t[2]) + g.center[0] + t[9];
    const double Y = ((qx * t[3] + qy * t[4]) + qz * t[5]) + g.center[1] + t[10];
    const double Z = ((qx * t[6] + qy * t[7]) + qz * t[8]) + g.center[2] + t[11];
    const double x0 = wave_min(X) - g.grow, x1 = wave_max(X) + g.grow;
    const double y0 = wave_min(Y) - g.grow, y1 = wave_max(Y) + g.grow;
    const double z0 = wave_min(Z) - g.grow, z1 = wave_max(Z) + g.grow;
    if (x0 > g.hi[0] || x1 < g.lo[0] || y0 > g.hi[1] || y1 < g.lo[1] || z0 > g.hi[2] || z1 < g.lo[2]) {
        if (exits && lane == 0) atomicAdd(exits + 1, 1ull);
        return false;
    }
    w.X = X; w.Y = Y; w.Z = Z;
    // wave-uniform by construction; readfirstlane tells the compiler so (scalar loop control and scalar loads of the cell starts)
    w.cx0 = __builtin_amdgcn_readfirstlane(cell_of(x0, g.lo[0], g.edge, g.nx));
    w.cx1 = __builtin_amdgcn_readfirstlane(cell_of(x1, g.lo[0], g.edge, g.nx));
    w.cy0 = __builtin_amdgcn_readfirstlane(cell_of(y0, g.lo[1], g.edge, g.ny));
    w.cy1 = __builtin_amdgcn_readfirstlane(cell_of(y1, g.lo[1], g.edge, g.ny));
    w.cz0 = __builtin_amdgcn_readfirstlane(cell_of(z0, g.lo[2], g.edge, g.nz));
    w.cz1 = __builtin_amdgcn_readfirstlane(cell_of(z1, g.lo[2], g.edge, g.nz));
    return true;
}

// step 4: f(index among the sorted receptor atoms, that atom) for every receptor atom of the block's cell range, called by the whole
// wave at once (f may hold barriers: the block is one wave).  s_rec: 64 float4 of LDS
template <class F>
__device__ __forceinline__ void walk_rows(const WalkGrid &g, const WalkBlock &w, const int32_t *__restrict__ cell_start,
                                          const float4 *__restrict__ rec, float4 *s_rec, F &&f)
{
    const int lane = threadIdx.x;
    for (int cz = w.cz0; cz <= w.cz1; ++cz)
        for (int cy = w.cy0; cy <= w.cy1; ++cy) {
            const int row = (cz * g.ny + cy) * g.nx;
            const int b0 = cell_start[row + w.cx0], b1 = cell_start[row + w.cx1 + 1];
            for (int base = b0; base < b1; base += 64) {
                const int cnt = b1 - base < 64 ? b1 - base : 64;
                __syncthreads();      // the previous batch has been read
                if (lane < cnt) s_rec[lane] = rec[base + lane];
                __syncthreads();
                for (int j = 0; j < cnt; ++j) f(base + j, s_rec[j]);
            }
        }
}

// step 4 for a kernel whose receptor atoms carry a second float4 (rec2 [Ar], sorted like rec): f(index, atom, its second float4), both
// staged by the same two barriers.  s_rec, s_rec2: 64 float4 of LDS each.  An overload of its own, so that the kernels of the
// one-array walk above compile to what they were.
template <class F>
__device__ __forceinline__ void walk_rows(const WalkGrid &g, const WalkBlock &w, const int32_t *__restrict__ cell_start,
                                          const float4 *__restrict__ rec, const float4 *__restrict__ rec2, float4 *s_rec, float4 *s_rec2,
                                          F &&f)
{
    const int lane = threadIdx.x;
    for (int cz = w.cz0; cz <= w.cz1; ++cz)
        for (int cy = w.cy0; cy <= w.cy1; ++cy) {
            const int row = (cz * g.ny + cy) * g.nx;
            const int b0 = cell_start[row + w.cx0], b1 = cell_start[row + w.cx1 + 1];
            for (int base = b0; base < b1; base += 64) {
                const int cnt = b1 - base < 64 ? b1 - base : 64;
                __syncthreads();      // the previous batch has been read
                if (lane < cnt) {
                    s_rec[lane] = rec[base + lane];
                    s_rec2[lane] = rec2[base + lane];
                }
                __syncthreads();
                for (int j = 0; j < cnt; ++j) f(base + j, s_rec[j], s_rec2[j]);
            }
        }
}

}  // namespace dfm
