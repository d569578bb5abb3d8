// kernels_surface.hip - buried solvent-accessible surface area (Shrake-Rupley) of P rigid ligand poses (include/dfmdock_amd.h:
// dfm_surface_create / dfm_pose_bsa; the float64 numpy definition is dfmdock_amd/surface.py).
//
// Every atom carries K sphere points c + R u_k (R = radius + probe, u_k the caller's table).  A point is exposed when no other atom of its
// own chain holds it (d < R_j, strict, d = sqrt((dx*dx + dy*dy) + dz*dz) in fp64) - that does not depend on the pose and is taken once,
// on the host, by surface_exposure below (this file is built with -ffp-contract=off for host and device alike).  A point is buried in a
// pose when it is exposed and an atom of the OTHER chain holds it.  Pose p of ligand atom a is (a - center) R(rot_p)^T + center + tr_p
// and its point k is x_a + R_a w_k with w_k = (R[:,0] u0 + R[:,1] u1) + R[:,2] u2; a receptor point is c_b + R_b u_k.  The decision is a
// bit; everything after it is an OR, a popcount or an integer sum, so no result depends on the order of the poses, on the blocks, on
// the order in which pairs are met or on the chunks of a call.
//
// What dfm_surface_create leaves on the device: the receptor atoms (x, y, z, radius) sorted by cell of a uniform grid whose edge is at
// least the largest R_a + R_b, with the cell starts, each sorted atom's index in the caller's order, radius class and K-bit exposure mask;
// the ligand atoms sorted by the Morton code of their cell, in blocks of 64 with a bounding sphere each, with the same per-atom arrays.
//
//   k_surface_pose    one lane per pose: the pose as 12 doubles (dfm_posewalk.h: pose_transform), zeroes the pose's class counters.
//   k_surface         one wave per (pose, block of 64 ligand atoms); the early exits and the staged receptor cell walk of dfm_posewalk.h.
//                     phase A  lanes are ATOMS.  Each receptor atom of the block's cell range, staged through LDS, is tested against the
//                              lane's atom in fp32: a pair passes unless d2 > ((R_a + R_b) 1.0001 + slack)^2.  A point of a lies R_a from
//                              x_a, so b can hold it only when |x_a - c_b| < R_a + R_b; slack (dfm_posewalk.h derives it: max(1e-3,
//                              2.5e-7 maxabs)) and the factor cover the fp32 rounding, so no pair that buries anything is dropped.
//                              Passing pairs (a, b) go to an LDS queue through a ballot and a prefix count.
//                     phase B  when the queue is nearly full and at the end: lanes are POINTS.  For each queued pair and each group of 64
//                              points, in both directions, the whole wave skips the group when the atom has no exposed point in it that
//                              is still unburied (ligand side) or no exposed point at all (receptor side); otherwise every lane takes the
//                              fp64 distance of its point in the definition's operation order and the ballot of d < R is the 64-bit
//                              buried mask.  The ligand atom's masks are ORed in LDS (the wave owns its 64 atoms), the receptor atom's
//                              into a per-(pose, receptor atom) K-bit mask in global memory by atomicOr.
//                     the end  lanes are atoms again: popcount of the block's masks -> lig_buried, integer atomics per radius class.
//   k_surface_finish  one lane per (pose, receptor atom): popcount of its mask -> rec_buried, integer atomics per radius class.
#include "dfm_internal.h"
#include "dfm_posewalk.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace dfm {

namespace {

constexpr int QCAP = 512;      // queue entries; drained when fewer than 64 are free

// phase B for the qn queued pairs of pose p.  s_x: X | Y | Z | R of the block's 64 atoms, s_w / s_u: the rotated and the plain sphere
// points as x | y | z rows of 256, s_bur [64][4]: the block's buried masks.  Wave-uniform control flow throughout.
__device__ __forceinline__ void drain(const SurfaceAtoms &at, int G, int blk, int64_t p, int lane, int qn, const uint32_t *s_q, const double *s_x,
                                      const double *s_w, const float *s_u, unsigned long long *s_bur, unsigned long long *__restrict__ rec_bur)
{
    const float4 *__restrict__ rec = reinterpret_cast<const float4 *>(at.rec);
    __syncthreads();      // the queue is written
    for (int i = 0; i < qn; ++i) {
        const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_q[i]);
        const int a = (int)(e >> 24), b = (int)(e & 0xffffffu);
        const float4 r = rec[b];
        const double bx = (double)r.x, by = (double)r.y, bz = (double)r.z, Rb = (double)r.w + at.sc.probe;
        const double ax = s_x[a], ay = s_x[64 + a], az = s_x[128 + a], Ra = s_x[192 + a];
        for (int g = 0; g < G; ++g) {
            const int k = g * 64 + lane;
            const unsigned long long todo = at.lig_exp[((int64_t)blk * 64 + a) * G + g] & ~s_bur[a * 4 + g];
            const unsigned long long rexp = at.rec_exp[(int64_t)b * G + g];
            __syncthreads();      // s_bur has been read by every lane before lane 0 changes it
            if (todo) {
                const double dx = (ax + Ra * s_w[k]) - bx, dy = (ay + Ra * s_w[256 + k]) - by, dz = (az + Ra * s_w[512 + k]) - bz;
                const double d = sqrt((dx * dx + dy * dy) + dz * dz);
                const unsigned long long hit = __ballot(d < Rb) & todo;
                if (hit && lane == 0) s_bur[a * 4 + g] |= hit;
            }
            if (rexp) {
                const double dx = (bx + Rb * (double)s_u[k]) - ax, dy = (by + Rb * (double)s_u[256 + k]) - ay, dz = (bz + Rb * (double)s_u[512 + k]) - az;
                const double d = sqrt((dx * dx + dy * dy) + dz * dz);
                const unsigned long long hit = __ballot(d < Ra) & rexp;
                if (hit && lane == 0) atomicOr(rec_bur + (p * at.Ar + b) * G + g, hit);
            }
            __syncthreads();      // lane 0's mask is visible to the next read
        }
    }
}

}  // namespace

__global__ __launch_bounds__(64) void k_surface_pose(const float *__restrict__ rot, const float *__restrict__ tr, int n, double *__restrict__ T,
                                                     int32_t *__restrict__ class_points)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    pose_transform(rot, tr, p, T);
    for (int c = 0; c < 32; ++c) class_points[(int64_t)p * 32 + c] = 0;
}

// grid (blocks of 64 ligand atoms, poses of the chunk).  rec_bur [n][Ar][G] zeroed by the caller; lig_buried [n][Al] (caller's atom
// order) or nullptr, written by the waves that reach the cell walk only, so zero it first; class_points [n][2][16]
__global__ __launch_bounds__(64) void k_surface(SurfaceAtoms at, const double *__restrict__ T, unsigned long long *__restrict__ rec_bur,
                                                int32_t *__restrict__ lig_buried, int32_t *__restrict__ class_points)
{
    __shared__ float4 s_rec[64];
    __shared__ double s_w[3 * 256];
    __shared__ float s_u[3 * 256];
    __shared__ double s_x[4 * 64];
    __shared__ unsigned long long s_bur[64 * 4];
    __shared__ uint32_t s_q[QCAP];
    const SurfaceConst &sc = at.sc;
    const int lane = threadIdx.x, blk = blockIdx.x, p = blockIdx.y, Al = at.Al, G = sc.G, a = blk * 64 + lane;
    WalkBlock w;
    // a NaN or infinite transform, a block out of reach of the receptor: nothing is buried
    if (!walk_front(sc.g, T, reinterpret_cast<const float4 *>(at.sphere), reinterpret_cast<const float4 *>(at.lig), Al, nullptr, w)) return;
    const bool valid = w.valid;
    const double *t = w.t, X = w.X, Y = w.Y, Z = w.Z, Ra = (double)w.l4.w + sc.probe;
    // the block's atoms and the pose's sphere points, for the lanes-are-points phase
    s_x[lane] = X; s_x[64 + lane] = Y; s_x[128 + lane] = Z; s_x[192 + lane] = Ra;
    for (int g = 0; g < 4; ++g) s_bur[lane * 4 + g] = 0ull;
    for (int g = 0; g < G; ++g) {
        const int k = g * 64 + lane;
        const float u0 = at.dirs[3 * k], u1 = at.dirs[3 * k + 1], u2 = at.dirs[3 * k + 2];
        s_u[k] = u0; s_u[256 + k] = u1; s_u[512 + k] = u2;
        s_w[k] = (t[0] * (double)u0 + t[1] * (double)u1) + t[2] * (double)u2;
        s_w[256 + k] = (t[3] * (double)u0 + t[4] * (double)u1) + t[5] * (double)u2;
        s_w[512 + k] = (t[6] * (double)u0 + t[7] * (double)u1) + t[8] * (double)u2;
    }
    const float xf = (float)X, yf = (float)Y, zf = (float)Z, raf = (float)Ra, probef = (float)sc.probe;
    int qn = 0;
    walk_rows(sc.g, w, at.cell_start, reinterpret_cast<const float4 *>(at.rec), s_rec, [&](int b, const float4 r) {
        const float dx = r.x - xf, dy = r.y - yf, dz = r.z - zf;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const float lim = (raf + (r.w + probef)) * 1.0001f + sc.slack;
        const bool close_by = valid && !(d2 > lim * lim);
        const unsigned long long m = __ballot(close_by);
        if (m) {
            const int at_q = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (close_by) s_q[at_q] = ((uint32_t)lane << 24) | (uint32_t)b;
            qn += __popcll(m);
            if (qn > QCAP - 64) {
                drain(at, G, blk, (int64_t)p, lane, qn, s_q, s_x, s_w, s_u, s_bur, rec_bur);
                qn = 0;
            }
        }
    });
    drain(at, G, blk, (int64_t)p, lane, qn, s_q, s_x, s_w, s_u, s_bur, rec_bur);
    if (valid) {
        int n = 0;
        for (int g = 0; g < G; ++g) n += __popcll(s_bur[lane * 4 + g]);
        if (lig_buried) lig_buried[(int64_t)p * Al + at.lig_index[a]] = n;
        if (n) atomicAdd(class_points + (int64_t)p * 32 + 16 + at.lig_class[a], n);
    }
}

// grid (blocks of 256 receptor atoms, poses of the chunk)
__global__ __launch_bounds__(256) void k_surface_finish(const unsigned long long *__restrict__ rec_bur, const int32_t *__restrict__ rec_index,
                                                        const int32_t *__restrict__ rec_class, int Ar, int G, int32_t *__restrict__ rec_buried,
                                                        int32_t *__restrict__ class_points)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (b >= Ar) return;
    int n = 0;
    for (int g = 0; g < G; ++g) n += __popcll(rec_bur[(p * Ar + b) * G + g]);
    if (rec_buried) rec_buried[p * Ar + rec_index[b]] = n;
    if (n) atomicAdd(class_points + p * 32 + rec_class[b], n);
}

hipError_t launch_surface_pose(const float *rot, const float *tr, int n, double *T, int32_t *class_points, hipStream_t s)
{
    hipLaunchKernelGGL(k_surface_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), token_lds(), s, rot, tr, n, T, class_points);
    return hipGetLastError();
}

hipError_t launch_surface(const SurfaceAtoms &at, const double *T, int n, uint64_t *rec_bur, int32_t *lig_buried, int32_t *rec_buried,
                          int32_t *class_points, hipStream_t s)
{
    if (n < 1 || n > 65535) return hipErrorInvalidValue;      // poses are gridDim.y
    hipLaunchKernelGGL(k_surface, dim3((unsigned)((at.Al + 63) / 64), (unsigned)n), dim3(64), token_lds(), s, at, T,
                       reinterpret_cast<unsigned long long *>(rec_bur), lig_buried, class_points);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_surface_finish, dim3((unsigned)((at.Ar + 255) / 256), (unsigned)n), dim3(256), token_lds(), s,
                       reinterpret_cast<const unsigned long long *>(rec_bur), at.rec_index, at.rec_class, at.Ar, at.sc.G, rec_buried,
                       class_points);
    return hipGetLastError();
}

// Isolated exposure of one chain on the host, exactly as the definition takes it.  xyz [n][3], radius [n]; start / order: the atoms
// sorted by cell of a grid (origin lo, dims, edge >= the largest R_i + R_j + pad), cell = (z ny + y) nx + x; mask [n][K / 64] in the
// caller's atom order.  Candidates of atom i: the atoms j != i of the 27 cells around it whose centre is closer than R_i + R_j + pad - a
// point of i lies R_i from c_i up to rounding far below pad - nearest first, so that a held point is found early.
void surface_exposure(int n, const float *xyz, const float *radius, double probe, int K, const float *dirs, const double lo[3],
                      const int dims[3], double edge, double pad, const int32_t *start, const int32_t *order, uint64_t *mask)
{
    const int G = K / 64;
    auto cell1 = [&](double x, int k) { return cell_of(x, lo[k], edge, dims[k]); };
    std::vector<std::pair<double, int>> cand;
    for (int i = 0; i < n; ++i) {
        const double cx = (double)xyz[(size_t)i * 3], cy = (double)xyz[(size_t)i * 3 + 1], cz = (double)xyz[(size_t)i * 3 + 2];
        const double Ri = (double)radius[i] + probe;
        const int c[3] = {cell1(cx, 0), cell1(cy, 1), cell1(cz, 2)};
        cand.clear();
        for (int z = std::max(0, c[2] - 1); z <= std::min(dims[2] - 1, c[2] + 1); ++z)
            for (int y = std::max(0, c[1] - 1); y <= std::min(dims[1] - 1, c[1] + 1); ++y) {
                const size_t row = ((size_t)z * dims[1] + y) * dims[0];
                for (int32_t q = start[row + std::max(0, c[0] - 1)]; q < start[row + std::min(dims[0] - 1, c[0] + 1) + 1]; ++q) {
                    const int j = order[q];
                    if (j == i) continue;
                    const double dx = (double)xyz[(size_t)j * 3] - cx, dy = (double)xyz[(size_t)j * 3 + 1] - cy, dz = (double)xyz[(size_t)j * 3 + 2] - cz;
                    const double d2 = (dx * dx + dy * dy) + dz * dz, lim = Ri + ((double)radius[j] + probe) + pad;
                    if (!(d2 > lim * lim)) cand.emplace_back(d2, j);
                }
            }
        std::sort(cand.begin(), cand.end());
        for (int g = 0; g < G; ++g) {
            uint64_t bits = 0;
            for (int l = 0; l < 64; ++l) {
                const float *u = dirs + (size_t)(g * 64 + l) * 3;
                const double qx = cx + Ri * (double)u[0], qy = cy + Ri * (double)u[1], qz = cz + Ri * (double)u[2];
                bool held = false;
                for (const auto &cj : cand) {
                    const int j = cj.second;
                    const double dx = qx - (double)xyz[(size_t)j * 3], dy = qy - (double)xyz[(size_t)j * 3 + 1], dz = qz - (double)xyz[(size_t)j * 3 + 2];
                    const double d = std::sqrt((dx * dx + dy * dy) + dz * dz);
                    if (d < (double)radius[j] + probe) { held = true; break; }
                }
                if (!held) bits |= 1ull << l;
            }
            mask[(size_t)i * G + g] = bits;
        }
    }
}

}  // namespace dfm
