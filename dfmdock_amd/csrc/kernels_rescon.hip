// kernels_rescon.hip - residue contacts of P rigid ligand poses: the SET of (receptor residue, ligand residue) pairs with two heavy atoms
// closer than a cutoff, counted by residue class (include/dfmdock_amd.h: dfm_rescon_create / dfm_pose_rescon; the float64 numpy
// definition is dfmdock_amd/affinity.py).
//
// An atom pair counts when d = sqrt((dx*dx + dy*dy) + dz*dz), fp64 on the widened fp32 receptor atom and the fp64 ligand atom, is below
// the cutoff - the contact test of kernels_sterics.hip.  What is asked for is not the number of such pairs but the set of residue pairs
// they make: a residue pair is found by many atoms, lanes, waves and blocks, and must count once.  So a pose has a bitmap [Lr][W] of
// 32-bit words in global memory, W = ceil(Rr / 32), bit i & 31 of word i >> 5 of row j = (receptor residue i, ligand residue j); setting
// a bit twice is setting it once.  Everything after the distance test is an integer, and OR commutes: no result depends on the order
// of the poses, on the blocks or on the chunks of a call.
//
//   k_rescon_pose     one lane per pose: the pose as 12 doubles (dfm_posewalk.h: pose_transform).
//   k_rescon          one wave per (pose, block of 64 ligand atoms): the early exits and the staged receptor cell walk of dfm_posewalk.h,
//                     the receptor atom's residue index riding as the bits of its float4's fourth component, the ligand atom's likewise.
//                     Per pair the shared fp32 reject, then the fp64 distance decides.  A counting pair sets its bit with a 32-bit
//                     atomicOr - after a relaxed load that skips the atomic when the bit is already there (a stale answer only costs
//                     the atomic: bits are never cleared while the kernel runs), and not at all when the lane's previous counting pair
//                     had the same receptor residue.  The bitmap is zeroed before the launch; a wave that leaves early leaves it so.
//   k_rescon_finish   one wave per pose, the lanes over the words of a row, one row after the other: popc(word & class mask) into a
//                     3 x 3 table by the row's ligand class (wave-uniform), the OR of the column words, the non-empty rows; integer
//                     wave sums, then lane 0 folds the table into the six unordered class pairs and stores the pose's nine totals.  No
//                     atomic and no floating point.  The two degree arrays are written only when asked for.
#include "dfm_internal.h"
#include "dfm_posewalk.h"

namespace dfm {

namespace {

__device__ __forceinline__ int wave_sum_i(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

__global__ __launch_bounds__(64) void k_rescon_pose(const float *__restrict__ rot, const float *__restrict__ tr, int n, double *__restrict__ T)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    pose_transform(rot, tr, p, T);
}

// grid (blocks of 64 ligand atoms, poses of the chunk).  bits [poses][Lr][W], zeroed
__global__ __launch_bounds__(64) void k_rescon(const float4 *__restrict__ rec, const int32_t *__restrict__ cell_start,
                                               const float4 *__restrict__ lig, const float4 *__restrict__ sphere,
                                               const double *__restrict__ T, ResconConst sc, int Al, int Lr, int W, uint32_t *bits)
{
    __shared__ float4 s_rec[64];
    const int p = blockIdx.y;
    WalkBlock w;
    if (!walk_front(sc.g, T, sphere, lig, Al, nullptr, w)) return;
    const bool valid = w.valid;
    const double X = w.X, Y = w.Y, Z = w.Z;
    const float xf = (float)X, yf = (float)Y, zf = (float)Z;
    // the lanes past Al repeat the last atom (walk_front): their row exists, and `valid` keeps them from writing
    uint32_t *row = bits + ((int64_t)p * Lr + __float_as_int(w.l4.w)) * W;
    int last = -1;
    walk_rows(sc.g, w, cell_start, rec, s_rec, [&](int, const float4 r) {
        const float dx = r.x - xf, dy = r.y - yf, dz = r.z - zf;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (valid && !(d2 > sc.reject2)) {
            const double ex = X - (double)r.x, ey = Y - (double)r.y, ez = Z - (double)r.z;
            const double d = sqrt((ex * ex + ey * ey) + ez * ez);
            const int i = __float_as_int(r.w);
            if (d < sc.cutoff && i != last) {
                last = i;
                uint32_t *word = row + (i >> 5);
                const uint32_t bit = 1u << (i & 31);
                if (!(__atomic_load_n(word, __ATOMIC_RELAXED) & bit)) atomicOr(word, bit);
            }
        }
    });
}

// grid (poses of the chunk).  tot [poses][9] = ic [6], n_pairs, n_rec_res, n_lig_res; rec_degree [poses][Rr] / lig_degree [poses][Lr] or
// nullptr
__global__ __launch_bounds__(64) void k_rescon_finish(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ class_mask,
                                                      const int32_t *__restrict__ lig_class, int Rr, int Lr, int W,
                                                      int32_t *__restrict__ tot, int32_t *__restrict__ rec_degree,
                                                      int32_t *__restrict__ lig_degree)
{
    const int lane = threadIdx.x, p = blockIdx.x;
    const uint32_t *b = bits + (int64_t)p * Lr * W;
    int t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, n_rec = 0, n_lig = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {      // W <= 128: at most two passes
        const int wd = w0 + lane;
        const bool in = wd < W;
        const uint32_t m0 = in ? class_mask[wd] : 0u, m1 = in ? class_mask[W + wd] : 0u, m2 = in ? class_mask[2 * W + wd] : 0u;
        uint32_t col = 0u;
        for (int j = 0; j < Lr; ++j) {
            const uint32_t v = in ? b[(int64_t)j * W + wd] : 0u;
            const int a = __builtin_amdgcn_readfirstlane(lig_class[j]);
            const int c0 = __popc(v & m0), c1 = __popc(v & m1), c2 = __popc(v & m2);
            col |= v;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t[k * 3] += a == k ? c0 : 0;
                t[k * 3 + 1] += a == k ? c1 : 0;
                t[k * 3 + 2] += a == k ? c2 : 0;
            }
        }
        n_rec += __popc(col);
    }
    // the rows: one lane per ligand residue, its words one after the other
    for (int j = lane; j < Lr; j += 64) {
        int deg = 0;
        for (int wd = 0; wd < W; ++wd) deg += __popc(b[(int64_t)j * W + wd]);
        n_lig += deg != 0 ? 1 : 0;
        if (lig_degree) lig_degree[(int64_t)p * Lr + j] = deg;
    }
    if (rec_degree)      // the columns: one lane per receptor residue
        for (int i = lane; i < Rr; i += 64) {
            int deg = 0;
            for (int j = 0; j < Lr; ++j) deg += (int)((b[(int64_t)j * W + (i >> 5)] >> (i & 31)) & 1u);
            rec_degree[(int64_t)p * Rr + i] = deg;
        }
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = wave_sum_i(t[k]);
    n_rec = wave_sum_i(n_rec);
    n_lig = wave_sum_i(n_lig);
    if (lane == 0) {
        int32_t *o = tot + (int64_t)p * 9;
        // t [ligand class][receptor class] -> AA, AP, AC, PP, PC, CC
        o[0] = t[0];
        o[1] = t[1] + t[3];
        o[2] = t[2] + t[6];
        o[3] = t[4];
        o[4] = t[5] + t[7];
        o[5] = t[8];
        o[6] = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7])) + t[8];
        o[7] = n_rec;
        o[8] = n_lig;
    }
}

hipError_t launch_rescon_pose(const float *rot, const float *tr, int n, double *T, hipStream_t s)
{
    hipLaunchKernelGGL(k_rescon_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), token_lds(), s, rot, tr, n, T);
    return hipGetLastError();
}

hipError_t launch_rescon(const ResconAtoms &at, const double *T, int n, uint32_t *bits, hipStream_t s)
{
    if (n < 1 || n > 65535) return hipErrorInvalidValue;      // poses are gridDim.y
    hipLaunchKernelGGL(k_rescon, dim3((unsigned)((at.Al + 63) / 64), (unsigned)n), dim3(64), token_lds(), s,
                       reinterpret_cast<const float4 *>(at.rec), at.cell_start, reinterpret_cast<const float4 *>(at.lig),
                       reinterpret_cast<const float4 *>(at.sphere), T, at.sc, at.Al, at.Lr, at.W, bits);
    return hipGetLastError();
}

hipError_t launch_rescon_finish(const ResconAtoms &at, const uint32_t *bits, int n, int32_t *tot, int32_t *rec_degree, int32_t *lig_degree,
                                hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rescon_finish, dim3((unsigned)n), dim3(64), token_lds(), s, bits, at.class_mask, at.lig_class, at.Rr, at.Lr, at.W,
                       tot, rec_degree, lig_degree);
    return hipGetLastError();
}

}  // namespace dfm
