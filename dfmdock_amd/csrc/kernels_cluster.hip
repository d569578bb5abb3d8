// kernels_cluster.hip - pose clustering (include/dfmdock_amd.h: dfm_pose_rmsd / dfm_pose_cluster; the float64 numpy definition is
// dfmdock_amd/cluster.py).
//
// k_pose_dist: all-pairs ligand RMSD without superposition over one 64 x 64 tile of the upper triangle of the pose x pose matrix per
// workgroup.  256 lanes, each owning a 4 x 4 register block of pairs; coordinates staged through LDS in chunks of 32, transposed so that a
// lane reads its four a-poses and its four b-poses as one float4 each.  Every pair accumulates d = xa - xb, acc = fma(d, d, acc) over the
// coordinates in index order, so a pair's value depends on the two poses alone: bitwise symmetric (d and -d square alike), the same for
// any B, any tile position and any order of the poses.  Epilogue: the RMSD matrix (evaluation) or one bit per pair of the B x ceil(B/32)
// adjacency bitmask, (a, b) and (b, a); a 64-pose tile edge covers two whole bitmask words, so every word has exactly one writer.
//
// Clustering on the bitmask: rule 0 (leader) is one persistent workgroup that walks the key order with the unassigned set in LDS; rule 1
// (greedy by size) is popcount counts, then per cluster a one-workgroup arg-max + member step and a grid-wide decrement of the counts of
// the members' unassigned neighbours by integer atomics (order-independent result).
#include <climits>

#include "dfm_internal.h"

namespace dfm {

namespace {

constexpr int PT = 64;      // poses per tile edge
constexpr int KC = 32;      // coordinates per LDS chunk
constexpr int SP = PT + 4;  // LDS row stride (floats): float4-aligned, and the transposing stores spread over the banks

// coordinate k of a pose row: the residue subset (res != nullptr) maps residue k / 9 of the subset to its ligand residue
__device__ inline int64_t coord_col(const int32_t *res, int k) { return res ? (int64_t)res[k / 9] * 9 + k % 9 : (int64_t)k; }

// tile t of the upper triangle (row-major over ti <= tj) -> (ti, tj)
__device__ inline void tri_tile(int64_t t, int nt, int *ti, int *tj)
{
    // rows before ti hold ti * nt - ti (ti - 1) / 2 tiles
    double disc = (2.0 * nt + 1) * (2.0 * nt + 1) - 8.0 * (double)t;
    int i = (int)((2.0 * nt + 1 - sqrt(disc)) / 2.0);
    if (i < 0) i = 0;
    if (i > nt - 1) i = nt - 1;
    auto start = [nt](int r) { return (int64_t)r * nt - (int64_t)r * (r - 1) / 2; };
    while (i > 0 && start(i) > t) --i;
    while (i < nt - 1 && start(i + 1) <= t) ++i;
    *ti = i;
    *tj = i + (int)(t - start(i));
}

}  // namespace

__global__ __launch_bounds__(256) void k_pose_dist(const float *__restrict__ X, int B, int L9, const int32_t *__restrict__ res, int D,
                                                    float inv_atoms, float radius, float *__restrict__ rmsd, uint32_t *__restrict__ mask,
                                                    int W)
{
    __shared__ float sA[KC * SP], sB[KC * SP];
    __shared__ uint32_t bD[PT * 2], bT[PT * 2];
    const int nt = (B + PT - 1) / PT;
    int ti, tj;
    tri_tile(blockIdx.x, nt, &ti, &tj);
    const int a0 = ti * PT, b0 = tj * PT, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < D; k0 += KC) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < (PT * KC) / 256; ++r) {      // consecutive lanes read consecutive coordinates of one pose
            const int idx = tid + r * 256, p = idx / KC, k = idx % KC, kk = k0 + k;
            const int pa = a0 + p, pb = b0 + p;
            float va = 0.f, vb = 0.f;
            if (kk < D) {
                const int64_t col = coord_col(res, kk);
                if (pa < B) va = X[(int64_t)pa * L9 + col];
                if (pb < B) vb = X[(int64_t)pb * L9 + col];
            }
            sA[k * SP + p] = va;
            sB[k * SP + p] = vb;
        }
        __syncthreads();
        const int kn = D - k0 < KC ? D - k0 : KC;      // past D the staged values are zero: stopping there keeps every pair's sum the same
#pragma unroll 8
        for (int k = 0; k < kn; ++k) {
            const float4 a = *reinterpret_cast<const float4 *>(&sA[k * SP + ty * 4]);
            const float4 b = *reinterpret_cast<const float4 *>(&sB[k * SP + tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = av[i] - bv[j];
                    acc[i][j] = fmaf(d, d, acc[i][j]);
                }
        }
    }
    const bool diag = ti == tj;
    if (rmsd) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int a = a0 + ty * 4 + i, b = b0 + tx * 4 + j;
                if (a >= B || b >= B) continue;
                const float r = sqrtf(acc[i][j] * inv_atoms);
                rmsd[(int64_t)a * B + b] = r;
                if (!diag) rmsd[(int64_t)b * B + a] = r;
            }
        return;
    }
    if (tid < PT * 2) { bD[tid] = 0u; bT[tid] = 0u; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int la = ty * 4 + i, lb = tx * 4 + j;
            if (a0 + la >= B || b0 + lb >= B) continue;
            if (sqrtf(acc[i][j] * inv_atoms) <= radius) {
                atomicOr(&bD[la * 2 + (lb >> 5)], 1u << (lb & 31));
                atomicOr(&bT[lb * 2 + (la >> 5)], 1u << (la & 31));
            }
        }
    __syncthreads();
    if (tid < PT * 2) {      // lanes 0..127: the two words of row a0 + tid / 2; diagonal tiles write their own rows once
        const int r = tid >> 1, w = tid & 1;
        if (a0 + r < B && tj * 2 + w < W) mask[(int64_t)(a0 + r) * W + tj * 2 + w] = bD[tid];
    } else if (!diag) {
        const int t = tid - PT * 2, r = t >> 1, w = t & 1;
        if (b0 + r < B && ti * 2 + w < W) mask[(int64_t)(b0 + r) * W + ti * 2 + w] = bT[t];
    }
}

hipError_t launch_pose_dist(const float *X, int B, int L9, const int32_t *res, int n_res, float radius, float *rmsd, uint32_t *mask,
                            hipStream_t s)
{
    const int nt = (B + PT - 1) / PT, W = (B + 31) / 32;
    const int64_t tiles = (int64_t)nt * (nt + 1) / 2;
    const int D = n_res * 9;
    hipLaunchKernelGGL(k_pose_dist, dim3((unsigned)tiles), dim3(256), 0, s, X, B, L9, res, D, 1.0f / (float)(n_res * 3), radius, rmsd,
                       mask, W);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
namespace {

template <typename T, typename Op> __device__ inline T block_reduce(T v, T *scr, Op op)
{
    // 1024 lanes = 16 waves; scr holds 16 entries
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    __syncthreads();
    if (lane == 0) scr[wave] = v;
    __syncthreads();
    T r = scr[0];
    for (int w = 1; w < nw; ++w) r = op(r, scr[w]);
    return r;
}

struct MinOp { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct SumOp { __device__ int operator()(int a, int b) const { return a + b; } };
struct MaxOp64 { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; } };

// word w of the candidate set every rule starts from: the poses that are their own neighbour (the diagonal of the bitmask).  A pose
// with a non-finite coordinate among the compared residues is nobody's neighbour, itself included (sqrtf(NaN) <= radius is false): it
// never opens a cluster and never joins one.  Bits at or beyond B stay clear.
__device__ inline uint32_t self_bits(const uint32_t *__restrict__ mask, int w, int W, int B)
{
    const int n = B - w * 32 < 32 ? B - w * 32 : 32;
    uint32_t u = 0;
    for (int b = 0; b < n; ++b) u |= ((mask[(int64_t)(w * 32 + b) * W + w] >> b) & 1u) << b;
    return u;
}

}  // namespace

constexpr int CL_THREADS = 1024;
constexpr int CL_MAX_WORDS = 65536 / 32;

// rule 0: leader clustering, one workgroup.  order[B]: pose indices in key order.  out: cluster_of [B] (-1 = unassigned), center / size
// [max_clusters], n_out[0] = clusters formed.
__global__ __launch_bounds__(CL_THREADS) void k_cluster_leader(const uint32_t *__restrict__ mask, int B, int W, const int32_t *__restrict__ order,
                                                              int max_clusters, int32_t *__restrict__ cluster_of, int32_t *__restrict__ center,
                                                              int32_t *__restrict__ size, int32_t *__restrict__ n_out)
{
    __shared__ uint32_t U[CL_MAX_WORDS];
    __shared__ int scr[16];
    const int tid = threadIdx.x;
    for (int w = tid; w < W; w += CL_THREADS) U[w] = self_bits(mask, w, W, B);
    for (int i = tid; i < B; i += CL_THREADS) cluster_of[i] = -1;
    __syncthreads();
    int pos = 0, k = 0;
    while (k < max_clusters && pos < B) {
        // the next unassigned pose in key order
        int found = INT_MAX;
        for (; pos < B; pos += CL_THREADS) {
            const int i = pos + tid;
            int cand = INT_MAX;
            if (i < B) {
                const int p = order[i];
                if ((U[p >> 5] >> (p & 31)) & 1u) cand = i;
            }
            found = block_reduce(cand, scr, MinOp());
            if (found != INT_MAX) break;
        }
        if (found == INT_MAX) break;
        const int p = order[found];
        pos = found + 1;
        __syncthreads();      // every lane has read U for the scan
        int cnt = 0;
        for (int w = tid; w < W; w += CL_THREADS) {
            const uint32_t m = mask[(int64_t)p * W + w] & U[w];
            U[w] &= ~m;
            cnt += __popc(m);
            for (uint32_t b = m; b; b &= b - 1) cluster_of[w * 32 + __ffs(b) - 1] = k;
        }
        cnt = block_reduce(cnt, scr, SumOp());
        if (tid == 0) { center[k] = p; size[k] = cnt; }
        ++k;
        __syncthreads();
    }
    if (tid == 0) n_out[0] = k;
}

// rule 1, step 0: counts[i] = neighbours of i (all poses unassigned), U = every pose that is its own neighbour, cluster_of = -1,
// state = {clusters, done, members}
__global__ __launch_bounds__(256) void k_cluster_count(const uint32_t *__restrict__ mask, int B, int W, int32_t *__restrict__ counts,
                                                       uint32_t *__restrict__ U, int32_t *__restrict__ cluster_of, int32_t *__restrict__ state)
{
    const int lane = threadIdx.x & 63, gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    for (int r = gw; r < B; r += nw) {
        int c = 0;
        for (int w = lane; w < W; w += 64) c += __popc(mask[(int64_t)r * W + w]);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) { counts[r] = c; cluster_of[r] = -1; }
    }
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    for (int w = g; w < W; w += gridDim.x * blockDim.x) U[w] = self_bits(mask, w, W, B);
    if (g < 3) state[g] = 0;
}

// rule 1, per cluster: arg-max of (count, better key) over the unassigned poses, then its unassigned neighbours join cluster state[0]
// (members listed in mlist, their number in state[2]); state[1] = 1 once no pose is left.  pos[i]: rank of pose i in key order, order its
// inverse.
__global__ __launch_bounds__(CL_THREADS) void k_cluster_pick(const uint32_t *__restrict__ mask, int B, int W, const int32_t *__restrict__ counts,
                                                            const int32_t *__restrict__ pos, const int32_t *__restrict__ order,
                                                            uint32_t *__restrict__ U, int32_t *__restrict__ cluster_of,
                                                            int32_t *__restrict__ center, int32_t *__restrict__ size, int32_t *__restrict__ mlist,
                                                            int32_t *__restrict__ state)
{
    __shared__ unsigned long long scr64[16];
    __shared__ int scr[16];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    if (state[1]) return;
    unsigned long long best = 0;
    for (int i = tid; i < B; i += CL_THREADS) {
        if (!((U[i >> 5] >> (i & 31)) & 1u)) continue;
        const unsigned long long v = ((unsigned long long)(uint32_t)counts[i] << 32) | (uint32_t)(0x7fffffff - pos[i]);
        best = v > best ? v : best;
    }
    best = block_reduce(best, scr64, MaxOp64());
    const int k = state[0];
    if (best == 0) {      // every pose assigned (a pose in U is its own neighbour, so it counts at least itself)
        if (tid == 0) state[1] = 1;
        return;
    }
    const int ctr = order[0x7fffffff - (int)(uint32_t)(best & 0xffffffffu)];      // rank in key order -> pose
    if (tid == 0) s_n = 0;
    __syncthreads();
    int cnt = 0;
    for (int w = tid; w < W; w += CL_THREADS) {
        const uint32_t m = mask[(int64_t)ctr * W + w] & U[w];
        if (!m) continue;
        U[w] &= ~m;
        cnt += __popc(m);
        for (uint32_t b = m; b; b &= b - 1) {
            const int j = w * 32 + __ffs(b) - 1;
            cluster_of[j] = k;
            mlist[atomicAdd(&s_n, 1)] = j;      // list order varies; what the decrement computes from it does not
        }
    }
    cnt = block_reduce(cnt, scr, SumOp());
    if (tid == 0) {
        center[k] = ctr; size[k] = cnt;
        state[0] = k + 1; state[2] = cnt;
    }
}

// rule 1, per cluster: every unassigned neighbour j of every new member loses one unassigned neighbour
__global__ __launch_bounds__(256) void k_cluster_dec(const uint32_t *__restrict__ mask, int W, const uint32_t *__restrict__ U,
                                                     const int32_t *__restrict__ mlist, const int32_t *__restrict__ state,
                                                     int32_t *__restrict__ counts)
{
    if (state[1]) return;
    const int64_t items = (int64_t)state[2] * W;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        const int m = mlist[it / W], w = (int)(it % W);
        for (uint32_t b = mask[(int64_t)m * W + w] & U[w]; b; b &= b - 1) atomicSub(&counts[w * 32 + __ffs(b) - 1], 1);
    }
}

hipError_t launch_cluster_leader(const uint32_t *mask, int B, const int32_t *order, int max_clusters, int32_t *cluster_of, int32_t *center,
                                 int32_t *size, int32_t *n_out, hipStream_t s)
{
    if (B > 65536) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cluster_leader, dim3(1), dim3(CL_THREADS), 0, s, mask, B, (B + 31) / 32, order, max_clusters, cluster_of, center,
                       size, n_out);
    return hipGetLastError();
}

hipError_t launch_cluster_count(const uint32_t *mask, int B, int32_t *counts, uint32_t *U, int32_t *cluster_of, int32_t *state, hipStream_t s)
{
    const int W = (B + 31) / 32, blocks = (B + 3) / 4 < 4 * device_cus() ? (B + 3) / 4 : 4 * device_cus();
    hipLaunchKernelGGL(k_cluster_count, dim3(blocks), dim3(256), token_lds(), s, mask, B, W, counts, U, cluster_of, state);
    return hipGetLastError();
}

hipError_t launch_cluster_step(const uint32_t *mask, int B, int32_t *counts, const int32_t *pos, const int32_t *order, uint32_t *U, int32_t *cluster_of,
                               int32_t *center, int32_t *size, int32_t *mlist, int32_t *state, hipStream_t s)
{
    const int W = (B + 31) / 32;
    hipLaunchKernelGGL(k_cluster_pick, dim3(1), dim3(CL_THREADS), 0, s, mask, B, W, counts, pos, order, U, cluster_of, center, size, mlist, state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cluster_dec, dim3(2 * device_cus()), dim3(256), token_lds(), s, mask, W, U, mlist, state, counts);
    return hipGetLastError();
}

}  // namespace dfm
