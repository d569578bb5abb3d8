// kernels_consensus.hip - consensus contact scoring of P poses (include/dfmdock_amd.h: dfm_pose_consensus; the float64 numpy definition
// is dfmdock_amd/consensus.py).
//
// A contact of pose p is a residue pair (receptor i, ligand j) whose minimum backbone-atom distance (9 atom pairs, min_dist9 of
// dfm_contact.h: the arithmetic of metrics._min_dist operation by operation, fp64 on the fp32 inputs) is below the cutoff.  Everything
// after that decision is an integer.  The contact bits of a chunk of poses live on the device as bits [n][W][R] uint64, W = ceil(L / 64):
// word (p, w, i) holds ligand residues 64 w .. 64 w + 63 of receptor residue i, bit j % 64 = contact (i, j), unused high bits 0 - the
// transpose of the layout the C ABI hands out, so that the 64 words a wave writes or reads at once are 512 contiguous bytes.
//
//   k_contact_bits       one wave per (pose, 64 ligand residues, 64 receptor residues).  Lane = ligand residue, held in registers; the
//                        receptor rows and their reach (largest CA-to-atom distance) are staged in LDS and read as broadcasts.  Per row
//                        a cheap fp32 reject, then min_dist9 for the lanes that survive; the wave's __ballot IS the packed word.  Lane r
//                        keeps the word of row r, so the wave ends with one 512-byte store.
//                        The reject is conservative by construction: with a, b the atoms of the closest pair,
//                        |CA_i - CA_j| <= |CA_i - a| + |a - b| + |b - CA_j| <= reach_i + d + reach_j, so d >= cutoff whenever
//                        |CA_i - CA_j| >= cutoff + reach_i + reach_j.  The fp32 test rejects only when
//                        |CA_i - CA_j|^2 > ((cutoff + reach_i + reach_j) * 1.0001 + 0.001)^2: every fp32 quantity in it carries a
//                        relative rounding error below 1e-6, the margin is 1e-4 relative plus 1e-3 A.  A comparison with NaN is false,
//                        i.e. not rejected: such pairs reach the fp64 arithmetic, which gives NaN = no contact.
//   k_contact_count      count[i][j] += contacts of the MEMBER poses: one wave per (64 receptor residues, w, slice of the poses), 64
//                        counters per lane in registers (static indices), one integer atomic per non-zero counter at the end.
//   k_contact_marginals  rec_count / lig_count: member poses in which a row / a column of the bit matrix is not empty (OR over the
//                        words of the row; OR over the rows, finished by a wave butterfly).
//   k_contact_score      one wave per pose, members or not: n_contacts = popcount, score_sum = sum of count over the set bits (int64).
//
// Integer sums and atomics only: no result depends on the order of the poses, on the slices or on the chunks of a call.
#include "dfm_contact.h"
#include "dfm_internal.h"

namespace dfm {

namespace {

constexpr int RS = 12;      // floats per staged receptor row: 9 coordinates, the reach, 2 of padding (16-byte rows)
constexpr int SW = 4;       // waves (poses) per workgroup of k_contact_score

// largest CA-to-atom distance of one residue (N, CA, C), fp32.  A NaN here makes the reject's comparison false (not rejected)
__device__ inline float reach(const float *__restrict__ x)
{
    const float ax = x[0] - x[3], ay = x[1] - x[4], az = x[2] - x[5];
    const float cx = x[6] - x[3], cy = x[7] - x[4], cz = x[8] - x[5];
    const float a = (ax * ax + ay * ay) + az * az, c = (cx * cx + cy * cy) + cz * cz;
    return sqrtf((a > c || a != a) ? a : c);
}

__device__ inline uint64_t wave_or(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, o);
    return v;
}

}  // namespace

__global__ __launch_bounds__(64) void k_contact_bits(const float *__restrict__ rec, const float *__restrict__ lig, int R, int L, int W,
                                                     float cutoff_f, double cutoff, uint64_t *__restrict__ bits)
{
    __shared__ float s_rec[64 * RS];
    const int lane = threadIdx.x, w = (int)(blockIdx.x % (unsigned)W), i0 = (int)(blockIdx.x / (unsigned)W) * 64, p = blockIdx.y;
    const int rows = R - i0 < 64 ? R - i0 : 64, j = w * 64 + lane;
    if (lane < rows) {
        const float *__restrict__ src = rec + (int64_t)(i0 + lane) * 9;
        float *dst = s_rec + lane * RS;
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[k] = src[k];
        dst[9] = reach(src);
    }
    const bool valid = j < L;
    float lj[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) lj[k] = valid ? lig[((int64_t)p * L + j) * 9 + k] : 0.f;
    const float far = cutoff_f + reach(lj);
    __syncthreads();
    uint64_t mine = 0;
    for (int r = 0; r < rows; ++r) {
        const float *ri = s_rec + r * RS;
        const float dx = ri[3] - lj[3], dy = ri[4] - lj[4], dz = ri[5] - lj[5];
        const float d2 = (dx * dx + dy * dy) + dz * dz, thr = (far + ri[9]) * 1.0001f + 1e-3f;
        bool c = false;
        if (valid && !(d2 > thr * thr)) c = min_dist9(ri, lj) < cutoff;
        const uint64_t word = __ballot(c);
        if (lane == r) mine = word;
    }
    if (lane < rows) bits[((int64_t)p * W + w) * R + i0 + lane] = mine;
}

// grid (W * ceil(R / 64), slices): poses blockIdx.y, blockIdx.y + slices, ... of the chunk
__global__ __launch_bounds__(64) void k_contact_count(const uint64_t *__restrict__ bits, const uint8_t *__restrict__ member, int n, int R, int L,
                                                      int W, int32_t *__restrict__ count)
{
    const int lane = threadIdx.x, w = (int)(blockIdx.x % (unsigned)W), i = (int)(blockIdx.x / (unsigned)W) * 64 + lane;
    int cnt[64];
#pragma unroll
    for (int b = 0; b < 64; ++b) cnt[b] = 0;
    for (int p = blockIdx.y; p < n; p += gridDim.y) {
        if (!member[p]) continue;
        const uint64_t word = i < R ? bits[((int64_t)p * W + w) * R + i] : 0;
        if (__ballot(word != 0) == 0) continue;
        const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            cnt[b] += (int)((lo >> b) & 1u);
            cnt[32 + b] += (int)((hi >> b) & 1u);
        }
    }
    if (i >= R) return;
    int32_t *__restrict__ row = count + (int64_t)i * L + w * 64;
#pragma unroll
    for (int b = 0; b < 64; ++b)
        if (cnt[b] != 0 && w * 64 + b < L) atomicAdd(row + b, cnt[b]);
}

// grid (W + ceil(R / 64), slices): blocks [0, W) count the columns of ligand word w, the others the rows of 64 receptor residues
__global__ __launch_bounds__(64) void k_contact_marginals(const uint64_t *__restrict__ bits, const uint8_t *__restrict__ member, int n, int R,
                                                          int L, int W, int32_t *__restrict__ rec_count, int32_t *__restrict__ lig_count)
{
    const int lane = threadIdx.x, role = blockIdx.x;
    int acc = 0;
    if (role < W) {
        for (int p = blockIdx.y; p < n; p += gridDim.y) {
            if (!member[p]) continue;
            const uint64_t *__restrict__ col = bits + ((int64_t)p * W + role) * R;
            uint64_t any = 0;
            for (int i = lane; i < R; i += 64) any |= col[i];
            acc += (int)((wave_or(any) >> lane) & 1u);
        }
        const int j = role * 64 + lane;
        if (acc != 0 && j < L) atomicAdd(lig_count + j, acc);
    } else {
        const int i = (role - W) * 64 + lane;
        if (i >= R) return;
        for (int p = blockIdx.y; p < n; p += gridDim.y) {
            if (!member[p]) continue;
            uint64_t any = 0;
            for (int w = 0; w < W; ++w) any |= bits[((int64_t)p * W + w) * R + i];
            acc += any != 0 ? 1 : 0;
        }
        if (acc != 0) atomicAdd(rec_count + i, acc);
    }
}

__global__ __launch_bounds__(64 * SW) void k_contact_score(const uint64_t *__restrict__ bits, const int32_t *__restrict__ count, int n, int R,
                                                           int L, int W, int32_t *__restrict__ n_contacts, int64_t *__restrict__ score_sum)
{
    const int lane = threadIdx.x & 63, p = blockIdx.x * SW + (threadIdx.x >> 6);
    if (p >= n) return;
    const int64_t words = (int64_t)W * R;
    const uint64_t *__restrict__ mine = bits + (int64_t)p * words;
    long long s = 0;
    int c = 0;
    for (int64_t q = lane; q < words; q += 64) {
        uint64_t word = mine[q];
        if (word == 0) continue;
        const int w = (int)(q / R), i = (int)(q % R);
        const int32_t *__restrict__ row = count + (int64_t)i * L + w * 64;
        c += __popcll(word);
        while (word != 0) {
            s += (long long)row[__ffsll((unsigned long long)word) - 1];
            word &= word - 1;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        n_contacts[p] = c;
        score_sum[p] = (int64_t)s;
    }
}

hipError_t launch_contact_bits(const float *rec, const float *lig, int n, int R, int L, float cutoff, uint64_t *bits, hipStream_t s)
{
    const int W = (L + 63) / 64, IB = (R + 63) / 64;
    hipLaunchKernelGGL(k_contact_bits, dim3((unsigned)(W * IB), (unsigned)n), dim3(64), token_lds(), s, rec, lig, R, L, W, cutoff,
                       (double)cutoff, bits);
    return hipGetLastError();
}

hipError_t launch_contact_count(const uint64_t *bits, const uint8_t *member, int n, int R, int L, int32_t *count, int32_t *rec_count,
                                int32_t *lig_count, hipStream_t s)
{
    const int W = (L + 63) / 64, IB = (R + 63) / 64;
    // enough waves to fill the device, at least 8 poses per slice so that the counters' atomics stay a small share of the work
    auto slices = [n](int per_pose) {
        const int want = (8 * 4 * device_cus() + per_pose - 1) / per_pose, most = (n + 7) / 8;
        return (unsigned)(want < 1 ? 1 : (want > most ? most : want));
    };
    hipLaunchKernelGGL(k_contact_count, dim3((unsigned)(W * IB), slices(W * IB)), dim3(64), token_lds(), s, bits, member, n, R, L, W, count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_contact_marginals, dim3((unsigned)(W + IB), slices(W + IB)), dim3(64), token_lds(), s, bits, member, n, R, L, W,
                       rec_count, lig_count);
    return hipGetLastError();
}

hipError_t launch_contact_score(const uint64_t *bits, const int32_t *count, int n, int R, int L, int32_t *n_contacts, int64_t *score_sum,
                                hipStream_t s)
{
    hipLaunchKernelGGL(k_contact_score, dim3((unsigned)((n + SW - 1) / SW)), dim3(64 * SW), token_lds(), s, bits, count, n, R, L,
                       (L + 63) / 64, n_contacts, score_sum);
    return hipGetLastError();
}

}  // namespace dfm
