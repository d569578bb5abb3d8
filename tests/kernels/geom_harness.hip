// geom_harness.hip - test-only host shim around the graph front end and the pose kernels of libdfmdock_amd.so (kernels_geom.hip):
// dfm::launch_knn_sample, launch_edge_feat (with and without the table classification), launch_l0_pairs, launch_init_pose and
// launch_clash_force (tests/geom_harness.py builds it).
//
// Host code, plus ONE test-only kernel (k_hw_log2: the hardware log2 the sampling race uses, evaluated on a given array, so that its
// error is measured on the instruction itself and not on the kernel under test).  The guard-band protocol is harness_common.h's.  The
// in / out blocks (out = 2) are the pose and the accumulated update k_clash_force changes in place, and the row counter.
// The host versions of philox4x32, u01 and pack_code (they are __host__ __device__) are exported for the CPU tests.
#include <hip/hip_runtime.h>

#include "../../dfmdock_amd/csrc/dfm_device.h"
#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

// buffer slots of one call (tests/geom_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_N4, S_CA4, S_CB4, S_EDGES, S_CTL, S_CODES, S_RADIAL, S_CODE0, S_SRC, S_ROWS, S_COUNTER, S_EVAL_CTR,
    S_REC_POS, S_LIG0, S_R0, S_TR_DRAW, S_LIG_CUR, S_TR_UPD, S_ROT_UPD, S_LOG_IN, S_LOG_OUT, N_SLOTS
};

enum Op { OP_KNN_SAMPLE, OP_EDGE_FEAT, OP_L0_PAIRS, OP_INIT_POSE, OP_CLASH_FORCE, OP_HW_LOG2 };

__global__ __launch_bounds__(256) void k_hw_log2(const float *__restrict__ x, float *__restrict__ y, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __builtin_amdgcn_logf(x[i]);
}

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    long long n;
    unsigned long long seed;
    float mask_dist;
    unsigned stream_id;
    int B, N, R, L, K, knn, nsamp, all_atoms;
};

HARNESS_EXPORTS(Call)

// ---- host versions of the device helpers ----------------------------------------------------------------------------------------
// n Philox blocks: counter words c[4 n], key (k0, k1) -> out[4 n]
void gh_philox(long long n, const unsigned *c, unsigned k0, unsigned k1, unsigned *out)
{
    for (long long i = 0; i < n; ++i) {
        const dfm::u32x4 r = dfm::philox4x32(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3], k0, k1);
        out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
    }
}
void gh_u01(long long n, const unsigned *x, float *out)
{
    for (long long i = 0; i < n; ++i) out[i] = dfm::u01(x[i]);
}
// u01 over all 2^24 values of x >> 8: smallest and largest value; returns 1 when non-decreasing, 2 when strictly increasing, else 0
int gh_u01_scan(float *lo, float *hi)
{
    float prev = dfm::u01(0u), mn = prev, mx = prev;
    int mono = 2;
    for (unsigned v = 1; v < (1u << 24); ++v) {
        const float u = dfm::u01(v << 8);
        if (u < prev) mono = 0;
        else if (u == prev && mono == 2) mono = 1;
        mn = u < mn ? u : mn; mx = u > mx ? u : mx;
        prev = u;
    }
    *lo = mn; *hi = mx;
    return mono;
}
unsigned gh_pack_code(int d, int om, int th, int ph, int rp) { return dfm::pack_code(d, om, th, ph, rp); }
unsigned gh_rng_edges() { return (unsigned)dfm::RNG_EDGES; }
unsigned gh_rng_init() { return (unsigned)dfm::RNG_INIT; }

// Search for a uniform of exactly the top value (x >> 8 == 0xFFFFFF) in the streams  philox(c0, c1, c2, c3; seed)  with
// c0 < n0, c1 = c1_mul * q for q < n1 and, for s < n2, c2 = s (vary_seed 0) or c2 = 0 and seed + s (vary_seed 1): at most max_blocks
// blocks.  found[4] = (s, c0, q, word).
int gh_find_top_uniform(unsigned n0, unsigned n1, unsigned c1_mul, unsigned n2, int vary_seed, unsigned c3, unsigned long long seed,
                        long long max_blocks, unsigned *found)
{
    long long done = 0;
    for (unsigned s = 0; s < n2; ++s) {
        const unsigned long long sd = vary_seed ? seed + s : seed;
        const unsigned k0 = (unsigned)sd, k1 = (unsigned)(sd >> 32);
        for (unsigned a = 0; a < n0; ++a)
            for (unsigned q = 0; q < n1; ++q) {
                if (done++ >= max_blocks) return 0;
                const dfm::u32x4 r = dfm::philox4x32(a, c1_mul * q, vary_seed ? 0u : s, c3, k0, k1);
                const unsigned w[4] = {r.x, r.y, r.z, r.w};
                for (unsigned e = 0; e < 4; ++e)
                    if ((w[e] >> 8) == 0xFFFFFFu) { found[0] = s; found[1] = a; found[2] = q; found[3] = e; return 1; }
            }
    }
    return 0;
}

// ---- one launch -----------------------------------------------------------------------------------------------------------------
int kh_run(const Call *c, int op)
{
    harness::Blocks<N_SLOTS> blk(c->buf);
    auto P = [&](int i) { return blk.ptr(i); };
    auto F = [&](int i) -> float * { return (float *)P(i); };
    auto F4 = [&](int i) -> const float4 * { return (const float4 *)P(i); };

    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess) {
        switch (op) {
        case OP_KNN_SAMPLE:
            e = dfm::launch_knn_sample(F4(S_CA4), c->B, c->N, c->knn, c->nsamp, (uint64_t)c->seed, c->stream_id, (int32_t *)P(S_EDGES),
                                       (const uint32_t *)P(S_CTL), s);
            break;
        case OP_EDGE_FEAT: {
            dfm::L0Classify cls;
            cls.code0 = (const uint2 *)P(S_CODE0); cls.src = (uint32_t *)P(S_SRC); cls.rows = (uint4 *)P(S_ROWS);
            cls.counter = (uint32_t *)P(S_COUNTER);
            e = dfm::launch_edge_feat(F4(S_N4), F4(S_CA4), F4(S_CB4), (const int32_t *)P(S_EDGES), c->B, c->N, c->R, c->K, c->mask_dist,
                                      (uint32_t *)P(S_CODES), F(S_RADIAL), cls, (uint32_t *)P(S_EVAL_CTR), s);
            break;
        }
        case OP_L0_PAIRS:
            e = dfm::launch_l0_pairs(F4(S_N4), F4(S_CA4), F4(S_CB4), c->R, c->L, c->mask_dist, (uint2 *)P(S_CODE0), (uint4 *)P(S_ROWS), s);
            break;
        case OP_INIT_POSE:
            e = dfm::launch_init_pose(F(S_REC_POS), F(S_LIG0), c->B, c->R, c->L, c->all_atoms, F(S_R0), F(S_TR_DRAW), (uint64_t)c->seed,
                                      F(S_LIG_CUR), F(S_TR_UPD), F(S_ROT_UPD), s);
            break;
        case OP_CLASH_FORCE: e = dfm::launch_clash_force(F(S_REC_POS), c->B, c->R, c->L, F(S_LIG_CUR), F(S_TR_UPD), s); break;
        case OP_HW_LOG2:
            hipLaunchKernelGGL(k_hw_log2, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, s, F(S_LOG_IN), F(S_LOG_OUT), c->n);
            e = hipGetLastError();
            break;
        default: e = hipErrorInvalidValue;
        }
    }
    return (int)blk.finish(e);
}

}  // extern "C"
