// dense_harness.hip - test-only host shim around the node-model launchers of libdfmdock_amd.so (tests/dense_harness.py builds it):
// dfm::launch_gemm_split, launch_gemm_f32 and launch_gn_stats.
//
// Host code only: no kernels here.  The guard-band protocol is harness_common.h's; this file fills a dfm::GemmArgs from the call record.
// Every output is out = 1: its interior starts as the sentinel.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

// buffer slots of one call (the GemmArgs pointer each one becomes)
enum Slot {
    S_A0, S_A1, S_W, S_WHI, S_WLO, S_BIAS, S_GN_SHIFT, S_GN_DEN, S_GN_W, S_GN_B, S_GN_PART, S_GN_MS, S_R,
    S_C, S_C2, S_C2B, S_CB, S_STAT, S_ZBUF, N_SLOTS
};

enum Op { OP_SPLIT, OP_F32, OP_GN_STATS };

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    int M, K, Nout, lda, ldw, ldc, pro, epi, rows_per_graph, a0_period, r_period;
    int a0_offset;      // bytes added to the A0 device pointer (4: an unaligned launch of launch_gemm_f32)
    int gn_B, gn_N;     // launch_gn_stats: trajectories, rows per trajectory (u = A0, mean_scale = GN_MS, fold = GN_W / GN_B,
                        // shift -> C, den -> C2)
};

HARNESS_EXPORTS(Call)

int dh_device_cus(int *cus)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
    return (int)e;
}

// Argument validation only: every pointer null, so a launcher that accepted the shape would have nothing to run on.  Without a device
// the launch itself fails; with one, the launch is recorded into a stream capture that is discarded, never executed.
int dh_validate_split(int M, int K, int Nout, int lda, int ldc, int pro, int epi, int rows_per_graph, int stats, int zbuf)
{
    dfm::GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.M = M; a.K = K; a.Nout = Nout; a.lda = lda; a.ldw = K; a.ldc = ldc; a.pro = pro; a.epi = epi; a.rows_per_graph = rows_per_graph;
    // non-null markers that are never dereferenced: the launcher's checks look at whether these are set
    static float marker[4];
    if (stats) a.stat_part = marker;
    if (zbuf) a.zbuf = marker;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return (int)dfm::launch_gemm_split(a, nullptr, nullptr, nullptr);
    hipStream_t s;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) return (int)e;
    e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { (void)hipStreamDestroy(s); return (int)e; }
    const hipError_t r = dfm::launch_gemm_split(a, nullptr, nullptr, s);
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(s, &g);
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    (void)hipStreamDestroy(s);
    return (int)r;
}

int kh_run(const Call *c, int op)
{
    harness::Blocks<N_SLOTS> blk(c->buf);
    auto P = [&](int i) { return blk.ptr(i); };
    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess) {
        if (op == OP_GN_STATS) {
            e = dfm::launch_gn_stats((const float *)P(S_A0), c->gn_B, c->gn_N, (const float *)P(S_GN_MS), (float *)P(S_C),
                                     (float *)P(S_C2), (const float *)P(S_GN_W), (const float *)P(S_GN_B), s);
        } else if (op == OP_SPLIT || op == OP_F32) {
            dfm::GemmArgs a;
            std::memset(&a, 0, sizeof(a));
            a.A0 = (const float *)((char *)P(S_A0) + c->a0_offset);
            a.A1 = (const float *)P(S_A1);
            a.lda = c->lda; a.K = c->K; a.W = (const float *)P(S_W); a.ldw = c->ldw; a.bias = (const float *)P(S_BIAS);
            a.M = c->M; a.Nout = c->Nout; a.pro = c->pro;
            a.gn_shift = (const float *)P(S_GN_SHIFT); a.gn_den = (const float *)P(S_GN_DEN);
            a.gn_w = (const float *)P(S_GN_W); a.gn_b = (const float *)P(S_GN_B); a.rows_per_graph = c->rows_per_graph;
            a.epi = c->epi; a.R = (const float *)P(S_R); a.C = (float *)P(S_C); a.ldc = c->ldc; a.C2 = (float *)P(S_C2);
            a.C2b = (uint16_t *)P(S_C2B); a.Cb = (uint16_t *)P(S_CB); a.stat_part = (float *)P(S_STAT);
            a.gn_part = (const float *)P(S_GN_PART); a.gn_ms = (const float *)P(S_GN_MS); a.zbuf = (float *)P(S_ZBUF);
            a.a0_period = c->a0_period; a.r_period = c->r_period;
            e = op == OP_SPLIT ? dfm::launch_gemm_split(a, (const uint16_t *)P(S_WHI), (const uint16_t *)P(S_WLO), s)
                               : dfm::launch_gemm_f32(a, s);
        } else {
            e = hipErrorInvalidValue;
        }
    }
    return (int)blk.finish(e);
}

}  // extern "C"
