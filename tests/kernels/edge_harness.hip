// edge_harness.hip - test-only host shim around the message-kernel launchers of libdfmdock_amd.so (tests/edge_harness.py builds it).
//
// Host code only: no kernels here.  The guard-band protocol is harness_common.h's; this file fills a host dfm::LayerDev / dfm::EdgeArgs
// whose pointers are the blocks.  The in / out blocks (out = 2) are agg (zero or sentinel), a message buffer for the coordinate
// kernel, the task counters and the row counters.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

// buffer slots of one call (tests/edge_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_A, S_BM, S_BMB, S_AH, S_EDGES, S_CODES, S_RADIAL, S_CA4,
    S_T, S_T2B, S_W2T, S_W2F, S_W2F16, S_B2, S_B2P, S_B2P16, S_ATT_W, S_W_R, S_W_R_S,
    S_WC1T, S_WC1F, S_WC1F16, S_BC1, S_BC1P, S_BC1P16, S_WC2, S_WC2_S,
    S_ROWS, S_N_ROWS, S_TABLE, S_X, S_SRC,
    S_AGG, S_FOUT, S_MBUF, S_TASK_CTR, S_RANGE, S_ROWS_OUT, S_COUNTER, S_MISS_TOTAL, N_SLOTS
};

// (eh_validate takes the first three)
enum Op { OP_EDGE_BF16, OP_COORD_BF16, OP_EDGE_F32, OP_EDGE_ROWS, OP_EDGE_ROWS32, OP_L0_GATHER, OP_L0_GATHER32 };

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    long long ab_bstride;
    float att_b;
    int B, N, R, K, last, f16, lig_only, agg_is_zero, n_rows_cap, repeat;
};

HARNESS_EXPORTS(Call)

static float g_last_ms = 0.f;
// GPU time of the last kh_run's launches (all `repeat` of them, between two events on the shim's stream), in ms
float eh_last_ms() { return g_last_ms; }

// the CU count the launchers size their grids and task forms by (256 without a device)
int eh_device_cus() { return dfm::device_cus(); }

int eh_tile_tasks(int B, int N, int K) { return dfm::edge_msg_tile_tasks(B, N, K) ? 1 : 0; }

// Argument validation only: every device pointer null, so a launcher that accepted the shape would have nothing to run on.  Without a
// device the launch itself fails; with one, the launch is recorded into a stream capture that is discarded, never executed.
int eh_validate(int op, int B, int N, int R, int K, int last, int lig_only)
{
    static dfm::LayerDev lw;
    dfm::EdgeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.B = B; a.N = N; a.R = R; a.K = K; a.last = last; a.lig_only = lig_only; a.lw = &lw;
    a.agg_is_zero = 1;      // (no memset of a null agg: the control shapes must reach the kernel launch)
    auto launch = [&](hipStream_t s) {
        return op == OP_EDGE_BF16 ? dfm::launch_edge_bf16(a, s) : op == OP_COORD_BF16 ? dfm::launch_coord_bf16(a, s) : dfm::launch_edge_f32(a, s);
    };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return (int)launch(nullptr);
    hipStream_t s;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) return (int)e;
    e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { (void)hipStreamDestroy(s); return (int)e; }
    const hipError_t r = launch(s);
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(s, &g);
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    (void)hipStreamDestroy(s);
    return (int)r;
}

// The launch runs `repeat` times (at least once) on the same buffers.
int kh_run(const Call *c, int op)
{
    harness::Blocks<N_SLOTS> blk(c->buf);
    auto P = [&](int i) { return blk.ptr(i); };
    dfm::LayerDev lw;
    std::memset(&lw, 0, sizeof(lw));
    lw.T = (float *)P(S_T); lw.T2b = (uint16_t *)P(S_T2B); lw.W2t = (float *)P(S_W2T); lw.W2f = (uint16_t *)P(S_W2F);
    lw.W2f16 = (uint16_t *)P(S_W2F16); lw.b2 = (float *)P(S_B2); lw.b2p = (uint32_t *)P(S_B2P); lw.b2p16 = (uint32_t *)P(S_B2P16);
    lw.att_w = (float *)P(S_ATT_W); lw.att_b = c->att_b; lw.w_r = (float *)P(S_W_R); lw.w_r_s = (float *)P(S_W_R_S);
    lw.Wc1t = (float *)P(S_WC1T); lw.Wc1f = (uint16_t *)P(S_WC1F); lw.Wc1f16 = (uint16_t *)P(S_WC1F16); lw.bc1 = (float *)P(S_BC1);
    lw.bc1p = (uint32_t *)P(S_BC1P); lw.bc1p16 = (uint32_t *)P(S_BC1P16); lw.wc2 = (float *)P(S_WC2); lw.wc2_s = (float *)P(S_WC2_S);
    dfm::EdgeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.A = (const float *)P(S_A); a.Bm = (const float *)P(S_BM); a.Bmb = (const uint16_t *)P(S_BMB); a.Ah = (const uint16_t *)P(S_AH);
    a.ab_bstride = c->ab_bstride; a.edges = (const int32_t *)P(S_EDGES); a.codes = (const uint32_t *)P(S_CODES);
    a.radial = (const float *)P(S_RADIAL); a.ca4 = (const float4 *)P(S_CA4);
    a.B = c->B; a.N = c->N; a.R = c->R; a.K = c->K; a.lw = &lw;
    a.agg = (float *)P(S_AGG); a.last = c->last; a.fout = (float *)P(S_FOUT); a.mbuf = (uint16_t *)P(S_MBUF); a.f16 = c->f16;
    a.lig_only = c->lig_only; a.agg_is_zero = c->agg_is_zero; a.range = (uint32_t *)P(S_RANGE); a.task_ctr = (uint32_t *)P(S_TASK_CTR);
    const uint4 *rows = (const uint4 *)P(S_ROWS);
    const uint32_t *n_rows = (const uint32_t *)P(S_N_ROWS);
    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], s);
    for (int rep = 0; rep < (c->repeat > 1 ? c->repeat : 1) && e == hipSuccess; ++rep) {
        switch (op) {
        case OP_EDGE_BF16: e = dfm::launch_edge_bf16(a, s); break;
        case OP_COORD_BF16: e = dfm::launch_coord_bf16(a, s); break;
        case OP_EDGE_F32: e = dfm::launch_edge_f32(a, s); break;
        case OP_EDGE_ROWS: e = dfm::launch_edge_rows(a, rows, n_rows, (uint32_t)c->n_rows_cap, (uint16_t *)P(S_ROWS_OUT), s); break;
        case OP_EDGE_ROWS32: e = dfm::launch_edge_rows32(a, rows, n_rows, (uint32_t)c->n_rows_cap, (float *)P(S_ROWS_OUT), s); break;
        case OP_L0_GATHER:
            e = dfm::launch_l0_gather((const uint16_t *)P(S_TABLE), (const uint16_t *)P(S_X), (const uint32_t *)P(S_SRC), a.agg, a.B, a.N,
                                      a.K, (uint32_t *)P(S_COUNTER), (unsigned long long *)P(S_MISS_TOTAL), s);
            break;
        case OP_L0_GATHER32:
            e = dfm::launch_l0_gather32((const float *)P(S_TABLE), (const float *)P(S_X), (const uint32_t *)P(S_SRC), a.agg, a.B, a.N,
                                        a.K, (uint32_t *)P(S_COUNTER), (unsigned long long *)P(S_MISS_TOTAL), s);
            break;
        default: e = hipErrorInvalidValue;
        }
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], s);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&g_last_ms, ev[0], ev[1]);
    for (int k = 0; k < 2; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    return (int)blk.finish(e);
}

}  // extern "C"
