// edge_harness.hip - test-only host shim around the message-kernel launchers of libdfmdock_amd.so (tests/edge_harness.py builds it).
//
// Host code only: no kernels here.  Every entry point takes host arrays, uploads each into a device block with GUARD bytes of
// sentinel (0xff: a NaN as fp32 and as fp16) before and after it, fills a host dfm::LayerDev / dfm::EdgeArgs whose pointers are those
// blocks, calls the SHIPPED launcher on a stream of its own, synchronises and copies the outputs back WITH their guard bands.  An
// output block's interior starts as the sentinel (out = 1) or as the caller's own contents (out = 2: agg zero or sentinel, a message
// buffer for the coordinate kernel, task counters, row counters).  Each entry point returns the hipError_t.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../dfmdock_amd/csrc/dfm_internal.h"

namespace {

constexpr size_t GUARD = 4096;      // bytes of sentinel on each side of a block
constexpr unsigned char SENTINEL = 0xff;

// buffer slots of one call (tests/edge_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_A, S_BM, S_BMB, S_AH, S_EDGES, S_CODES, S_RADIAL, S_CA4,
    S_T, S_T2B, S_W2T, S_W2F, S_W2F16, S_B2, S_B2P, S_B2P16, S_ATT_W, S_W_R, S_W_R_S,
    S_WC1T, S_WC1F, S_WC1F16, S_BC1, S_BC1P, S_BC1P16, S_WC2, S_WC2_S,
    S_ROWS, S_N_ROWS, S_TABLE, S_X, S_SRC,
    S_AGG, S_FOUT, S_MBUF, S_TASK_CTR, S_RANGE, S_ROWS_OUT, S_COUNTER, S_MISS_TOTAL, N_SLOTS
};

}  // namespace

extern "C" {

// One host buffer.  out 0: input, `bytes` bytes at host.  out 1 / 2: host holds GUARD + bytes + GUARD bytes and receives the whole
// device block, guards included; out 2 also uploads the interior host[GUARD .. GUARD + bytes) first.  host == nullptr: unused (nullptr).
struct EhBuf {
    void *host;
    long long bytes;
    int out;
};

struct EhCall {
    EhBuf buf[N_SLOTS];
    long long ab_bstride;
    float att_b;
    int B, N, R, K, last, f16, lig_only, agg_is_zero, n_rows_cap, repeat;
};

long long eh_guard_bytes() { return (long long)GUARD; }

static float g_last_ms = 0.f;
// GPU time of the last eh_run's launches (all `repeat` of them, between two events on the shim's stream), in ms
float eh_last_ms() { return g_last_ms; }

// the CU count the launchers size their grids and task forms by (256 without a device)
int eh_device_cus() { return dfm::device_cus(); }

int eh_tile_tasks(int B, int N, int K) { return dfm::edge_msg_tile_tasks(B, N, K) ? 1 : 0; }

// Argument validation only: every device pointer null, so a launcher that accepted the shape would have nothing to run on.  Without a
// device the launch itself fails; with one, the launch is recorded into a stream capture that is discarded, never executed.
// op: 0 launch_edge_bf16, 1 launch_coord_bf16, 2 launch_edge_f32.
int eh_validate(int op, int B, int N, int R, int K, int last, int lig_only)
{
    static dfm::LayerDev lw;
    dfm::EdgeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.B = B; a.N = N; a.R = R; a.K = K; a.last = last; a.lig_only = lig_only; a.lw = &lw;
    a.agg_is_zero = 1;      // (no memset of a null agg: the control shapes must reach the kernel launch)
    auto launch = [&](hipStream_t s) {
        return op == 0 ? dfm::launch_edge_bf16(a, s) : op == 1 ? dfm::launch_coord_bf16(a, s) : dfm::launch_edge_f32(a, s);
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

// op: 0 launch_edge_bf16, 1 launch_coord_bf16, 2 launch_edge_f32, 3 launch_edge_rows, 4 launch_edge_rows32, 5 launch_l0_gather,
// 6 launch_l0_gather32.  The launch runs `repeat` times (at least once) on the same buffers.
int eh_run(const EhCall *c, int op)
{
    void *dev[N_SLOTS] = {};
    hipError_t e = hipSuccess;
    hipStream_t s = nullptr;
    for (int i = 0; i < N_SLOTS && e == hipSuccess; ++i) {
        const EhBuf &b = c->buf[i];
        if (!b.host) continue;
        const size_t total = GUARD + (size_t)b.bytes + GUARD;
        if ((e = hipMalloc(&dev[i], total)) != hipSuccess) break;
        if ((e = hipMemset(dev[i], SENTINEL, total)) != hipSuccess) break;
        if (b.out == 0) e = hipMemcpy((char *)dev[i] + GUARD, b.host, (size_t)b.bytes, hipMemcpyHostToDevice);
        else if (b.out == 2) e = hipMemcpy((char *)dev[i] + GUARD, (const char *)b.host + GUARD, (size_t)b.bytes, hipMemcpyHostToDevice);
    }
    auto P = [&](int i) -> void * { return dev[i] ? (char *)dev[i] + GUARD : nullptr; };
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
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    const uint4 *rows = (const uint4 *)P(S_ROWS);
    const uint32_t *n_rows = (const uint32_t *)P(S_N_ROWS);
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], s);
    for (int rep = 0; rep < (c->repeat > 1 ? c->repeat : 1) && e == hipSuccess; ++rep) {
        switch (op) {
        case 0: e = dfm::launch_edge_bf16(a, s); break;
        case 1: e = dfm::launch_coord_bf16(a, s); break;
        case 2: e = dfm::launch_edge_f32(a, s); break;
        case 3: e = dfm::launch_edge_rows(a, rows, n_rows, (uint32_t)c->n_rows_cap, (uint16_t *)P(S_ROWS_OUT), s); break;
        case 4: e = dfm::launch_edge_rows32(a, rows, n_rows, (uint32_t)c->n_rows_cap, (float *)P(S_ROWS_OUT), s); break;
        case 5:
            e = dfm::launch_l0_gather((const uint16_t *)P(S_TABLE), (const uint16_t *)P(S_X), (const uint32_t *)P(S_SRC), a.agg, a.B, a.N,
                                      a.K, (uint32_t *)P(S_COUNTER), (unsigned long long *)P(S_MISS_TOTAL), s);
            break;
        case 6:
            e = dfm::launch_l0_gather32((const float *)P(S_TABLE), (const float *)P(S_X), (const uint32_t *)P(S_SRC), a.agg, a.B, a.N,
                                        a.K, (uint32_t *)P(S_COUNTER), (unsigned long long *)P(S_MISS_TOTAL), s);
            break;
        default: e = hipErrorInvalidValue;
        }
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], s);
    if (s) {
        const hipError_t e2 = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e2;
        (void)hipStreamDestroy(s);
    }
    if (e == hipSuccess) e = hipEventElapsedTime(&g_last_ms, ev[0], ev[1]);
    for (int k = 0; k < 2; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    for (int i = 0; i < N_SLOTS && e == hipSuccess; ++i)
        if (dev[i] && c->buf[i].out)
            e = hipMemcpy(c->buf[i].host, dev[i], GUARD + (size_t)c->buf[i].bytes + GUARD, hipMemcpyDeviceToHost);
    for (int i = 0; i < N_SLOTS; ++i)
        if (dev[i]) (void)hipFree(dev[i]);
    return (int)e;
}

}  // extern "C"
