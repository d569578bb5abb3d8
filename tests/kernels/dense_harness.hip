// dense_harness.hip - test-only host shim around the node-model launchers of libdfmdock_amd.so (tests/dense_harness.py builds it).
//
// Host code only: no kernels here.  Every entry point takes host arrays, uploads each into a device block with GUARD bytes of
// sentinel (0xff: a NaN as fp32 and as fp16) before and after it, fills a dfm::GemmArgs, calls the SHIPPED launcher on a stream of its
// own, synchronises and copies the outputs back WITH their guard bands.  The interior of every output block starts as the sentinel too,
// so an element the kernel should have written and did not is visible as well.  Each entry point returns the hipError_t.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../dfmdock_amd/csrc/dfm_internal.h"

namespace {

constexpr size_t GUARD = 4096;      // bytes of sentinel on each side of a block
constexpr unsigned char SENTINEL = 0xff;

// buffer slots of one call (the GemmArgs pointer each one becomes)
enum Slot {
    S_A0, S_A1, S_W, S_WHI, S_WLO, S_BIAS, S_GN_SHIFT, S_GN_DEN, S_GN_W, S_GN_B, S_GN_PART, S_GN_MS, S_R,
    S_C, S_C2, S_C2B, S_CB, S_STAT, S_ZBUF, N_SLOTS
};

}  // namespace

extern "C" {

// One host buffer.  Inputs: `bytes` bytes at host.  Outputs (out != 0): host holds GUARD + bytes + GUARD bytes and receives the whole
// device block, guards included.  host == nullptr: the slot is unused (nullptr in GemmArgs).
struct DhBuf {
    void *host;
    long long bytes;
    int out;
};

struct DhCall {
    DhBuf buf[N_SLOTS];
    int M, K, Nout, lda, ldw, ldc, pro, epi, rows_per_graph, a0_period, r_period;
    int a0_offset;      // bytes added to the A0 device pointer (4: an unaligned launch of launch_gemm_f32)
    int gn_B, gn_N;     // launch_gn_stats: trajectories, rows per trajectory (u = A0, mean_scale = GN_MS, fold = GN_W / GN_B,
                        // shift -> C, den -> C2)
};

long long dh_guard_bytes() { return (long long)GUARD; }

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

static int run(const DhCall *c, int op)
{
    void *dev[N_SLOTS] = {};
    hipError_t e = hipSuccess;
    hipStream_t s = nullptr;
    dfm::GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int i = 0; i < N_SLOTS && e == hipSuccess; ++i) {
        const DhBuf &b = c->buf[i];
        if (!b.host) continue;
        const size_t total = GUARD + (size_t)b.bytes + GUARD;
        if ((e = hipMalloc(&dev[i], total)) != hipSuccess) break;
        if ((e = hipMemset(dev[i], SENTINEL, total)) != hipSuccess) break;
        if (!b.out) e = hipMemcpy((char *)dev[i] + GUARD, b.host, (size_t)b.bytes, hipMemcpyHostToDevice);
    }
    auto P = [&](int i) -> void * { return dev[i] ? (char *)dev[i] + GUARD : nullptr; };
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) {
        if (op == 2) {
            e = dfm::launch_gn_stats((const float *)P(S_A0), c->gn_B, c->gn_N, (const float *)P(S_GN_MS), (float *)P(S_C),
                                     (float *)P(S_C2), (const float *)P(S_GN_W), (const float *)P(S_GN_B), s);
        } else {
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
            e = op == 0 ? dfm::launch_gemm_split(a, (const uint16_t *)P(S_WHI), (const uint16_t *)P(S_WLO), s)
                        : dfm::launch_gemm_f32(a, s);
        }
    }
    if (s) {
        const hipError_t e2 = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e2;
        (void)hipStreamDestroy(s);
    }
    for (int i = 0; i < N_SLOTS && e == hipSuccess; ++i)
        if (dev[i] && c->buf[i].out)
            e = hipMemcpy(c->buf[i].host, dev[i], GUARD + (size_t)c->buf[i].bytes + GUARD, hipMemcpyDeviceToHost);
    for (int i = 0; i < N_SLOTS; ++i)
        if (dev[i]) (void)hipFree(dev[i]);
    return (int)e;
}

int dh_gemm_split(const DhCall *c) { return run(c, 0); }
int dh_gemm_f32(const DhCall *c) { return run(c, 1); }
int dh_gn_stats(const DhCall *c) { return run(c, 2); }

}  // extern "C"
