// metrics_harness.hip - test-only host shim around the docking-metrics launchers of libdfmdock_amd.so (tests/metrics_harness.py builds
// it): dfm::launch_native_pairs, launch_metrics_reduce, launch_metrics_finish.
//
// Host code only: no kernels here.  Every entry point takes host arrays, checks that each is large enough for the launch it feeds (a
// short one is hipErrorInvalidValue and nothing is launched), uploads each into a device block with GUARD bytes of sentinel (0xff) before
// and after it, fills dfm::MetricsChain / dfm::MetricsConst from the call record, calls the SHIPPED launcher on a stream of its own,
// synchronises and copies the outputs back WITH their guard bands.  An output block's interior starts as the sentinel.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../dfmdock_amd/csrc/dfm_internal.h"

namespace {

constexpr size_t GUARD = 4096;      // bytes of sentinel on each side of a block
constexpr unsigned char SENTINEL = 0xff;

// buffer slots of one call (tests/metrics_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_REC_NAT, S_LIG_NAT, S_REC_MODEL, S_LIG_MODEL, S_FREC, S_FLIG, S_CONTACTS, S_REC_CONST, S_SUMS, S_XF, S_RMSD, S_RECOVERED, S_PAIRS,
    N_SLOTS
};

enum Op { OP_NATIVE_PAIRS, OP_REDUCE, OP_FINISH, OP_FULL };

}  // namespace

extern "C" {

// One host buffer.  out 0: input, `bytes` bytes at host.  out 1: host holds GUARD + bytes + GUARD bytes and receives the whole device
// block, guards included.  host == nullptr: unused.
struct MhBuf {
    void *host;
    long long bytes;
    int out;
};

struct MhCall {
    MhBuf buf[N_SLOTS];
    double iface_cutoff, contact_cutoff;
    double T_rec[3], T_lig[3], T_rec_iface[3], T_lig_iface[3], o[3];
    // R, L: the chain lengths of the arrays; n_*: the counts k_metrics_solve / k_metrics_resid divide by (the test may set them apart)
    int P, R, L, chains, n_rec, n_lig, n_rec_iface, n_lig_iface, n_contacts, rec_moves;
};

long long mh_guard_bytes() { return (long long)GUARD; }
long long mh_call_bytes() { return (long long)sizeof(MhCall); }

int mh_run(const MhCall *c, int op)
{
    const long long P = c->P, R = c->R, L = c->L, ch = c->chains;
    auto has = [&](int i, long long bytes) { return c->buf[i].host && c->buf[i].bytes >= bytes; };
    if (R < 1 || L < 1) return (int)hipErrorInvalidValue;
    bool ok = has(S_REC_NAT, R * 36) && has(S_LIG_NAT, L * 36);
    if (op == OP_NATIVE_PAIRS) {
        ok = ok && has(S_PAIRS, R * L) && c->buf[S_PAIRS].out == 1;
    } else if (op == OP_REDUCE || op == OP_FINISH || op == OP_FULL) {
        ok = ok && P >= 1 && (ch == 1 || ch == 2) && has(S_LIG_MODEL, P * L * 36) && has(S_FLIG, L) && has(S_FREC, R) && has(S_SUMS, P * ch * 192);
        if (ch == 2 || op != OP_REDUCE) ok = ok && has(S_REC_MODEL, (c->rec_moves ? P : 1) * R * 36);
        if (ch == 2) ok = ok && c->rec_moves == 1;
        if (op != OP_FINISH) ok = ok && c->buf[S_SUMS].out == 1;
        if (op != OP_REDUCE) {
            ok = ok && c->n_contacts >= 0 && has(S_CONTACTS, (long long)c->n_contacts * 8) && has(S_XF, P * 288) && has(S_RMSD, P * 24) &&
                 has(S_RECOVERED, P * 4) && (ch == 2 || (has(S_REC_CONST, 192) && c->rec_moves == 0)) && c->buf[S_XF].out == 1 &&
                 c->buf[S_RMSD].out == 1 && c->buf[S_RECOVERED].out == 1 && c->buf[S_CONTACTS].out == 0;
            if (ok) {      // the residue indices k_metrics_resid follows into the poses
                const int32_t *ct = (const int32_t *)c->buf[S_CONTACTS].host;
                for (int k = 0; k < c->n_contacts; ++k) ok = ok && ct[2 * k] >= 0 && ct[2 * k] < R && ct[2 * k + 1] >= 0 && ct[2 * k + 1] < L;
            }
        }
    } else {
        ok = false;
    }
    if (!ok) return (int)hipErrorInvalidValue;

    void *dev[N_SLOTS] = {};
    hipError_t e = hipSuccess;
    hipStream_t s = nullptr;
    for (int i = 0; i < N_SLOTS && e == hipSuccess; ++i) {
        const MhBuf &b = c->buf[i];
        if (!b.host) continue;
        const size_t total = GUARD + (size_t)b.bytes + GUARD;
        if ((e = hipMalloc(&dev[i], total)) != hipSuccess) break;
        if ((e = hipMemset(dev[i], SENTINEL, total)) != hipSuccess) break;
        if (b.out == 0 && b.bytes > 0) e = hipMemcpy((char *)dev[i] + GUARD, b.host, (size_t)b.bytes, hipMemcpyHostToDevice);
    }
    auto D = [&](int i) -> void * { return dev[i] ? (char *)dev[i] + GUARD : nullptr; };

    const dfm::MetricsChain lig = {(const float *)D(S_LIG_MODEL), (const float *)D(S_LIG_NAT), (const uint8_t *)D(S_FLIG), c->L};
    const dfm::MetricsChain rec = {(const float *)D(S_REC_MODEL), (const float *)D(S_REC_NAT), (const uint8_t *)D(S_FREC), c->R};
    dfm::MetricsConst mc;
    std::memset(&mc, 0, sizeof(mc));
    mc.n_rec = c->n_rec; mc.n_lig = c->n_lig; mc.n_rec_iface = c->n_rec_iface; mc.n_lig_iface = c->n_lig_iface;
    mc.n_contacts = c->n_contacts; mc.rec_moves = c->rec_moves; mc.contact_cutoff = c->contact_cutoff;
    for (int k = 0; k < 3; ++k) {
        mc.T_rec[k] = c->T_rec[k]; mc.T_lig[k] = c->T_lig[k]; mc.T_rec_iface[k] = c->T_rec_iface[k]; mc.T_lig_iface[k] = c->T_lig_iface[k];
        mc.o[k] = c->o[k];
    }

    // the fills and uploads above went through the null stream, which a non-blocking stream does not wait for
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess && op == OP_NATIVE_PAIRS)
        e = dfm::launch_native_pairs(rec.native, lig.native, c->R, c->L, c->iface_cutoff, c->contact_cutoff, (uint8_t *)D(S_PAIRS), s);
    if (e == hipSuccess && (op == OP_REDUCE || op == OP_FULL)) e = dfm::launch_metrics_reduce(lig, rec, c->chains, c->P, mc, (double *)D(S_SUMS), s);
    if (e == hipSuccess && (op == OP_FINISH || op == OP_FULL))
        e = dfm::launch_metrics_finish(lig, rec, (const double *)D(S_SUMS), c->chains, (const double *)D(S_REC_CONST), mc,
                                       (const int32_t *)D(S_CONTACTS), c->P, (double *)D(S_XF), (double *)D(S_RMSD), (int32_t *)D(S_RECOVERED), s);
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

}  // extern "C"
