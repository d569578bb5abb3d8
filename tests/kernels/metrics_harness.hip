// metrics_harness.hip - test-only host shim around the docking-metrics launchers of libdfmdock_amd.so (tests/metrics_harness.py builds
// it): dfm::launch_native_pairs, launch_metrics_reduce, launch_metrics_finish.
//
// Host code only: no kernels here.  The guard-band protocol is harness_common.h's.  BEFORE anything is uploaded this file checks that
// every array is large enough for the launch it feeds and that the contact indices are in range (a failure is hipErrorInvalidValue
// and no device is touched); then it fills dfm::MetricsChain / dfm::MetricsConst from the call record.  Every output is out = 1.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

// buffer slots of one call (tests/metrics_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_REC_NAT, S_LIG_NAT, S_REC_MODEL, S_LIG_MODEL, S_FREC, S_FLIG, S_CONTACTS, S_REC_CONST, S_SUMS, S_XF, S_RMSD, S_RECOVERED, S_PAIRS,
    N_SLOTS
};

enum Op { OP_NATIVE_PAIRS, OP_REDUCE, OP_FINISH, OP_FULL };

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    double iface_cutoff, contact_cutoff;
    double T_rec[3], T_lig[3], T_rec_iface[3], T_lig_iface[3], o[3];
    // R, L: the chain lengths of the arrays; n_*: the counts k_metrics_solve / k_metrics_resid divide by (the test may set them apart)
    int P, R, L, chains, n_rec, n_lig, n_rec_iface, n_lig_iface, n_contacts, rec_moves;
};

HARNESS_EXPORTS(Call)

int kh_run(const Call *c, int op)
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

    harness::Blocks<N_SLOTS> blk(c->buf);
    auto D = [&](int i) { return blk.ptr(i); };

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

    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess && op == OP_NATIVE_PAIRS)
        e = dfm::launch_native_pairs(rec.native, lig.native, c->R, c->L, c->iface_cutoff, c->contact_cutoff, (uint8_t *)D(S_PAIRS), s);
    if (e == hipSuccess && (op == OP_REDUCE || op == OP_FULL)) e = dfm::launch_metrics_reduce(lig, rec, c->chains, c->P, mc, (double *)D(S_SUMS), s);
    if (e == hipSuccess && (op == OP_FINISH || op == OP_FULL))
        e = dfm::launch_metrics_finish(lig, rec, (const double *)D(S_SUMS), c->chains, (const double *)D(S_REC_CONST), mc,
                                       (const int32_t *)D(S_CONTACTS), c->P, (double *)D(S_XF), (double *)D(S_RMSD), (int32_t *)D(S_RECOVERED), s);
    return (int)blk.finish(e);
}

}  // extern "C"
