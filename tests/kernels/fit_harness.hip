// fit_harness.hip - test-only host shim around the rigid-pose-fit launchers of libdfmdock_amd.so (tests/fit_harness.py builds it):
// dfm::launch_fit_reduce, launch_fit_solve, launch_fit_resid.
//
// Host code only: no kernels here.  The guard-band protocol is harness_common.h's.  BEFORE anything is uploaded this file checks that
// every array is large enough for the launch it feeds (a failure is hipErrorInvalidValue and no device is touched); then it fills
// dfm::FitChain from the call record.  R = 0: the decoys bring no receptor.  Every output is out = 1; `solve` alone reads the sums, and
// `resid` alone the xf, that a test hands it as inputs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

// buffer slots of one call (tests/fit_harness.py SLOTS lists the same names in the same order)
enum Slot { S_LIG_REF, S_LIG_POS, S_REC_REF, S_REC_POS, S_SUMS, S_XF, S_ROT, S_TR, S_RMSD, S_REC_RMSD, N_SLOTS };

enum Op { OP_REDUCE, OP_SOLVE, OP_RESID, OP_FULL };

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    double o[3];
    int P, L, R;
};

HARNESS_EXPORTS(Call)

int kh_run(const Call *c, int op)
{
    const long long P = c->P, L = c->L, R = c->R, ch = R > 0 ? 2 : 1;
    auto has = [&](int i, long long bytes) { return c->buf[i].host && c->buf[i].bytes >= bytes; };
    auto is_out = [&](int i) { return c->buf[i].out == 1; };
    if (P < 1 || L < 1 || R < 0 || op < OP_REDUCE || op > OP_FULL) return (int)hipErrorInvalidValue;
    const bool reduce = op == OP_REDUCE || op == OP_FULL, solve = op == OP_SOLVE || op == OP_FULL, resid = op == OP_RESID || op == OP_FULL;
    bool ok = true;
    if (reduce || solve) ok = ok && has(S_SUMS, P * ch * 15 * 8);
    if (reduce || resid) {
        ok = ok && has(S_LIG_REF, L * 36) && has(S_LIG_POS, P * L * 36);
        if (R > 0) ok = ok && has(S_REC_REF, R * 36) && has(S_REC_POS, P * R * 36);
    }
    if (reduce) ok = ok && is_out(S_SUMS);
    if (solve) ok = ok && has(S_XF, P * 24 * 8) && has(S_ROT, P * 12) && has(S_TR, P * 12) && is_out(S_XF) && is_out(S_ROT) && is_out(S_TR);
    if (resid) ok = ok && has(S_XF, P * 24 * 8) && has(S_RMSD, P * 8) && is_out(S_RMSD) && (R == 0 || (has(S_REC_RMSD, P * 8) && is_out(S_REC_RMSD)));
    if (!ok) return (int)hipErrorInvalidValue;

    harness::Blocks<N_SLOTS> blk(c->buf);
    auto D = [&](int i) { return blk.ptr(i); };
    const dfm::FitChain lig = {(const float *)D(S_LIG_POS), (const float *)D(S_LIG_REF), c->L};
    const dfm::FitChain rec = {(const float *)D(S_REC_POS), (const float *)D(S_REC_REF), c->R};

    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess && reduce) e = dfm::launch_fit_reduce(lig, rec, c->P, c->o, (double *)D(S_SUMS), s);
    if (e == hipSuccess && solve)
        e = dfm::launch_fit_solve((const double *)D(S_SUMS), c->L, c->R, c->P, (double *)D(S_XF), (float *)D(S_ROT), (float *)D(S_TR), s);
    if (e == hipSuccess && resid)
        e = dfm::launch_fit_resid(lig, rec, (const double *)D(S_XF), c->P, c->o, (double *)D(S_RMSD), (double *)D(S_REC_RMSD), s);
    return (int)blk.finish(e);
}

}  // extern "C"
