// aux_harness.hip - test-only host shim around the five launchers of libdfmdock_amd.so that the other eight harnesses leave out
// (tests/aux_harness.py builds it): dfm::launch_pair_dist_sum (k_pair_dist_sum + k_dist_finish + k_dist_mean), launch_restraint,
// launch_symmetry, launch_igso3_cdf and launch_start_pose.
//
// Host code only: no kernels here.  The one entry point takes a call record of named host buffers and an op code.  BEFORE anything is
// uploaded it checks everything a kernel would follow as an index - every array long enough for the launch it feeds, pair indices
// below R / L, gstart strictly increasing from 0 to P, `big` naming each group of more than RS_SMALL pairs once and no other,
// G <= RS_MAX_GROUPS, part / res of pair_dist_sum_parts(R, L) slots, contact_bins in 1 .. 63, the index into t_dev (ctl[0] - 1 or step)
// inside it, for the symmetry step R == L, the order in SYM_MIN_ORDER .. SYM_MAX_ORDER and a control block of 16 bytes (k_symmetry reads
// ctl[3], k_restraint stops at ctl[0]) - and answers hipErrorInvalidValue without a launch when one fails: no call makes a kernel read
// or write outside its blocks.  Then the guard-band protocol of harness_common.h runs with the shipped structs (PairDistSumArgs,
// RestraintArgs, SymmetryArgs, StartArgs) filled from the record.  An optional pointer whose slot is unused is passed as nullptr.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

using harness::GUARD;

// buffer slots of one call (tests/aux_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_P, S_Q, S_CA4, S_W_D, S_LN_W, S_LN_B, S_W3F, S_PAIR_NLL, S_PCONTACT, S_EDIST, S_PCONTACT_MEAN, S_PART, S_RES,
    S_REC_POS, S_GSTART, S_PAIRS, S_UPPER, S_WEIGHT, S_BIG, S_LIG, S_TR_UPD, S_ROT_UPD, S_T_DEV, S_CTL, S_OUT,
    S_PREP_POS, S_PREP_CA4, S_PREP_CB4,
    S_CDF, S_START, S_U_INJ, S_AXIS_INJ, S_TR_INJ,
    S_SYM_OUT, S_STEP_OUT,
    N_SLOTS
};

enum Op { OP_PAIR_DIST_SUM, OP_RESTRAINT, OP_IGSO3_CDF, OP_START_POSE, OP_SYMMETRY };

constexpr long long H = 256;

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    double sigma, sigma_r3;
    long long start_bstride;
    float near_cut, k_tr, k_rot, max_tr, max_rot, t_start, gain_rot, gain_tr;
    // B trajectories; R / L residues; G groups of n_pairs pairs, n_big of them large; n_t entries of t_dev; n the order of the symmetry
    int B, R, L, contact_bins, all_atoms, perturb, G, n_big, n_pairs, apply, prep_next, n_t, n, snap_last;
    unsigned step, seed_lo, seed_hi, num_steps;
};

HARNESS_EXPORTS(Call)
long long ax_parts(int R, int L) { return (long long)dfm::pair_dist_sum_parts(R, L); }
int ax_rs_small() { return dfm::RS_SMALL; }
int ax_rs_max_groups() { return dfm::RS_MAX_GROUPS; }
int ax_sym_out() { return dfm::SYM_OUT; }
int ax_sym_min_order() { return dfm::SYM_MIN_ORDER; }
int ax_sym_max_order() { return dfm::SYM_MAX_ORDER; }

// the checks alone (what kh_run does first): hipSuccess or hipErrorInvalidValue.  Touches no device.
int ax_check(const Call *c, int op)
{
    auto has = [&](int i, long long bytes) { return c->buf[i].host && c->buf[i].bytes >= bytes; };
    auto in = [&](int i, long long bytes) { return has(i, bytes) && c->buf[i].out == 0; };
    auto out = [&](int i, long long bytes) { return has(i, bytes) && c->buf[i].out == 1; };
    auto io = [&](int i, long long bytes) { return has(i, bytes) && c->buf[i].out == 2; };
    auto opt_in = [&](int i, long long bytes) { return !c->buf[i].host || in(i, bytes); };
    auto opt_out = [&](int i, long long bytes) { return !c->buf[i].host || out(i, bytes); };
    bool ok = true;
    for (int i = 0; i < N_SLOTS; ++i) ok = ok && c->buf[i].bytes >= 0 && c->buf[i].out >= 0 && c->buf[i].out <= 2;
    if (!ok) return (int)hipErrorInvalidValue;
    const long long B = c->B, R = c->R, L = c->L, N = R + L;

    if (op == OP_PAIR_DIST_SUM) {
        ok = B >= 1 && B <= 65535 && R >= 1 && L >= 1 && R <= (1 << 20) && L <= (1 << 20) && c->contact_bins >= 1 && c->contact_bins <= 63;
        if (!ok) return (int)hipErrorInvalidValue;
        const long long parts = dfm::pair_dist_sum_parts((int)R, (int)L), map = B * R * L * 4;
        ok = in(S_P, B * N * H * 4) && in(S_Q, B * N * H * 4) && in(S_CA4, B * N * 16) && in(S_W_D, H * 4) && in(S_LN_W, H * 4) &&
             in(S_LN_B, H * 4) && in(S_W3F, 64 * H * 4) && opt_out(S_PAIR_NLL, map) && opt_out(S_PCONTACT, map) && opt_out(S_EDIST, map) &&
             opt_out(S_PCONTACT_MEAN, R * L * 4) && (!c->buf[S_PCONTACT_MEAN].host || c->buf[S_PCONTACT].host) &&
             out(S_PART, B * parts * 4 * 8) && out(S_RES, B * 4 * 8);
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    if (op == OP_RESTRAINT) {
        const long long G = c->G, P = c->n_pairs, nb = c->n_big;
        ok = B >= 1 && B <= 65535 && R >= 1 && L >= 1 && R <= (1 << 20) && L <= (1 << 20) && G >= 0 && G <= dfm::RS_MAX_GROUPS && P >= 0 &&
             P <= dfm::RS_MAX_PAIRS && nb >= 0 && nb <= G && (c->apply == 0 || c->apply == 1) && (c->prep_next == 0 || c->prep_next == 1);
        if (!ok) return (int)hipErrorInvalidValue;
        ok = in(S_REC_POS, R * 36) && in(S_GSTART, (G + 1) * 4) && in(S_PAIRS, P * 8) && in(S_UPPER, G * 4) && in(S_WEIGHT, G * 4) &&
             (nb == 0 || in(S_BIG, nb * 4)) && (c->apply ? io(S_LIG, B * L * 36) : has(S_LIG, B * L * 36) && c->buf[S_LIG].out != 1) &&
             (c->apply ? io(S_TR_UPD, B * 12) && io(S_ROT_UPD, B * 12) : !c->buf[S_TR_UPD].host && !c->buf[S_ROT_UPD].host) &&
             opt_out(S_OUT, B * 32);
        if (ok && c->prep_next) ok = out(S_PREP_POS, B * N * 16) && out(S_PREP_CA4, B * N * 16) && out(S_PREP_CB4, B * N * 16);
        if (ok && !c->prep_next) ok = !c->buf[S_PREP_POS].host && !c->buf[S_PREP_CA4].host && !c->buf[S_PREP_CB4].host;
        if (!ok) return (int)hipErrorInvalidValue;
        const int32_t *gs = (const int32_t *)c->buf[S_GSTART].host, *pr = (const int32_t *)c->buf[S_PAIRS].host;
        ok = gs[0] == 0 && gs[G] == P;
        for (long long g = 0; g < G && ok; ++g) ok = gs[g] < gs[g + 1];      // (an empty group would follow pair -1)
        for (long long q = 0; q < P && ok; ++q) ok = pr[2 * q] >= 0 && pr[2 * q] < R && pr[2 * q + 1] >= 0 && pr[2 * q + 1] < L;
        if (ok) {
            std::vector<char> large((size_t)G + 1, 0);
            long long n_large = 0;
            for (long long g = 0; g < G; ++g)
                if (gs[g + 1] - gs[g] > dfm::RS_SMALL) { large[(size_t)g] = 1; ++n_large; }
            ok = n_large == nb;
            const int32_t *big = (const int32_t *)c->buf[S_BIG].host;
            for (long long k = 0; k < nb && ok; ++k) {
                ok = big[k] >= 0 && big[k] < G && large[(size_t)big[k]] == 1;
                if (ok) large[(size_t)big[k]] = 2;      // once
            }
        }
        if (ok && c->buf[S_T_DEV].host) {
            ok = c->n_t >= 1 && in(S_T_DEV, (long long)c->n_t * 4) && opt_in(S_CTL, 12);
            if (ok) {
                const uint32_t idx = c->buf[S_CTL].host ? ((const uint32_t *)c->buf[S_CTL].host)[0] - 1u : c->step;
                ok = idx < (uint32_t)c->n_t;
            }
        } else if (ok) {
            ok = !c->buf[S_CTL].host;      // a control word without times would be ignored: refuse the misuse
        }
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    if (op == OP_SYMMETRY) {
        ok = B >= 1 && B <= 65535 && R == L && L >= 1 && L <= (1 << 20) && c->n >= dfm::SYM_MIN_ORDER && c->n <= dfm::SYM_MAX_ORDER &&
             (c->apply == 0 || c->apply == 1) && (c->prep_next == 0 || c->prep_next == 1) && (c->snap_last == 0 || c->snap_last == 1);
        if (!ok) return (int)hipErrorInvalidValue;
        ok = in(S_REC_POS, R * 36) && (c->apply ? io(S_LIG, B * L * 36) : has(S_LIG, B * L * 36) && c->buf[S_LIG].out != 1) &&
             (c->apply ? io(S_TR_UPD, B * 12) && io(S_ROT_UPD, B * 12) : !c->buf[S_TR_UPD].host && !c->buf[S_ROT_UPD].host) &&
             opt_out(S_SYM_OUT, B * dfm::SYM_OUT * 8) && opt_out(S_STEP_OUT, B * 24);
        if (ok && c->prep_next) ok = out(S_PREP_POS, B * N * 16) && out(S_PREP_CA4, B * N * 16) && out(S_PREP_CB4, B * N * 16);
        if (ok && !c->prep_next) ok = !c->buf[S_PREP_POS].host && !c->buf[S_PREP_CA4].host && !c->buf[S_PREP_CB4].host;
        if (ok && c->buf[S_T_DEV].host) {
            ok = c->n_t >= 1 && in(S_T_DEV, (long long)c->n_t * 4) && opt_in(S_CTL, 16);      // (k_symmetry reads ctl[3]: 16 bytes, not k_restraint's 12)
            if (ok) {
                const uint32_t idx = c->buf[S_CTL].host ? ((const uint32_t *)c->buf[S_CTL].host)[0] - 1u : c->step;
                ok = idx < (uint32_t)c->n_t;
            }
        } else if (ok) {
            ok = !c->buf[S_CTL].host;
        }
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    if (op == OP_IGSO3_CDF) return out(S_CDF, (long long)dfm::IGSO3_N * 8) ? (int)hipSuccess : (int)hipErrorInvalidValue;
    if (op == OP_START_POSE) {
        ok = B >= 1 && B <= 65535 && L >= 1 && L <= (1 << 20) && (c->start_bstride == 0 || c->start_bstride >= L * 9) &&
             c->start_bstride <= (1ll << 32) && (c->perturb == 0 || c->perturb == 1);
        if (!ok) return (int)hipErrorInvalidValue;
        ok = in(S_START, ((B - 1) * c->start_bstride + L * 9) * 4) && (!c->perturb || in(S_CDF, (long long)dfm::IGSO3_N * 8)) &&
             opt_in(S_U_INJ, B * 4) && opt_in(S_AXIS_INJ, B * 12) && opt_in(S_TR_INJ, B * 12) && opt_out(S_LIG, B * L * 36) &&
             out(S_TR_UPD, B * 12) && out(S_ROT_UPD, B * 12);
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    return (int)hipErrorInvalidValue;
}

int kh_run(const Call *c, int op)
{
    if (ax_check(c, op) != (int)hipSuccess) return (int)hipErrorInvalidValue;

    harness::Blocks<N_SLOTS> blk(c->buf);
    auto P = [&](int i) { return blk.ptr(i); };
    auto F = [&](int i) -> float * { return (float *)P(i); };

    dfm::PairDistSumArgs pd;
    std::memset(&pd, 0, sizeof(pd));
    pd.P = F(S_P); pd.Q = F(S_Q); pd.ca4 = (const float4 *)P(S_CA4); pd.B = c->B; pd.R = c->R; pd.L = c->L;
    pd.w_d = F(S_W_D); pd.ln_w = F(S_LN_W); pd.ln_b = F(S_LN_B); pd.w3f = F(S_W3F);
    pd.contact_bins = c->contact_bins; pd.near_cut = c->near_cut;
    pd.pair_nll = F(S_PAIR_NLL); pd.pcontact = F(S_PCONTACT); pd.edist = F(S_EDIST); pd.pcontact_mean = F(S_PCONTACT_MEAN);
    pd.part = (double *)P(S_PART); pd.res = (double *)P(S_RES);

    dfm::RestraintArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.rec_pos = F(S_REC_POS); ra.R = c->R; ra.L = c->L; ra.all_atoms = c->all_atoms;
    ra.gstart = (const int32_t *)P(S_GSTART); ra.pairs = (const int32_t *)P(S_PAIRS); ra.upper = F(S_UPPER); ra.weight = F(S_WEIGHT);
    ra.big = (const int32_t *)P(S_BIG); ra.G = c->G; ra.n_big = c->n_big;
    ra.k_tr = c->k_tr; ra.k_rot = c->k_rot; ra.max_tr = c->max_tr; ra.max_rot = c->max_rot; ra.t_start = c->t_start;
    ra.lig = F(S_LIG); ra.apply = c->apply; ra.tr_update = F(S_TR_UPD); ra.rot_update = F(S_ROT_UPD);
    ra.t_dev = F(S_T_DEV); ra.step = c->step; ra.ctl = (const uint32_t *)P(S_CTL); ra.out = F(S_OUT);
    ra.prep_next = c->prep_next;
    ra.prep_pos = (float4 *)P(S_PREP_POS); ra.prep_ca4 = (float4 *)P(S_PREP_CA4); ra.prep_cb4 = (float4 *)P(S_PREP_CB4);

    dfm::SymmetryArgs sy;
    std::memset(&sy, 0, sizeof(sy));
    sy.rec_pos = F(S_REC_POS); sy.R = c->R; sy.L = c->L; sy.all_atoms = c->all_atoms; sy.n = c->n;
    sy.gain_rot = c->gain_rot; sy.gain_tr = c->gain_tr; sy.max_rot = c->max_rot; sy.max_tr = c->max_tr; sy.t_start = c->t_start;
    sy.snap_last = c->snap_last; sy.lig = F(S_LIG); sy.apply = c->apply; sy.tr_update = F(S_TR_UPD); sy.rot_update = F(S_ROT_UPD);
    sy.t_dev = F(S_T_DEV); sy.step = c->step; sy.num_steps = c->num_steps; sy.ctl = (const uint32_t *)P(S_CTL);
    sy.out = (double *)P(S_SYM_OUT); sy.step_out = F(S_STEP_OUT); sy.prep_next = c->prep_next;
    sy.prep_pos = (float4 *)P(S_PREP_POS); sy.prep_ca4 = (float4 *)P(S_PREP_CA4); sy.prep_cb4 = (float4 *)P(S_PREP_CB4);

    dfm::StartArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.start = F(S_START); sa.start_bstride = c->start_bstride; sa.L = c->L; sa.all_atoms = c->all_atoms; sa.perturb = c->perturb;
    sa.cdf = (const double *)P(S_CDF); sa.sigma_r3 = c->sigma_r3;
    sa.u_inj = F(S_U_INJ); sa.axis_inj = F(S_AXIS_INJ); sa.tr_inj = F(S_TR_INJ); sa.seed_lo = c->seed_lo; sa.seed_hi = c->seed_hi;
    sa.lig_cur = F(S_LIG); sa.tr_update = F(S_TR_UPD); sa.rot_update = F(S_ROT_UPD);

    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess) switch (op) {
        case OP_PAIR_DIST_SUM: e = dfm::launch_pair_dist_sum(pd, s); break;
        case OP_RESTRAINT: e = dfm::launch_restraint(ra, c->B, s); break;
        case OP_IGSO3_CDF: e = dfm::launch_igso3_cdf(c->sigma, (double *)P(S_CDF), s); break;
        case OP_START_POSE: e = dfm::launch_start_pose(sa, c->B, s); break;
        case OP_SYMMETRY: e = dfm::launch_symmetry(sy, c->B, s); break;
        default: e = hipErrorInvalidValue;
    }
    return (int)blk.finish(e);
}

}  // extern "C"
