// heads_harness.hip - test-only host shim around the pair-head and score-head launchers of libdfmdock_amd.so (tests/heads_harness.py
// builds it).
//
// Host code only: no kernels here.  The guard-band protocol is harness_common.h's; this file fills a host dfm::PairArgs / dfm::HeadsDev
// / dfm::HeadArgs whose pointers are the blocks.  The in / out blocks (out = 2) are the pose and the accumulated updates k_heads
// changes in place.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

// buffer slots of one call (tests/heads_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_P, S_Q, S_CA4, S_W_D, S_LN_W, S_LN_B, S_W3, S_S, S_FPART, S_SPART, S_CLASH, S_FVEC, S_CONF, S_DIST,
    S_ENA, S_ENB, S_EN_LN_W, S_EN_LN_B, S_EN_W3,
    S_T, S_T_W, S_T_LIN, S_TRS0, S_TRS_LN_W, S_TRS_LN_B, S_TRS4, S_ROTS0, S_ROTS_LN_W, S_ROTS_LN_B, S_ROTS4, S_BASE,
    S_SCORES, S_Z_ROT, S_Z_TR, S_LIG, S_TR_UPD, S_ROT_UPD, S_TRACE_POSE, S_TRACE_SCORES, S_STEP_PARAMS, S_CTL,
    S_REC_POS, S_PREP_POS, S_PREP_CA4, S_PREP_CB4, N_SLOTS
};

enum Op { OP_PAIR_HEAD, OP_PAIR_HEAD_M, OP_PAIR_FINISH_S, OP_PAIR_FINISH, OP_PAIR_DIST, OP_ENERGY_PAIRS, OP_TIME_EMBED, OP_HEADS, OP_PREP_POSE };

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    long long hid_bstride, z_bstride, trace_bstride, trace_s_bstride;
    unsigned long long seed;
    float cut_off, inv_pool, pool_div;
    float g2_r, g_r, hg2_r, g2_t, g_t, hg2_t, dt, sqrt_dt, rot_noise, tr_noise;
    int B, R, L, Rp, mode, n_part, want_energy, en_mode, do_update, ode, all_atoms, prep_next, step, n_times;
};

HARNESS_EXPORTS(Call)
long long hh_step_params_bytes() { return (long long)sizeof(dfm::StepParams); }

int kh_run(const Call *c, int op)
{
    harness::Blocks<N_SLOTS> blk(c->buf);
    auto P = [&](int i) { return blk.ptr(i); };
    auto F = [&](int i) -> float * { return (float *)P(i); };

    dfm::PairArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.P = F(S_P); pa.Q = F(S_Q); pa.ca4 = (const float4 *)P(S_CA4); pa.B = c->B; pa.R = c->R; pa.L = c->L;
    pa.w_d = F(S_W_D); pa.ln_w = F(S_LN_W); pa.ln_b = F(S_LN_B); pa.w3 = F(S_W3); pa.mode = c->mode; pa.cut_off = c->cut_off;
    pa.fpart = F(S_FPART); pa.spart = F(S_SPART); pa.clash_part = (int32_t *)P(S_CLASH); pa.S = F(S_S); pa.Rp = c->Rp;

    dfm::HeadsDev hw;      // built here from the uploaded weight arrays
    std::memset(&hw, 0, sizeof(hw));
    hw.en_ln_w = F(S_EN_LN_W); hw.en_ln_b = F(S_EN_LN_B); hw.en_w3 = F(S_EN_W3);
    hw.t_W = F(S_T_W); hw.t_lin = F(S_T_LIN);
    hw.trs0 = F(S_TRS0); hw.trs_ln_w = F(S_TRS_LN_W); hw.trs_ln_b = F(S_TRS_LN_B); hw.trs4 = F(S_TRS4);
    hw.rots0 = F(S_ROTS0); hw.rots_ln_w = F(S_ROTS_LN_W); hw.rots_ln_b = F(S_ROTS_LN_B); hw.rots4 = F(S_ROTS4);

    dfm::HeadArgs ha;
    std::memset(&ha, 0, sizeof(ha));
    ha.fvec = F(S_FVEC); ha.ca4 = (const float4 *)P(S_CA4); ha.B = c->B; ha.R = c->R; ha.L = c->L;
    ha.hid_base = F(S_BASE); ha.hid_bstride = c->hid_bstride; ha.hw = &hw; ha.scores = F(S_SCORES);
    ha.want_energy = c->want_energy; ha.en_part = F(S_SPART); ha.clash_part = (const int32_t *)P(S_CLASH); ha.n_part = c->n_part;
    ha.en_mode = c->en_mode; ha.pool_div = c->pool_div; ha.do_update = c->do_update;
    ha.g2_r = c->g2_r; ha.g_r = c->g_r; ha.hg2_r = c->hg2_r; ha.g2_t = c->g2_t; ha.g_t = c->g_t; ha.hg2_t = c->hg2_t;
    ha.dt = c->dt; ha.sqrt_dt = c->sqrt_dt; ha.rot_noise = c->rot_noise; ha.tr_noise = c->tr_noise; ha.ode = c->ode;
    ha.z_rot = F(S_Z_ROT); ha.z_tr = F(S_Z_TR); ha.z_bstride = c->z_bstride; ha.seed = c->seed; ha.step = (uint32_t)c->step;
    ha.all_atoms = c->all_atoms; ha.lig_cur = F(S_LIG); ha.tr_update = F(S_TR_UPD); ha.rot_update = F(S_ROT_UPD);
    ha.trace_pose = F(S_TRACE_POSE); ha.trace_bstride = c->trace_bstride;
    ha.trace_scores = F(S_TRACE_SCORES); ha.trace_s_bstride = c->trace_s_bstride;
    ha.step_params = (const dfm::StepParams *)P(S_STEP_PARAMS); ha.ctl = (const uint32_t *)P(S_CTL);
    ha.prep_next = c->prep_next; ha.rec_pos = F(S_REC_POS);
    ha.prep_pos = (float4 *)P(S_PREP_POS); ha.prep_ca4 = (float4 *)P(S_PREP_CA4); ha.prep_cb4 = (float4 *)P(S_PREP_CB4);

    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess) {
        switch (op) {
        case OP_PAIR_HEAD: e = dfm::launch_pair_head(pa, s); break;
        case OP_PAIR_HEAD_M: e = dfm::launch_pair_head_m(pa, s); break;
        case OP_PAIR_FINISH_S: e = dfm::launch_pair_finish_s(pa, c->n_part, c->inv_pool, F(S_FVEC), F(S_CONF), s); break;
        case OP_PAIR_FINISH: e = dfm::launch_pair_finish(F(S_FPART), c->B, c->R, c->L, c->inv_pool, F(S_FVEC), F(S_SPART), F(S_CONF), s); break;
        case OP_PAIR_DIST:
            e = dfm::launch_pair_dist(pa.P, pa.Q, pa.ca4, c->B, c->R, c->L, pa.w_d, pa.ln_w, pa.ln_b, pa.w3, F(S_DIST), s);
            break;
        case OP_ENERGY_PAIRS:
            e = dfm::launch_energy_pairs(F(S_ENA), F(S_ENB), pa.ca4, c->B, c->R, c->L, c->cut_off, &hw, c->want_energy, F(S_SPART),
                                         (int32_t *)P(S_CLASH), s);
            break;
        case OP_TIME_EMBED: e = dfm::launch_time_embed(F(S_T), c->n_times, &hw, F(S_BASE), s); break;
        case OP_HEADS: e = dfm::launch_heads(ha, s); break;
        case OP_PREP_POSE:
            e = dfm::launch_prep_pose(F(S_REC_POS), F(S_LIG), c->B, c->R, c->L, c->all_atoms, (float4 *)P(S_PREP_POS), (float4 *)P(S_PREP_CA4),
                                      (float4 *)P(S_PREP_CB4), s);
            break;
        default: e = hipErrorInvalidValue;
        }
    }
    return (int)blk.finish(e);
}

}  // extern "C"
