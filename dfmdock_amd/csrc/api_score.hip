// api_score.hip - the calls that evaluate the score network on given poses: dfm_score, dfm_score_distogram and the runtime parity
// check dfm_complex_selfcheck.  Each is the scaffold of api_forward.hip around enqueue_forward, its own heads and its read-back.
#include <cmath>
#include <cstring>
#include <vector>

#include "dfm_engine.h"

using namespace dfm;

// to_ires (score_net_mlsb.py:297-303,:383): Linear(256,512) SiLU Linear(512,512) SiLU Linear(512,1) on the final node
// features; never read by the sampler, fp32 GEMMs in every engine
static hipError_t enqueue_ires(dfm_complex *cx, int B)
{
    const dfm_model *m = cx->m;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    GemmArgs g = gemm_args(W.h, H, H, m->ir0_w, H, m->ir0_b, B * cx->N, 2 * H, W.ir1, 2 * H);
    hipError_t e = launch_gemm_f32(g, s);
    g.A0 = W.ir1; g.lda = 2 * H; g.K = 2 * H; g.pro = 3; g.W = m->ir2_w; g.ldw = 2 * H; g.bias = m->ir2_b; g.C = W.ir2;
    if (e == hipSuccess) e = launch_gemm_f32(g, s);
    g.A0 = W.ir2; g.W = m->ir4_w; g.bias = m->ir4_b; g.Nout = 1; g.C = W.ir3; g.ldc = 1;
    if (e == hipSuccess) e = launch_gemm_f32(g, s);
    return e;
}

// the outputs of dfm_score to the caller's arrays; synchronises
static int read_score_out(dfm_complex *cx, int B, const float *h_first_dev, const float *ires_dev, const float *dist_dev, bool want_energy,
                          dfm_score_out *out)
{
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const size_t N = cx->N, L = cx->L, K = cx->K;
    std::vector<float> sc((size_t)B * 8);
    HIPCHK(hipEventRecord(cx->ev_total[1], s));
    HIPCHK(hipMemcpyAsync(sc.data(), W.scores, sc.size() * 4, hipMemcpyDeviceToHost, s));
    if (out->f) HIPCHK(hipMemcpyAsync(out->f, W.fvec, (size_t)B * L * 3 * 4, hipMemcpyDeviceToHost, s));
    if (out->h_last) HIPCHK(hipMemcpyAsync(out->h_last, W.h, (size_t)B * N * H * 4, hipMemcpyDeviceToHost, s));
    if (out->h_first) HIPCHK(hipMemcpyAsync(out->h_first, h_first_dev, (size_t)B * N * H * 4, hipMemcpyDeviceToHost, s));
    if (out->edges) HIPCHK(hipMemcpyAsync(out->edges, W.edges, (size_t)B * N * K * 4, hipMemcpyDeviceToHost, s));
    if (out->edge_codes) HIPCHK(hipMemcpyAsync(out->edge_codes, W.codes, (size_t)B * N * K * 4, hipMemcpyDeviceToHost, s));
    if (ires_dev) HIPCHK(hipMemcpyAsync(out->ires, ires_dev, (size_t)B * N * 4, hipMemcpyDeviceToHost, s));
    if (dist_dev) HIPCHK(hipMemcpyAsync(out->dist_logits, dist_dev, (size_t)B * cx->R * L * 64 * 4, hipMemcpyDeviceToHost, s));
    if (out->confidence) {
        if (cx->m->hp.family == 1 && want_energy) HIPCHK(hipMemcpyAsync(out->confidence, W.conf, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        else std::memset(out->confidence, 0, (size_t)B * 4);
    }
    HIPCHK(hipStreamSynchronize(s));
    unpack_scores(sc.data(), B, out->tr_score, out->rot_score, 3, out->energy, out->num_clashes);
    return DFM_OK;
}

extern "C" int dfm_score(dfm_complex *cx, int B, const float *lig_pos, const float *t, const int32_t *edges,
                         uint64_t seed, uint32_t flags, dfm_score_out *out)
{
    if (!cx || !lig_pos || !t || !out || !out->tr_score || !out->rot_score) return fail(DFM_E_INVALID, "NULL argument");
    if (B < 1) return fail(DFM_E_INVALID, "B must be >= 1");
    const EngineSel sel = engine_sel(flags);
    const bool want_energy = flags & DFM_F_ENERGY;
    const bool want_ires = (flags & DFM_F_IRES) && out->ires;
    const bool want_dist = (flags & DFM_F_DIST) && out->dist_logits;
    if (want_dist && cx->m->hp.family != 1) return fail(DFM_E_INVALID, "DFM_F_DIST needs a family-1 model (EGNN_Net has to_dist, Score_Net does not)");
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    // layer 0 through the message table: on request only (dfm_score stays a pure function of its arguments and flags)
    const bool l0 = (flags & DFM_F_L0_TABLE) != 0;
    if (l0 && !(sel.has_table && l0_eligible(cx)))
        return fail(DFM_E_INVALID, "DFM_F_L0_TABLE needs the fp32 or the DFM_F_MFMA16 engine (no DFM_F_F16 / DFM_F_BF16_OPS), depth >= 2 and a complex / batch within the table budgets");
    int rc = begin_call(cx, B, sel, l0);
    if (rc) return rc;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const size_t N = cx->N, L = cx->L, K = cx->K;
    DevPool tmp;   // per-call device buffers (injected edges, debug tap); released on every return path
    tmp.bind(s);
    int32_t *edges_dev = nullptr;
    float *h_first_dev = nullptr, *dist_dev = nullptr;
    if ((rc = upload_batch(cx, B, lig_pos, t, edges, tmp, &edges_dev)) != DFM_OK) return rc;
    if (out->h_first) HIPCHK(tmp.alloc(&h_first_dev, (size_t)B * N * H));
    if (want_ires && !W.ir3) {      // kept with the workspace: a forward() loop does not pay three hipMalloc / hipFree pairs per call
        // (ir3 is the last of the three: a call that failed half-way allocates all of them again; the pool owns the orphans)
        W.ir1 = W.ir2 = nullptr;
        HIPCHK(W.pool.alloc(&W.ir1, (size_t)W.Bcap * N * 2 * H)); HIPCHK(W.pool.alloc(&W.ir2, (size_t)W.Bcap * N * 2 * H));
        HIPCHK(W.pool.alloc(&W.ir3, (size_t)W.Bcap * N));
    }
    FwdOpts o = fwd_opts(sel);
    o.want_energy = want_energy; o.profile = flags & DFM_F_PROFILE; o.edges_dev = edges_dev;
    o.edges_pitch = (int64_t)N * K; o.seed = seed; o.h_first_out = h_first_dev; o.l0_table = l0;
    // (h_first: a depth-1 model's first layer is its last - the tap needs that layer's node model too)
    o.need_node_out = want_energy || want_ires || want_dist || out->h_last != nullptr || out->h_first != nullptr;
    HIPCHK(hipEventRecord(cx->ev_total[0], s));
    if ((rc = enqueue_forward(cx, B, o)) != DFM_OK) return rc;
    HeadArgs ha;
    fill_head_args(cx, B, want_energy, &ha);
    HIPCHK(launch_heads(ha, s));
    if (want_ires) HIPCHK(enqueue_ires(cx, B));
    if (want_dist) {
        // dist_logits (egnn_net.py:447): project every node through the stacked halves of to_dist.0 (reusing the A / Bm buffers),
        // then the pair kernel; fp32 in every engine
        const PairHeadDev &D = cx->m->dist;
        HIPCHK(tmp.alloc(&dist_dev, (size_t)B * cx->R * L * 64));
        HIPCHK(project_ab(cx, B, D.wab));
        HIPCHK(launch_pair_dist(W.A, W.Bm, W.ca4, B, cx->R, (int)L, D.w_d, D.ln_w, D.ln_b, D.w3, dist_dev, s));
    }
    if ((rc = read_score_out(cx, B, h_first_dev, want_ires ? W.ir3 : nullptr, dist_dev, want_energy, out)) != DFM_OK) return rc;
    if (o.profile && (rc = finish_profile(cx)) != DFM_OK) return rc;
    return guard.done(DFM_OK);
}

// ------------------------------------------------------------------------------------------------
// The distogram head of the second family reduced on the device (kernels_pair.hip: k_pair_dist_sum).  The forward is dfm_score's: same
// uploads, time embedding, graph, layers and stream; then to_dist.0's projection GEMM into W.A / W.Bm as under DFM_F_DIST, and the fused
// pair kernel in place of k_pair_dist - the [B,R,L,64] logits are never stored.
static thread_local double g_distogram_ms[2] = {};

extern "C" int dfm_score_distogram(dfm_complex *cx, int B, const float *lig_pos, const float *t, const int32_t *edges, uint64_t seed,
                                   uint32_t flags, const dfm_distogram_params *prm, dfm_distogram_out *out)
{
    if (!cx || !lig_pos || !t || !prm || !out || !out->nll || !out->nll_near || !out->n_near || !out->exp_contacts)
        return fail(DFM_E_INVALID, "NULL argument");
    if (B < 1) return fail(DFM_E_INVALID, "B must be >= 1");
    if (cx->m->hp.family != 1) return fail(DFM_E_INVALID, "dfm_score_distogram needs a family-1 model (EGNN_Net has to_dist, Score_Net does not)");
    if (prm->contact_bins < 1 || prm->contact_bins > 63) return fail(DFM_E_INVALID, "contact_bins must be in 1..63");
    if (prm->near_cutoff != prm->near_cutoff) return fail(DFM_E_INVALID, "near_cutoff is NaN");
    if (flags & (DFM_F_L0_TABLE | DFM_F_PROFILE | DFM_F_DIST | DFM_F_IRES))
        return fail(DFM_E_INVALID, "dfm_score_distogram takes the engine flags only (DFM_F_MFMA16, DFM_F_F16, DFM_F_BF16_OPS)");
    const float near_cut = prm->near_cutoff > 0.f ? prm->near_cutoff : cx->m->hp.cut_off;
    const EngineSel sel = engine_sel(flags);
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    int rc = begin_call(cx, B, sel, false);
    if (rc) return rc;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const size_t N = cx->N, L = cx->L, K = cx->K, RL = (size_t)cx->R * L;
    struct Ev {
        hipEvent_t e = nullptr;
        ~Ev() { if (e) (void)hipEventDestroy(e); }
    } ev_begin, ev_end;
    HIPCHK(hipEventCreate(&ev_begin.e)); HIPCHK(hipEventCreate(&ev_end.e));
    HIPCHK(hipEventRecord(ev_begin.e, s));
    DevPool tmp;
    tmp.bind(s);
    int32_t *edges_dev = nullptr;
    if ((rc = upload_batch(cx, B, lig_pos, t, edges, tmp, &edges_dev)) != DFM_OK) return rc;
    PairDistSumArgs a;
    a.pair_nll = a.pcontact = a.edist = a.pcontact_mean = nullptr;
    HIPCHK(tmp.alloc(&a.part, (size_t)B * pair_dist_sum_parts(cx->R, (int)L) * 4));
    HIPCHK(tmp.alloc(&a.res, (size_t)B * 4));
    if (out->pair_nll) HIPCHK(tmp.alloc(&a.pair_nll, (size_t)B * RL));
    if (out->pcontact || out->pcontact_mean) HIPCHK(tmp.alloc(&a.pcontact, (size_t)B * RL));
    if (out->edist) HIPCHK(tmp.alloc(&a.edist, (size_t)B * RL));
    if (out->pcontact_mean) HIPCHK(tmp.alloc(&a.pcontact_mean, RL));
    FwdOpts o = fwd_opts(sel);
    o.edges_dev = edges_dev; o.edges_pitch = (int64_t)N * K; o.seed = seed;
    HIPCHK(hipEventRecord(cx->ev_total[0], s));
    if ((rc = enqueue_forward(cx, B, o)) != DFM_OK) return rc;
    const dfm_model *m = cx->m;
    HIPCHK(project_ab(cx, B, m->dist.wab));
    a.P = W.A; a.Q = W.Bm; a.ca4 = W.ca4; a.B = B; a.R = cx->R; a.L = (int)L;
    a.w_d = m->dist.w_d; a.ln_w = m->dist.ln_w; a.ln_b = m->dist.ln_b; a.w3f = m->dist_w3f;
    a.contact_bins = prm->contact_bins; a.near_cut = near_cut;
    HIPCHK(launch_pair_dist_sum(a, s));
    std::vector<double> hres((size_t)B * 4);
    HIPCHK(hipEventRecord(cx->ev_total[1], s));
    HIPCHK(hipMemcpyAsync(hres.data(), a.res, hres.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out->pair_nll) HIPCHK(hipMemcpyAsync(out->pair_nll, a.pair_nll, (size_t)B * RL * 4, hipMemcpyDeviceToHost, s));
    if (out->pcontact) HIPCHK(hipMemcpyAsync(out->pcontact, a.pcontact, (size_t)B * RL * 4, hipMemcpyDeviceToHost, s));
    if (out->edist) HIPCHK(hipMemcpyAsync(out->edist, a.edist, (size_t)B * RL * 4, hipMemcpyDeviceToHost, s));
    if (out->pcontact_mean) HIPCHK(hipMemcpyAsync(out->pcontact_mean, a.pcontact_mean, RL * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(ev_end.e, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        out->nll[b] = (float)hres[(size_t)b * 4]; out->nll_near[b] = (float)hres[(size_t)b * 4 + 1];
        out->n_near[b] = (int32_t)hres[(size_t)b * 4 + 2]; out->exp_contacts[b] = (float)hres[(size_t)b * 4 + 3];
    }
    float up_ms = 0.f, k_ms = 0.f, down_ms = 0.f;
    (void)hipEventElapsedTime(&up_ms, ev_begin.e, cx->ev_total[0]);
    (void)hipEventElapsedTime(&k_ms, cx->ev_total[0], cx->ev_total[1]);
    (void)hipEventElapsedTime(&down_ms, cx->ev_total[1], ev_end.e);
    g_distogram_ms[0] = (double)up_ms + (double)down_ms;
    g_distogram_ms[1] = (double)k_ms;
    return guard.done(DFM_OK);
}

extern "C" int dfm_distogram_last_timing(double *copy_ms, double *kernel_ms)
{
    if (!copy_ms || !kernel_ms) return fail(DFM_E_INVALID, "NULL argument");
    *copy_ms = g_distogram_ms[0];
    *kernel_ms = g_distogram_ms[1];
    return DFM_OK;
}

// ------------------------------------------------------------------------------------------------
// Runtime parity evidence for weights the build has never seen (include/dfmdock_amd.h: dfm_selfcheck_out).
struct SelfcheckPass { std::vector<float> tr, rot, energy, f; };      // [B][3], [B][3], [B], [B][L][3] of one engine

// one evaluation with the energy head, read back; keep_edges (or nullptr): [B][N][K] for the graphs it drew.  Synchronises
static int selfcheck_pass(dfm_complex *cx, int B, const FwdOpts &o, int32_t *keep_edges, SelfcheckPass &r)
{
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    int rc = enqueue_forward(cx, B, o);
    if (rc) return rc;
    HeadArgs ha;
    fill_head_args(cx, B, true, &ha);
    HIPCHK(launch_heads(ha, s));
    std::vector<float> sc((size_t)B * 8);
    r.f.resize((size_t)B * cx->L * 3);
    HIPCHK(hipMemcpyAsync(sc.data(), W.scores, sc.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(r.f.data(), W.fvec, r.f.size() * 4, hipMemcpyDeviceToHost, s));
    if (keep_edges) HIPCHK(hipMemcpyAsync(keep_edges, W.edges, (size_t)B * cx->N * cx->K * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    r.tr.resize((size_t)B * 3); r.rot.resize((size_t)B * 3); r.energy.resize(B);
    unpack_scores(sc.data(), B, r.tr.data(), r.rot.data(), 3, r.energy.data(), nullptr);
    return DFM_OK;
}

// deviations of the 16-bit pass from the fp32 pass, and what the pooling of f makes of them
static void selfcheck_deviations(const dfm_complex *cx, int B, const SelfcheckPass &r32, const SelfcheckPass &r16, const std::vector<float4> &ca,
                                 dfm_selfcheck_out &o)
{
    auto dev_of = [](const float *a, const float *ref, size_t n) {      // L-inf over L-inf; NaN / inf anywhere -> NaN (never "ok")
        double d = 0, mx = 0;
        for (size_t i = 0; i < n; ++i) {
            if (!std::isfinite(a[i]) || !std::isfinite(ref[i])) return std::nanf("");
            d = std::fmax(d, std::fabs((double)a[i] - (double)ref[i])); mx = std::fmax(mx, std::fabs((double)ref[i]));
        }
        return (float)(d / std::fmax(mx, 1e-30));
    };
    auto worse = [](float cur, float v) { return (v != v || cur != cur) ? std::nanf("") : std::fmax(cur, v); };
    const size_t R = cx->R, L = cx->L;
    for (int b = 0; b < B; ++b) {
        const float *f32 = &r32.f[(size_t)b * L * 3], *f16 = &r16.f[(size_t)b * L * 3];
        const float df = dev_of(f16, f32, L * 3);
        o.dev_f = worse(o.dev_f, df);
        o.dev_tr_score = worse(o.dev_tr_score, dev_of(&r16.tr[(size_t)b * 3], &r32.tr[(size_t)b * 3], 3));
        o.dev_rot_score = worse(o.dev_rot_score, dev_of(&r16.rot[(size_t)b * 3], &r32.rot[(size_t)b * 3], 3));
        const double e32 = r32.energy[b], e16 = r16.energy[b];
        o.dev_energy = worse(o.dev_energy, (std::isfinite(e32) && std::isfinite(e16)) ? (float)(std::fabs(e16 - e32) / std::fmax(std::fabs(e32), 0.1)) : std::nanf(""));
        // pooled force mean_l f and torque mean_l (r_l x f_l) (score_net_mlsb.py:396-405): cancellation ratios and the bounds they give
        double mf[3] = {0, 0, 0}, mt[3] = {0, 0, 0}, af = 0, at = 0, fmax = 0, rmean = 0;
        for (size_t l = 0; l < L; ++l) {
            const float *v = f32 + l * 3;
            const float4 r4 = ca[R + l];
            const double r[3] = {r4.x, r4.y, r4.z};
            const double c[3] = {r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]};
            for (int k = 0; k < 3; ++k) { mf[k] += v[k]; mt[k] += c[k]; fmax = std::fmax(fmax, std::fabs((double)v[k])); }
            af += std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
            at += std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            rmean += std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        }
        const double nf = std::sqrt(mf[0] * mf[0] + mf[1] * mf[1] + mf[2] * mf[2]) / (double)L;      // |mean f|
        const double nt = std::sqrt(mt[0] * mt[0] + mt[1] * mt[1] + mt[2] * mt[2]) / (double)L;      // |mean r x f|
        af /= (double)L; at /= (double)L; rmean /= (double)L;
        o.cancel_ratio[0] = std::fmin(o.cancel_ratio[0], (float)(nf / std::fmax(af, 1e-30)));
        o.cancel_ratio[1] = std::fmin(o.cancel_ratio[1], (float)(nt / std::fmax(at, 1e-30)));
        const double dabs = std::sqrt(3.0) * (double)df * fmax;      // |d f_l| <= sqrt(3) dev_f max|f| for every l
        o.score_bound[0] = worse(o.score_bound[0], (float)(dabs / std::fmax(nf, 1e-30)));
        o.score_bound[1] = worse(o.score_bound[1], (float)(dabs * rmean / std::fmax(nt, 1e-30)));
    }
}

// the range telemetry of the fp32 pass (rg: [depth + 1][8] float bits) and the saturation count of the 16-bit pass, then the verdict
static void selfcheck_verdict(const dfm_model *m, const std::vector<uint32_t> &rg, unsigned long long sat, dfm_selfcheck_out &o)
{
    const int depth = m->hp.depth;
    const float LOG2E = -SILU_S;
    auto val = [&](int l, int k) { return __builtin_bit_cast(float, rg[(size_t)l * 8 + k]); };
    float worst = 0.f;
    for (int l = 0; l <= depth; ++l) o.max_h[l] = val(l, 0);
    for (int l = 0; l < depth; ++l) {
        o.max_A[l] = LOG2E * val(l, 1); o.max_Bm[l] = LOG2E * val(l, 2);
        o.max_tab[l] = std::fmax(m->tab_max[l][0], m->tab_max[l][1]);
        o.max_sum16[l] = o.max_Bm[l] + m->tab_max[l][0] + m->tab_max[l][1];
        o.max_pre[l] = LOG2E * val(l, 3); o.max_acc[l] = LOG2E * val(l, 4);
        for (float v : {o.max_A[l], o.max_Bm[l], o.max_tab[l], o.max_sum16[l], o.max_pre[l], o.max_acc[l]}) worst = (v != v) ? INFINITY : std::fmax(worst, v);
    }
    o.headroom = worst > 0.f ? o.limit / worst : INFINITY;
    o.saturated = (int64_t)sat;
    o.range_ok = (worst < o.limit && sat == 0) ? 1 : 0;
    const float gate_tr = std::fmax(o.gate_score, 2.0f * o.score_bound[0]), gate_rot = std::fmax(o.gate_score, 2.0f * o.score_bound[1]);
    o.dev_ok = (o.dev_f <= o.gate_f && o.dev_energy <= o.gate_energy && o.dev_tr_score <= gate_tr && o.dev_rot_score <= gate_rot) ? 1 : 0;
    o.ok = o.range_ok && o.dev_ok;
}

extern "C" int dfm_complex_selfcheck(dfm_complex *cx, int n_eval, const float *t_in, uint64_t seed, uint32_t flags, dfm_selfcheck_out *out)
{
    if (!cx || !out) return fail(DFM_E_INVALID, "NULL argument");
    if (n_eval < 1 || n_eval > 16) return fail(DFM_E_INVALID, "n_eval must be in 1..16");
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    const int B = n_eval;
    // the 16-bit pass runs the engine as dfm_sample runs it: layer 0 through the message table where the complex is eligible
    const EngineSel sel16 = engine_sel(flags | DFM_F_MFMA16);
    const bool l0 = table_by_default(sel16, flags) && l0_eligible(cx);
    int rc = begin_call(cx, B, sel16, l0);
    if (rc) return rc;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const int depth = cx->m->hp.depth;
    const size_t N = cx->N, L = cx->L, K = cx->K;
    std::vector<float> t(B);
    for (int b = 0; b < B; ++b) {
        t[b] = t_in ? t_in[b] : (B == 1 ? 0.5f : 1.0f + (0.001f - 1.0f) * (float)b / (float)(B - 1));
        if (!(t[b] >= 0.f && t[b] <= 1.f)) return fail(DFM_E_INVALID, "Invalid t (need 0 <= t <= 1)");
    }
    DevPool tmp;
    tmp.bind(s);
    uint32_t *range_d = nullptr;
    unsigned long long *sat_d = nullptr;
    int32_t *edges_d = nullptr;
    HIPCHK(tmp.alloc(&range_d, (size_t)(depth + 1) * 8)); HIPCHK(tmp.alloc(&sat_d, 1)); HIPCHK(tmp.alloc(&edges_d, (size_t)B * N * K));
    HIPCHK(hipMemsetAsync(range_d, 0, (size_t)(depth + 1) * 8 * 4, s)); HIPCHK(hipMemsetAsync(sat_d, 0, 8, s));
    for (int b = 0; b < B; ++b)
        HIPCHK(hipMemcpyAsync(W.lig_cur + (size_t)b * L * 9, cx->lig0, L * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(W.t_dev, t.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(launch_time_embed(W.t_dev, B, &cx->m->heads, W.hid_base, s));

    // the fp32 pass draws the graphs and leaves them in edges_d; the 16-bit pass replays them
    SelfcheckPass r32, r16;
    FwdOpts o = fwd_opts(engine_sel(0));
    o.want_energy = true; o.need_node_out = true; o.seed = seed; o.range = range_d;
    if ((rc = selfcheck_pass(cx, B, o, edges_d, r32)) != DFM_OK) return rc;
    std::vector<float4> ca(N);      // centred CA of the (one) pose: r of the torque pooling
    HIPCHK(hipMemcpyAsync(ca.data(), W.ca4, N * sizeof(float4), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    o = fwd_opts(sel16);
    o.want_energy = true; o.need_node_out = true; o.seed = seed;
    o.edges_dev = edges_d; o.edges_pitch = (int64_t)N * K; o.sat = sat_d; o.l0_table = l0;
    if (l0)      // the table's own entries (S * gate * m as fp16) are clamped like every other 16-bit store: count them too
        HIPCHK(launch_sat_count(cx->l0_table, (long long)((size_t)cx->R * cx->R + (size_t)cx->L * cx->L) * H, sat_d, s));
    if ((rc = selfcheck_pass(cx, B, o, nullptr, r16)) != DFM_OK) return rc;
    std::vector<uint32_t> rg((size_t)(depth + 1) * 8);
    unsigned long long sat = 0;
    HIPCHK(hipMemcpyAsync(rg.data(), range_d, rg.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&sat, sat_d, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));

    std::memset(out, 0, sizeof(*out));
    out->n_eval = B; out->depth = depth;
    out->gate_f = 1e-2f; out->gate_score = 1e-2f; out->gate_energy = 3e-2f; out->limit = 6.0e4f;
    out->cancel_ratio[0] = out->cancel_ratio[1] = 1e30f;
    selfcheck_deviations(cx, B, r32, r16, ca, *out);
    selfcheck_verdict(cx->m, rg, sat, *out);
    return guard.done(DFM_OK);
}
