// api_sample.hip - the sampler behind dfm_sample and dfm_refine (Euler-Maruyama over the time grid of dfm_schedule.h, step by step or
// as one captured step graph replayed), the IGSO(3) cdf tables and the forward marginal of the local refinement.  The host only
// enqueues: no synchronisation inside the step loop.
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "dfm_engine.h"

using namespace dfm;

// The sampler behind dfm_sample and dfm_refine: the time grid linspace(t_first, eps, num_steps) and `start`, which fills ws.lig_cur /
// tr_update / rot_update with the start poses on the handle's stream (per-call device buffers from `tmp`).  Everything after the
// start - noise scales, last step without noise, annealing, ODE, clash force, restraint step, symmetry step, final evaluation - is shared.
using StartFn = std::function<int(DevPool &tmp)>;

// one sampler call: its arguments, its time grid, its per-call device buffers and what they decide
struct SampleCall {
    dfm_complex *cx;
    int B, num_steps;
    uint32_t flags;
    uint64_t seed;
    float tr_noise_scale, rot_noise_scale;
    TimeGrid grid;
    float *zr_d = nullptr, *zt_d = nullptr, *tp_d = nullptr, *tsc_d = nullptr, *ip_d = nullptr;      // injected z, traces, the start poses
    int32_t *ed_d = nullptr;                                                                         // injected graphs
    bool step_energy = false;
    bool use_graph = false;      // the step loop is a replayed captured graph
    // the pose a step produces is prepared for the next evaluation by that step's k_heads (one dependent launch less per step) unless
    // something still moves it afterwards (clash force) or the step is a captured graph (whose first launch is the preparation)
    bool fuse_prep = false;
    // the restraint step (DFM_F_RESTRAINTS with a set stored): after k_heads, before the clash force.  Without the clash force it is the
    // last kernel that moves the pose and takes over k_heads' preparation of it - the flag adds no dependent launch per step
    bool restr = false;
    // the symmetry step (DFM_F_SYMMETRY with a symmetry stored): the last thing that moves the pose in a step, after the clash force, so
    // a snapped final pose stays snapped.  Under fuse_prep it is the kernel that prepares the pose (k_heads and k_restraint then do not)
    bool sym = false;
};

// the by-value arguments of step i's k_heads launch
static void step_head_args(const SampleCall &c, int i, HeadArgs &ha)
{
    Workspace &W = c.cx->ws;
    const size_t L = c.cx->L, S = c.num_steps;
    fill_head_args(c.cx, c.B, c.step_energy, &ha);
    ha.hid_base = W.hid_base + (size_t)i * 2 * HI; ha.hid_bstride = 0;      // this step's time for the whole batch
    ha.do_update = 1;
    const StepParams p = step_params(c.grid, i, c.flags, c.tr_noise_scale, c.rot_noise_scale, c.num_steps);
    ha.g2_r = p.g2_r; ha.g_r = p.g_r; ha.hg2_r = p.hg2_r; ha.g2_t = p.g2_t; ha.g_t = p.g_t; ha.hg2_t = p.hg2_t;
    ha.dt = p.dt; ha.sqrt_dt = p.sqrt_dt; ha.tr_noise = p.tr_noise; ha.rot_noise = p.rot_noise;
    ha.ode = (c.flags & DFM_F_ODE) ? 1 : 0;
    ha.z_rot = c.zr_d ? c.zr_d + (size_t)i * 3 : nullptr; ha.z_tr = c.zt_d ? c.zt_d + (size_t)i * 3 : nullptr;
    ha.z_bstride = (int64_t)S * 3; ha.seed = c.seed; ha.step = p.step;
    if (c.tp_d) { ha.trace_pose = c.tp_d + (size_t)i * L * 9; ha.trace_bstride = (int64_t)S * L * 9; }
    if (c.tsc_d) { ha.trace_scores = c.tsc_d + (size_t)i * 8; ha.trace_s_bstride = (int64_t)(S + 1) * 8; }
}

static hipError_t restraint_step(const SampleCall &c, int i, const uint32_t *ctl)
{
    Workspace &W = c.cx->ws;
    RestraintArgs ra = restraint_args(c.cx, W.lig_cur);
    ra.apply = 1; ra.tr_update = W.tr_update; ra.rot_update = W.rot_update;
    ra.t_dev = W.t_dev; ra.step = (uint32_t)i; ra.ctl = ctl;
    if (c.fuse_prep && !c.sym) { ra.prep_next = 1; ra.prep_pos = W.pos; ra.prep_ca4 = W.ca4; ra.prep_cb4 = W.cb4; }
    return launch_restraint(ra, c.B, c.cx->stream);
}

static hipError_t symmetry_step(const SampleCall &c, int i, const uint32_t *ctl)
{
    Workspace &W = c.cx->ws;
    SymmetryArgs sa = symmetry_args(c.cx, W.lig_cur);
    sa.apply = 1; sa.tr_update = W.tr_update; sa.rot_update = W.rot_update;
    sa.t_dev = W.t_dev; sa.step = (uint32_t)i; sa.num_steps = (uint32_t)c.num_steps; sa.ctl = ctl;
    if (c.fuse_prep) { sa.prep_next = 1; sa.prep_pos = W.pos; sa.prep_ca4 = W.ca4; sa.prep_cb4 = W.cb4; }
    return launch_symmetry(sa, c.B, c.cx->stream);
}

// the per-call device buffers: injections, traces
static int sample_buffers(SampleCall &c, const dfm_inject *inj, const dfm_traj_out *out, DevPool &tmp)
{
    const size_t B = c.B, S = c.num_steps, N = c.cx->N, L = c.cx->L, K = c.cx->K;
    if (inj) {
        if (inj->z_rot) HIPCHK(tmp.upload(&c.zr_d, inj->z_rot, B * S * 3));
        if (inj->z_tr) HIPCHK(tmp.upload(&c.zt_d, inj->z_tr, B * S * 3));
        if (inj->edges) HIPCHK(tmp.upload(&c.ed_d, inj->edges, B * (S + 1) * N * K));
    }
    if (out->trace_pose) HIPCHK(tmp.alloc(&c.tp_d, B * S * L * 9));
    if (out->trace_scores) HIPCHK(tmp.alloc(&c.tsc_d, B * (S + 1) * 8));
    return DFM_OK;
}

// captures one step (evaluation, k_heads on the device-side scalars, restraint step, clash force, symmetry step) into cx->step_exec
static int capture_step_graph(const SampleCall &c, FwdOpts o, uint64_t key)
{
    dfm_complex *cx = c.cx;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    if (cx->step_exec) { (void)hipGraphExecDestroy(cx->step_exec); cx->step_exec = nullptr; }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    o.ctl = W.step_ctl; o.edges_dev = nullptr; o.want_energy = false; o.need_node_out = false;
    int crc = enqueue_forward(cx, c.B, o);
    if (crc == DFM_OK) {
        HeadArgs ha;
        step_head_args(c, 0, ha);
        ha.hid_base = W.hid_base; ha.step_params = W.step_params; ha.ctl = W.step_ctl;
        hipError_t e = launch_heads(ha, s);
        if (e == hipSuccess && c.restr) e = restraint_step(c, 0, W.step_ctl);
        if (e == hipSuccess && (c.flags & DFM_F_CLASH_FORCE)) e = launch_clash_force(cx->rec_pos, c.B, cx->R, cx->L, W.lig_cur, W.tr_update, s);
        if (e == hipSuccess && c.sym) e = symmetry_step(c, 0, W.step_ctl);
        if (e != hipSuccess) crc = fail(DFM_E_HIP, hipGetErrorString(e));
    }
    const std::string keep = g_err;
    hipError_t ee = hipStreamEndCapture(s, &graph);      // always: a stream left in capture mode is unusable
    if (crc != DFM_OK) { if (graph) (void)hipGraphDestroy(graph); g_err = keep; return crc; }
    if (ee != hipSuccess) return fail(DFM_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
    ee = hipGraphInstantiate(&cx->step_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ee != hipSuccess) { cx->step_exec = nullptr; return fail(DFM_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ee)); }
    cx->step_key = key; cx->step_gen = cx->buf_gen;
    return DFM_OK;
}

// Replayed step graph (DFM_F_GRAPH, or DFM_GRAPH=1 in the environment): nothing injected, traced or timed per launch.  Same
// kernels with the same arguments as the plain path - bitwise the same trajectories (tests/test_gpu_graph.py).
static int run_steps_graph(const SampleCall &c, const FwdOpts &o, bool l0)
{
    dfm_complex *cx = c.cx;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const size_t S = c.num_steps;
    std::vector<StepParams> sp(S);
    for (int i = 0; i < c.num_steps; ++i) sp[i] = step_params(c.grid, i, c.flags, c.tr_noise_scale, c.rot_noise_scale, c.num_steps);
    const uint32_t ctl_h[4] = {0u, (uint32_t)c.seed, (uint32_t)(c.seed >> 32), (uint32_t)c.num_steps};      // ([3]: the symmetry step's "last step")
    HIPCHK(hipMemcpyAsync(W.step_params, sp.data(), S * sizeof(StepParams), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(W.step_ctl, ctl_h, sizeof(ctl_h), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));      // (pageable sources: the copies have read them)
    const uint64_t key = graph_key(c.B, c.flags, l0, c.restr, c.sym);
    if (!cx->step_exec || cx->step_key != key || cx->step_gen != cx->buf_gen) {
        const int rc = capture_step_graph(c, o, key);
        if (rc) return rc;
    }
    for (int i = 0; i < c.num_steps; ++i) HIPCHK(hipGraphLaunch(cx->step_exec, s));
    cx->fwd_counter = (uint32_t)c.num_steps;      // the final evaluation draws its graph from Philox stream num_steps
    return DFM_OK;
}

// the plain step loop: evaluation, k_heads with the step's scalars by value, restraint step, clash force, symmetry step
static int run_steps(const SampleCall &c, FwdOpts o)
{
    dfm_complex *cx = c.cx;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const size_t N = cx->N, L = cx->L, K = cx->K, S = c.num_steps;
    for (int i = 0; i < c.num_steps; ++i) {
        o.edges_dev = c.ed_d ? c.ed_d + (size_t)i * N * K : nullptr;
        o.want_energy = c.step_energy; o.need_node_out = c.step_energy;
        o.pose_prepared = c.fuse_prep && i > 0;
        const int rc = enqueue_forward(cx, c.B, o);
        if (rc) return rc;
        HeadArgs ha;
        step_head_args(c, i, ha);
        if (c.fuse_prep && !c.restr && !c.sym) { ha.prep_next = 1; ha.rec_pos = cx->rec_pos; ha.prep_pos = W.pos; ha.prep_ca4 = W.ca4; ha.prep_cb4 = W.cb4; }
        HIPCHK(launch_heads(ha, s));
        if (c.restr) HIPCHK(restraint_step(c, i, nullptr));
        if (c.flags & DFM_F_CLASH_FORCE)   // inference_base.py:458-461
            HIPCHK(launch_clash_force(cx->rec_pos, c.B, cx->R, cx->L, W.lig_cur, W.tr_update, s));
        if (c.sym) HIPCHK(symmetry_step(c, i, nullptr));
        if (c.tp_d && (c.restr || c.sym || (c.flags & DFM_F_CLASH_FORCE)))      // the trace holds the pose after the whole step
            HIPCHK(hipMemcpy2DAsync(c.tp_d + (size_t)i * L * 9, S * L * 9 * 4, W.lig_cur, L * 9 * 4, L * 9 * 4, c.B, hipMemcpyDeviceToDevice, s));
    }
    return DFM_OK;
}

// final evaluation of the last pose, with the energy head (inference_base.py:463-466; same t as the last step), and the read-back
static int finish_sample(const SampleCall &c, FwdOpts o, dfm_traj_out *out)
{
    dfm_complex *cx = c.cx;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const size_t B = c.B, N = cx->N, L = cx->L, K = cx->K, S = c.num_steps;
    o.edges_dev = c.ed_d ? c.ed_d + S * N * K : nullptr;
    o.want_energy = true; o.need_node_out = true; o.pose_prepared = c.fuse_prep;
    const int rc = enqueue_forward(cx, c.B, o);
    if (rc) return rc;
    HeadArgs ha;
    fill_head_args(cx, c.B, true, &ha);
    ha.hid_base = W.hid_base + (S - 1) * 2 * HI; ha.hid_bstride = 0;      // same t as the last step
    if (c.tsc_d) { ha.trace_scores = c.tsc_d + S * 8; ha.trace_s_bstride = (int64_t)(S + 1) * 8; }
    HIPCHK(launch_heads(ha, s));
    HIPCHK(hipEventRecord(cx->ev_total[1], s));
    std::vector<float> sc(B * 8);
    HIPCHK(hipMemcpyAsync(sc.data(), W.scores, sc.size() * 4, hipMemcpyDeviceToHost, s));
    if (out->lig_pos) HIPCHK(hipMemcpyAsync(out->lig_pos, W.lig_cur, B * L * 9 * 4, hipMemcpyDeviceToHost, s));
    if (out->rot_update) HIPCHK(hipMemcpyAsync(out->rot_update, W.rot_update, B * 3 * 4, hipMemcpyDeviceToHost, s));
    if (out->tr_update) HIPCHK(hipMemcpyAsync(out->tr_update, W.tr_update, B * 3 * 4, hipMemcpyDeviceToHost, s));
    if (c.tp_d) HIPCHK(hipMemcpyAsync(out->trace_pose, c.tp_d, B * S * L * 9 * 4, hipMemcpyDeviceToHost, s));
    if (c.tsc_d) HIPCHK(hipMemcpyAsync(out->trace_scores, c.tsc_d, B * (S + 1) * 8 * 4, hipMemcpyDeviceToHost, s));
    if (c.ip_d) HIPCHK(hipMemcpyAsync(out->init_pose, c.ip_d, B * L * 9 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    unpack_scores(sc.data(), c.B, out->final_scores, out->final_scores ? out->final_scores + 3 : nullptr, 6, out->energy, out->num_clashes);
    return DFM_OK;
}

static int sample_impl(dfm_complex *cx, int B, int num_steps, float eps, float tr_noise_scale, float rot_noise_scale,
                       uint32_t flags, uint64_t seed, const dfm_inject *inj, dfm_traj_out *out, float t_first, const StartFn &start)
{
    if (!cx || !out) return fail(DFM_E_INVALID, "NULL argument");
    if (B < 1 || num_steps < 2) return fail(DFM_E_INVALID, "need B >= 1 and num_steps >= 2");
    if (num_steps > (1 << 24)) return fail(DFM_E_INVALID, "num_steps above 2^24");
    const EngineSel sel = engine_sel(flags);
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    // layer 0 through the complex's message table whenever the shipped 16-bit plan (or the fp32 engine) runs and the complex is
    // eligible - a property of the complex alone (l0_eligible), so a trajectory's bits do not depend on the batch it is sampled in
    const bool l0 = table_by_default(sel, flags) && l0_eligible(cx);
    int rc = begin_call(cx, B, sel, l0);
    if (rc) return rc;
    if ((rc = ensure_time_grid(cx, (size_t)(B > num_steps ? B : num_steps))) != DFM_OK) return rc;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    SampleCall c{cx, B, num_steps, flags, seed, tr_noise_scale, rot_noise_scale};
    if (time_grid(cx->m->hp, t_first, eps, num_steps, &c.grid) != DFM_OK)      // ValueError parity: t outside [0,1]
        return fail(DFM_E_INVALID, "Invalid t (so3 sigma needs 0 <= t <= 1)");
    DevPool tmp;   // per-call device buffers (injections, traces)
    tmp.bind(s);
    if ((rc = sample_buffers(c, inj, out, tmp)) != DFM_OK) return rc;

    // every trajectory of a step shares its time: the time-dependent half of the score-scale MLPs for the whole grid, once per call
    HIPCHK(hipMemcpyAsync(W.t_dev, c.grid.ts.data(), (size_t)num_steps * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(launch_time_embed(W.t_dev, num_steps, &cx->m->heads, W.hid_base, s));
    HIPCHK(hipEventRecord(cx->ev_total[0], s));
    if ((rc = start(tmp)) != DFM_OK) return rc;
    if (out->init_pose) {
        HIPCHK(tmp.alloc(&c.ip_d, (size_t)B * cx->L * 9));
        HIPCHK(hipMemcpyAsync(c.ip_d, W.lig_cur, (size_t)B * cx->L * 9 * 4, hipMemcpyDeviceToDevice, s));
    }
    FwdOpts o = fwd_opts(sel);
    o.profile = flags & DFM_F_PROFILE; o.seed = seed; o.edges_pitch = (int64_t)(num_steps + 1) * cx->N * cx->K;
    o.l0_table = l0;
    c.step_energy = (flags & DFM_F_STEP_ENERGY) != 0;
    static const bool graph_env_on = [] { const char *e = getenv("DFM_GRAPH"); return e && atoi(e) != 0; }();
    c.use_graph = (graph_env_on || (flags & DFM_F_GRAPH)) && !(flags & (DFM_F_PROFILE | DFM_F_STEP_ENERGY)) && !inj && !c.tp_d && !c.tsc_d;
    c.fuse_prep = !c.use_graph && !(flags & DFM_F_CLASH_FORCE);
    c.restr = (flags & DFM_F_RESTRAINTS) && cx->rs_G > 0;
    c.sym = (flags & DFM_F_SYMMETRY) && cx->sym_n > 0;
    if ((rc = c.use_graph ? run_steps_graph(c, o, l0) : run_steps(c, o)) != DFM_OK) return rc;
    if ((rc = finish_sample(c, o, out)) != DFM_OK) return rc;
    if (o.profile && (rc = finish_profile(cx)) != DFM_OK) return rc;
    return guard.done(DFM_OK);
}

extern "C" int dfm_sample(dfm_complex *cx, int B, int num_steps, float eps, float tr_noise_scale, float rot_noise_scale,
                          uint32_t flags, uint64_t seed, const dfm_inject *inj, dfm_traj_out *out)
{
    // randomize_pose (inference_base.py:318-340) at t = 1
    const StartFn start = [&](DevPool &tmp) -> int {
        float *R0_d = nullptr, *trd_d = nullptr;
        if (inj && inj->R0) HIPCHK(tmp.upload(&R0_d, inj->R0, (size_t)B * 9));
        if (inj && inj->tr_draw) HIPCHK(tmp.upload(&trd_d, inj->tr_draw, (size_t)B * 3));
        HIPCHK(launch_init_pose(cx->rec_pos, cx->lig0, B, cx->R, cx->L, cx->m->hp.family == 1, R0_d, trd_d, seed, cx->ws.lig_cur,
                                cx->ws.tr_update, cx->ws.rot_update, cx->stream));
        return DFM_OK;
    };
    return sample_impl(cx, B, num_steps, eps, tr_noise_scale, rot_noise_scale, flags, seed, inj, out, 1.0f, start);
}

// ------------------------------------------------------------------------------------------------
// Local refinement (include/dfmdock_amd.h: dfm_refine; definition: dfmdock_amd/refine.py).
// The sigma index of time t on the reference's grid (so3_diffuser.py:199-206: digitize(sigma(t), sigma(linspace(0, 1, 1000))) - 1), the
// grid sigma, and the device table of that index - built on `s` and waited for on first use, then shared by every handle of the model.
static int igso3_table(dfm_model *m, double t, hipStream_t s, int *idx_out, double *sigma_out, const double **dev_out)
{
    double st = 0.0;
    int rc = dfm_diffusion_coef(&m->hp, 1, t, nullptr, &st);
    if (rc) return rc;
    int idx = -1;
    double sg = 0.0;
    for (int i = 0; i < IGSO3_N; ++i) {      // the grid is increasing: idx = #(grid <= sigma(t)) - 1
        const double ti = i == IGSO3_N - 1 ? 1.0 : (double)i * (1.0 / (double)(IGSO3_N - 1));      // np.linspace(0, 1, 1000)
        double si = 0.0;
        dfm_diffusion_coef(&m->hp, 1, ti, nullptr, &si);
        if (si <= st) { idx = i; sg = si; } else break;
    }
    if (idx < 0) return fail(DFM_E_INVALID, "sigma(t) below the sigma grid");
    std::lock_guard<std::mutex> g(m->ig_m);
    auto it = m->ig_tab.find(idx);
    if (it == m->ig_tab.end()) {
        double *d = nullptr;
        HIPCHK(m->pool.alloc(&d, (size_t)IGSO3_N));
        HIPCHK(launch_igso3_cdf(sg, d, s));
        HIPCHK(hipStreamSynchronize(s));
        it = m->ig_tab.emplace(idx, d).first;
    }
    if (idx_out) *idx_out = idx;
    if (sigma_out) *sigma_out = sg;
    if (dev_out) *dev_out = it->second;
    return DFM_OK;
}

extern "C" int dfm_igso3_table(dfm_model *m, double t, int *sigma_idx, double *sigma, double *cdf)
{
    if (!m) return fail(DFM_E_INVALID, "NULL argument");
    DEVICE_SCOPE(m->device);
    const double *dev = nullptr;
    int rc = igso3_table(m, t, nullptr, sigma_idx, sigma, &dev);
    if (rc) return rc;
    if (cdf) HIPCHK(hipMemcpy(cdf, dev, (size_t)IGSO3_N * sizeof(double), hipMemcpyDeviceToHost));
    return DFM_OK;
}

static int fill_start_args(dfm_complex *cx, int B, float t, uint64_t seed, const dfm_refine_inject *rinj, DevPool &tmp, const double *cdf,
                           StartArgs *a)
{
    std::memset(a, 0, sizeof(*a));
    a->start = cx->lig0; a->start_bstride = 0;
    a->L = cx->L; a->all_atoms = cx->m->hp.family == 1; a->perturb = 1;
    a->cdf = cdf;
    dfm_diffusion_coef(&cx->m->hp, 0, (double)t, nullptr, &a->sigma_r3);
    a->seed_lo = (uint32_t)seed; a->seed_hi = (uint32_t)(seed >> 32);
    if (rinj) {
        float *u = nullptr, *ax = nullptr, *tr = nullptr;
        if (rinj->u_angle) HIPCHK(tmp.upload(&u, rinj->u_angle, (size_t)B));
        if (rinj->axis_draw) HIPCHK(tmp.upload(&ax, rinj->axis_draw, (size_t)B * 3));
        if (rinj->tr_draw) HIPCHK(tmp.upload(&tr, rinj->tr_draw, (size_t)B * 3));
        a->u_inj = u; a->axis_inj = ax; a->tr_inj = tr;
    }
    return DFM_OK;
}

extern "C" int dfm_forward_marginal(dfm_complex *cx, int B, float t, uint64_t seed, const dfm_refine_inject *rinj, float *rot, float *tr)
{
    if (!cx || !rot || !tr) return fail(DFM_E_INVALID, "NULL argument");
    if (B < 1) return fail(DFM_E_INVALID, "need B >= 1");
    if (!(t >= 0.0f && t <= 1.0f)) return fail(DFM_E_INVALID, "Invalid t (need 0 <= t <= 1)");
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    hipStream_t s = cx->stream;
    const double *cdf = nullptr;
    int rc = igso3_table(cx->m, (double)t, s, nullptr, nullptr, &cdf);
    if (rc) return rc;
    DevPool tmp;
    tmp.bind(s);
    StartArgs a;
    if ((rc = fill_start_args(cx, B, t, seed, rinj, tmp, cdf, &a)) != DFM_OK) return rc;
    float *o = nullptr;
    HIPCHK(tmp.alloc(&o, (size_t)B * 6));
    a.rot_update = o; a.tr_update = o + (size_t)B * 3;      // lig_cur stays NULL: the updates only
    HIPCHK(launch_start_pose(a, B, s));
    HIPCHK(hipMemcpyAsync(rot, a.rot_update, (size_t)B * 3 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(tr, a.tr_update, (size_t)B * 3 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return guard.done(DFM_OK);
}

extern "C" int dfm_refine(dfm_complex *cx, int B, int num_steps, float eps, float tr_noise_scale, float rot_noise_scale, uint32_t flags,
                          uint64_t seed, const dfm_refine_params *p, const dfm_inject *inj, const dfm_refine_inject *rinj, dfm_traj_out *out)
{
    if (!cx || !out || !p) return fail(DFM_E_INVALID, "NULL argument");
    if (B < 1 || num_steps < 2) return fail(DFM_E_INVALID, "need B >= 1 and num_steps >= 2");
    if (num_steps > (1 << 24)) return fail(DFM_E_INVALID, "num_steps above 2^24");
    if (!(p->t_begin > eps && p->t_begin <= 1.0f)) return fail(DFM_E_INVALID, "need eps < t_begin <= 1");
    if (inj && (inj->R0 || inj->tr_draw))
        return fail(DFM_E_INVALID, "dfm_inject.R0 / tr_draw belong to randomize_pose: inject the start of dfm_refine through dfm_refine_inject");
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    const double *cdf = nullptr;
    if (p->perturb) {
        int rc = igso3_table(cx->m, (double)p->t_begin, cx->stream, nullptr, nullptr, &cdf);
        if (rc) return rc;
    }
    const StartFn start = [&](DevPool &tmp) -> int {
        StartArgs a;
        int rc = fill_start_args(cx, B, p->t_begin, seed, p->perturb ? rinj : nullptr, tmp, cdf, &a);
        if (rc) return rc;
        a.perturb = p->perturb ? 1 : 0;
        if (p->start_pos) {
            float *sp = nullptr;
            HIPCHK(tmp.upload(&sp, p->start_pos, (size_t)B * cx->L * 9));
            a.start = sp; a.start_bstride = (int64_t)cx->L * 9;
        }
        a.lig_cur = cx->ws.lig_cur; a.tr_update = cx->ws.tr_update; a.rot_update = cx->ws.rot_update;
        HIPCHK(launch_start_pose(a, B, cx->stream));
        return DFM_OK;
    };
    return guard.done(sample_impl(cx, B, num_steps, eps, tr_noise_scale, rot_noise_scale, flags, seed, inj, out, p->t_begin, start));
}
