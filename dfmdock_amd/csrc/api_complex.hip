// api_complex.hip - the complex handle: creation and destruction, the stored pose, the homomer flag, the interface restraints, and the
// device memory behind a call - the workspace, the time grid and the layer-0 message table.  Everything runs on the handle's one stream.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dfm_device.h"
#include "dfm_engine.h"

using namespace dfm;

static int degree_of(const dfm_hparams &hp, int N, int *knn, int *ns)
{   // score_net_mlsb.py:89-94
    int k = hp.knn, s = hp.n_sample;
    if (N < k) { k = N; s = 0; }
    if (N < k + s) s = N - k;
    *knn = k; *ns = s;
    return k + s;
}

// layer-0 operands of the 16-bit MFMA edge kernel: SILU_S * A0 (fp32 and fp16) and SILU_S * Bm0 (fp16)
__global__ void k_scale_ab(const float *__restrict__ A0, const float *__restrict__ Bm0, float *__restrict__ A0s,
                           uint16_t *__restrict__ A0h, uint16_t *__restrict__ Bmb0, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { A0s[i] = SILU_S * A0[i]; A0h[i] = f2h(SILU_S * A0[i]); Bmb0[i] = f2h(SILU_S * Bm0[i]); }
}

// layer 0's [Wa|Wb] projection of the node embedding: pose independent, once per complex (again when the homomer flag changes)
static hipError_t project_layer0(dfm_complex *cx)
{
    const LayerDev &L0 = cx->m->layers[0];
    const int N = cx->N;
    GemmArgs g = gemm_args(cx->h0, H, H, L0.Wab, H, cx->homomer ? L0.bias_ab_h : L0.bias_ab, N, 2 * H, cx->A0, H);
    g.epi = 2; g.C2 = cx->Bm0;
    hipError_t e = launch_gemm_f32(g, cx->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_scale_ab, dim3((N * H + 255) / 256), dim3(256), token_lds(), cx->stream, cx->A0, cx->Bm0, cx->A0s, cx->A0h, cx->Bmb0, N * H);
    return hipGetLastError();
}

// "" when every coordinate of the given arrays (either may be NULL: not given) is a number, else the message of the refusal
static std::string stored_pose_error(const float *rec_pos, int R, const float *lig_pos, int L)
{
    size_t k;
    if (rec_pos && (k = first_nonfinite(rec_pos, (size_t)R * 9)) < (size_t)R * 9) return "rec_pos: residue " + std::to_string(k / 9) + " is not finite";
    if (lig_pos && (k = first_nonfinite(lig_pos, (size_t)L * 9)) < (size_t)L * 9) return "lig_pos: residue " + std::to_string(k / 9) + " is not finite";
    return "";
}

extern "C" dfm_complex *dfm_complex_create(dfm_model *m, const float *rec_x, const float *lig_x, const float *rec_pos,
                                           const float *lig_pos, int R, int L)
{
    if (!m || !rec_x || !lig_x || !rec_pos || !lig_pos) { fail(DFM_E_INVALID, "NULL argument"); return nullptr; }
    if (R < 1 || L < 1 || R + L > MAX_NODES) { fail(DFM_E_INVALID, "need 1 <= R, L and R + L <= 4096"); return nullptr; }
    // the stored pose is what the layer-0 table and the A0 / Bm0 operands are built from: it must be numbers (checked before anything
    // is created or enqueued)
    if (const std::string bad = stored_pose_error(rec_pos, R, lig_pos, L); !bad.empty()) { fail(DFM_E_INVALID, bad); return nullptr; }
    DeviceScope ds(m->device);
    if (ds.err != hipSuccess) { fail(DFM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(ds.err)); return nullptr; }
    dfm_complex *cx = new dfm_complex();
    cx->m = m; cx->device = m->device; cx->R = R; cx->L = L; cx->N = R + L;
    cx->K = degree_of(m->hp, cx->N, &cx->knn, &cx->nsamp);
    const int N = cx->N, lm = m->hp.lm_embed_dim;
    DevPool &P = cx->pool;
    // A handle's stream is NON-BLOCKING and everything the handle does - uploads included - is ordered on it: nothing here goes
    // through the legacy default stream, whose implicit synchronisation would make the creation of the next complex of a set run
    // wait for the whole dfm_sample call of the current one (driver.run_set overlaps the two from separate host threads).
    bool ok = hipStreamCreateWithFlags(&cx->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreate(&cx->ev_total[0]) == hipSuccess && hipEventCreate(&cx->ev_total[1]) == hipSuccess;
    float *x = nullptr;
    cx->pool.bind(cx->stream); cx->rs_pool.bind(cx->stream); cx->ws.pool.bind(cx->stream); cx->l0_pool.bind(cx->stream); cx->l0_pool32.bind(cx->stream);
    DevPool tmp;      // staging of the raw node features: a cached block (hipMalloc / hipFree would drain the device)
    tmp.bind(cx->stream);
    ok = ok && tmp.alloc(&x, (size_t)N * lm) == hipSuccess;
    ok = ok && hipMemcpyAsync(x, rec_x, (size_t)R * lm * sizeof(float), hipMemcpyHostToDevice, cx->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(x + (size_t)R * lm, lig_x, (size_t)L * lm * sizeof(float), hipMemcpyHostToDevice, cx->stream) == hipSuccess;
    ok = ok && P.upload_async(&cx->rec_pos, rec_pos, (size_t)R * 9, cx->stream) == hipSuccess;
    ok = ok && P.upload_async(&cx->lig0, lig_pos, (size_t)L * 9, cx->stream) == hipSuccess;
    ok = ok && P.alloc(&cx->h0, (size_t)N * H) == hipSuccess && P.alloc(&cx->A0, (size_t)N * H) == hipSuccess;
    ok = ok && P.alloc(&cx->Bm0, (size_t)N * H) == hipSuccess && P.alloc(&cx->Bmb0, (size_t)N * H) == hipSuccess;
    ok = ok && P.alloc(&cx->A0s, (size_t)N * H) == hipSuccess;
    ok = ok && P.alloc(&cx->A0h, (size_t)N * H) == hipSuccess;
#if defined(DFM_EDGE_STAMP) || defined(DFM_EDGE_TRACE)
    ok = ok && P.alloc(&cx->stamp_dev, 48 + 8 * 130) == hipSuccess && hipMemsetAsync(cx->stamp_dev, 0, (48 + 8 * 130) * 8, cx->stream) == hipSuccess;
#else      // product: four words for the message kernel's clock stamps (profiled calls only, dfm_profile::edge_shader_cycles)
    ok = ok && P.alloc(&cx->stamp_dev, 8) == hipSuccess && hipMemsetAsync(cx->stamp_dev, 0, 8 * 8, cx->stream) == hipSuccess;
#endif
    if (ok) {
        // node = single_embed(cat[rec_x, lig_x]) (score_net_mlsb.py:365-366): pose independent, once per complex
        const GemmArgs g = gemm_args(x, lm, lm, m->single_embed, lm, nullptr, N, H, cx->h0, H);
        ok = launch_gemm_f32(g, cx->stream) == hipSuccess;
        ok = ok && project_layer0(cx) == hipSuccess;
    }
    // (also on failure: the uploads above may still be reading the caller's buffers)
    const bool drained = cx->stream && hipStreamSynchronize(cx->stream) == hipSuccess;
    ok = ok && drained;
    tmp.release(drained);
    if (!ok) {
        fail(DFM_E_HIP, std::string("complex creation failed: ") + hipGetErrorString(hipGetLastError()));
        dfm_complex_destroy(cx);
        return nullptr;
    }
    return cx;
}

extern "C" void dfm_complex_destroy(dfm_complex *cx)
{
    if (!cx) return;
    DeviceScope ds(cx->device);
    bool drained = false;
    if (cx->stream) drained = hipStreamSynchronize(cx->stream) == hipSuccess;
    // every block of the handle was only ever touched by its own stream, which is drained now: no device-wide wait
    cx->ws.pool.release(drained); cx->ws.tpool.release(drained); cx->l0_pool.release(drained); cx->l0_pool32.release(drained); cx->pool.release(drained);
    cx->rs_pool.release(drained);
    if (cx->stream) (void)hipStreamDestroy(cx->stream);
    if (cx->step_exec) (void)hipGraphExecDestroy(cx->step_exec);
    for (hipEvent_t e : cx->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : cx->ev_l0) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) if (cx->ev_total[i]) (void)hipEventDestroy(cx->ev_total[i]);
    delete cx;
}

extern "C" int dfm_complex_degree(const dfm_complex *cx) { return cx ? cx->K : -1; }

extern "C" int dfm_complex_set_pose(dfm_complex *cx, const float *rec_pos, const float *lig_pos)
{
    if (!cx) return fail(DFM_E_INVALID, "NULL argument");
    // both arrays are checked before either is copied: a refused call keeps the stored pose and the tables built from it
    if (const std::string bad = stored_pose_error(rec_pos, cx->R, lig_pos, cx->L); !bad.empty()) return fail(DFM_E_INVALID, bad);
    DEVICE_SCOPE(cx->device);
    // the stream may still read the old poses (an earlier call never returns before its work is done, but stay safe)
    HIPCHK(hipStreamSynchronize(cx->stream));
    if (rec_pos) HIPCHK(hipMemcpyAsync(cx->rec_pos, rec_pos, (size_t)cx->R * 9 * sizeof(float), hipMemcpyHostToDevice, cx->stream));
    if (lig_pos) HIPCHK(hipMemcpyAsync(cx->lig0, lig_pos, (size_t)cx->L * 9 * sizeof(float), hipMemcpyHostToDevice, cx->stream));
    HIPCHK(hipStreamSynchronize(cx->stream));
    cx->l0_valid = false; cx->l0_valid32 = false;      // the intra-chain geometry may have changed: the layer-0 message tables are rebuilt on next use
    return DFM_OK;
}

extern "C" int dfm_complex_set_homomer(dfm_complex *cx, int flag)
{
    if (!cx) return fail(DFM_E_INVALID, "NULL argument");
    flag = flag ? 1 : 0;
    if (flag && cx->m->hp.positional_embed_dim != 67)
        return fail(DFM_E_INVALID, "the model has no sym channel (positional_embed_dim is 66)");
    if (flag == cx->homomer) return DFM_OK;
    DEVICE_SCOPE(cx->device);
    // the flag is committed only once the layer-0 projections that depend on it are rebuilt: a failed call leaves the old state
    // usable and a retry with the same flag does the work again instead of returning DFM_OK on stale operands
    const int old = cx->homomer;
    cx->homomer = flag;
    cx->l0_valid = false; cx->l0_valid32 = false;      // A0 carries the flag's bias: the layer-0 message tables are rebuilt on next use
    hipError_t e = project_layer0(cx);
    if (e == hipSuccess) e = hipStreamSynchronize(cx->stream);
    if (e != hipSuccess) {
        cx->homomer = old;
        (void)project_layer0(cx);                      // best effort: put the old projection back
        (void)hipStreamSynchronize(cx->stream);
        return fail(DFM_E_HIP, hipGetErrorString(e));
    }
    return DFM_OK;
}

// ------------------------------------------------------------------------------------------------
// defaults of dfm_restraint_params, tuned on four DB5 fixtures
static dfm_restraint_params default_restraint_params() { return dfm_restraint_params{0.25f, 3e-3f, 10.0f, 0.3f, 1.0f}; }

// the host checks of a restraint set; `big` = the groups of more than RS_SMALL pairs
static int check_restraints(const dfm_complex *cx, int G, const int32_t *gstart, const int32_t *pairs, const float *upper, const float *weight,
                            std::vector<int32_t> &big)
{
    if (!gstart || !pairs || !upper || !weight) return fail(DFM_E_INVALID, "restraints: NULL array");
    if (gstart[0] != 0) return fail(DFM_E_INVALID, "restraints: group_start[0] must be 0");
    for (int g = 0; g < G; ++g) {
        const long long n = (long long)gstart[g + 1] - gstart[g];
        if (n < 1) return fail(DFM_E_INVALID, "restraints: group " + std::to_string(g) + " is empty (group_start must increase)");
        if (gstart[g + 1] > RS_MAX_PAIRS) return fail(DFM_E_INVALID, "restraints: more than " + std::to_string(RS_MAX_PAIRS) + " pairs");
        if (n > RS_SMALL) big.push_back(g);
        if (!(upper[g] > 0.f) || !std::isfinite(upper[g]))
            return fail(DFM_E_INVALID, "restraints: group " + std::to_string(g) + ": upper bound must be finite and > 0");
        if (!(weight[g] >= 0.f) || !std::isfinite(weight[g]))
            return fail(DFM_E_INVALID, "restraints: group " + std::to_string(g) + ": weight must be finite and >= 0");
    }
    for (int q = 0; q < gstart[G]; ++q) {
        if (pairs[q * 2] < 0 || pairs[q * 2] >= cx->R || pairs[q * 2 + 1] < 0 || pairs[q * 2 + 1] >= cx->L)
            return fail(DFM_E_INVALID, "restraints: pair " + std::to_string(q) + " = (" + std::to_string(pairs[q * 2]) + ", " +
                                           std::to_string(pairs[q * 2 + 1]) + ") outside [0, R) x [0, L) = [0, " + std::to_string(cx->R) +
                                           ") x [0, " + std::to_string(cx->L) + ")");
    }
    return DFM_OK;
}

extern "C" int dfm_complex_set_restraints(dfm_complex *cx, int G, const int32_t *gstart, const int32_t *pairs, const float *upper,
                                          const float *weight, const dfm_restraint_params *par)
{
    if (!cx) return fail(DFM_E_INVALID, "NULL argument");
    if (G < 0 || G > RS_MAX_GROUPS) return fail(DFM_E_INVALID, "restraints: need 0 <= n_groups <= " + std::to_string(RS_MAX_GROUPS));
    dfm_restraint_params pr = par ? *par : default_restraint_params();
    if (!(pr.k_tr >= 0.f) || !(pr.k_rot >= 0.f) || !(pr.max_tr >= 0.f) || !(pr.max_rot >= 0.f) || !std::isfinite(pr.k_tr) ||
        !std::isfinite(pr.k_rot) || !std::isfinite(pr.max_tr) || !std::isfinite(pr.max_rot) || std::isnan(pr.t_start))
        return fail(DFM_E_INVALID, "restraints: k_tr, k_rot, max_tr, max_rot must be finite and >= 0, t_start a number");
    std::vector<int32_t> big;
    if (G > 0) {
        const int rc = check_restraints(cx, G, gstart, pairs, upper, weight, big);
        if (rc) return rc;
    }
    DEVICE_SCOPE(cx->device);
    HIPCHK(hipStreamSynchronize(cx->stream));      // nothing in flight reads the old set any more
    DevPool np;
    np.bind(cx->stream);
    int32_t *d_gs = nullptr, *d_pairs = nullptr, *d_big = nullptr;
    float *d_up = nullptr, *d_w = nullptr;
    if (G > 0) {
        const size_t P = (size_t)gstart[G];
        hipError_t e = np.upload_async(&d_gs, gstart, (size_t)G + 1, cx->stream);
        if (e == hipSuccess) e = np.upload_async(&d_pairs, pairs, P * 2, cx->stream);
        if (e == hipSuccess) e = np.upload_async(&d_up, upper, (size_t)G, cx->stream);
        if (e == hipSuccess) e = np.upload_async(&d_w, weight, (size_t)G, cx->stream);
        if (e == hipSuccess && !big.empty()) e = np.upload_async(&d_big, big.data(), big.size(), cx->stream);
        const hipError_t es = hipStreamSynchronize(cx->stream);
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) { np.release(es == hipSuccess); return fail(DFM_E_HIP, std::string("restraints upload: ") + hipGetErrorString(e)); }
    }
    std::swap(cx->rs_pool.ptrs, np.ptrs);
    np.release(true);      // the old set
    cx->rs_gstart = d_gs; cx->rs_pairs = d_pairs; cx->rs_big = d_big; cx->rs_upper = d_up; cx->rs_weight = d_w;
    cx->rs_G = G; cx->rs_nbig = (int)big.size(); cx->rs_par = pr;
    // the captured step graph holds the old set's pointers and parameters by value: capture again on the next call
    if (cx->step_exec) { (void)hipGraphExecDestroy(cx->step_exec); cx->step_exec = nullptr; }
    return DFM_OK;
}

RestraintArgs dfm::restraint_args(const dfm_complex *cx, float *lig)
{
    RestraintArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rec_pos = cx->rec_pos; a.R = cx->R; a.L = cx->L; a.all_atoms = cx->m->hp.family == 1;
    a.gstart = cx->rs_gstart; a.pairs = cx->rs_pairs; a.upper = cx->rs_upper; a.weight = cx->rs_weight; a.big = cx->rs_big;
    a.G = cx->rs_G; a.n_big = cx->rs_nbig;
    a.k_tr = cx->rs_par.k_tr; a.k_rot = cx->rs_par.k_rot; a.max_tr = cx->rs_par.max_tr; a.max_rot = cx->rs_par.max_rot;
    a.t_start = cx->rs_par.t_start;
    a.lig = lig;
    return a;
}

extern "C" int dfm_restraint_eval(dfm_complex *cx, int B, const float *lig_pos, float *energy, int32_t *n_satisfied, float *step)
{
    if (!cx || !lig_pos || !energy || !n_satisfied) return fail(DFM_E_INVALID, "NULL argument");
    if (B < 1) return fail(DFM_E_INVALID, "need B >= 1");
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    DevPool tmp;
    tmp.bind(cx->stream);
    float *lig = nullptr, *o = nullptr;
    HIPCHK(tmp.upload_async(&lig, lig_pos, (size_t)B * cx->L * 9, cx->stream));
    HIPCHK(tmp.alloc(&o, (size_t)B * 8));
    RestraintArgs a = restraint_args(cx, lig);
    a.out = o;
    HIPCHK(launch_restraint(a, B, cx->stream));
    std::vector<float> h((size_t)B * 8);
    HIPCHK(hipMemcpyAsync(h.data(), o, h.size() * 4, hipMemcpyDeviceToHost, cx->stream));
    HIPCHK(hipStreamSynchronize(cx->stream));
    for (int b = 0; b < B; ++b) {
        energy[b] = h[(size_t)b * 8];
        n_satisfied[b] = (int32_t)h[(size_t)b * 8 + 1];
        if (step) std::memcpy(step + (size_t)b * 6, &h[(size_t)b * 8 + 2], 6 * sizeof(float));
    }
    return guard.done(DFM_OK);
}

// ------------------------------------------------------------------------------------------------
// defaults of dfm_symmetry_params: starting values, not measured against a trained checkpoint
static dfm_symmetry_params default_symmetry_params() { return dfm_symmetry_params{0.5f, 0.5f, 0.3f, 10.0f, 1.0f, 1}; }

extern "C" int dfm_complex_set_symmetry(dfm_complex *cx, int n, const dfm_symmetry_params *par)
{
    if (!cx) return fail(DFM_E_INVALID, "NULL argument");
    dfm_symmetry_params pr = par ? *par : default_symmetry_params();
    if (n != 0) {
        if (n < SYM_MIN_ORDER || n > SYM_MAX_ORDER)
            return fail(DFM_E_INVALID, "symmetry: need n = 0 or " + std::to_string(SYM_MIN_ORDER) + " <= n <= " + std::to_string(SYM_MAX_ORDER));
        if (cx->R != cx->L)
            return fail(DFM_E_INVALID, "symmetry: receptor and ligand must be the same chain (R = " + std::to_string(cx->R) + ", L = " +
                                           std::to_string(cx->L) + ")");
    }
    if (n == 0) pr = default_symmetry_params();      // a clear takes no parameters: whatever p points at is ignored
    if (!(pr.gain_rot > 0.f && pr.gain_rot <= 1.f) || !(pr.gain_tr > 0.f && pr.gain_tr <= 1.f))
        return fail(DFM_E_INVALID, "symmetry: gain_rot and gain_tr must lie in (0, 1]");
    if (!(pr.max_rot > 0.f) || !(pr.max_tr > 0.f) || !std::isfinite(pr.max_rot) || !std::isfinite(pr.max_tr) || std::isnan(pr.t_start))
        return fail(DFM_E_INVALID, "symmetry: max_rot and max_tr must be finite and > 0, t_start a number");
    DEVICE_SCOPE(cx->device);
    HIPCHK(hipStreamSynchronize(cx->stream));
    cx->sym_n = n; cx->sym_par = pr;
    // the captured step graph holds the order and the parameters by value (or no symmetry step at all): capture again on the next call
    if (cx->step_exec) { (void)hipGraphExecDestroy(cx->step_exec); cx->step_exec = nullptr; }
    return DFM_OK;
}

SymmetryArgs dfm::symmetry_args(const dfm_complex *cx, float *lig)
{
    SymmetryArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rec_pos = cx->rec_pos; a.R = cx->R; a.L = cx->L; a.all_atoms = cx->m->hp.family == 1;
    a.n = cx->sym_n;
    a.gain_rot = cx->sym_par.gain_rot; a.gain_tr = cx->sym_par.gain_tr; a.max_rot = cx->sym_par.max_rot; a.max_tr = cx->sym_par.max_tr;
    a.t_start = cx->sym_par.t_start; a.snap_last = cx->sym_par.snap_last ? 1 : 0;
    a.lig = lig;
    return a;
}

extern "C" int dfm_symmetry_eval(dfm_complex *cx, int B, const float *lig_pos, dfm_symmetry_out *out)
{
    if (!cx || !lig_pos || !out || !out->step) return fail(DFM_E_INVALID, "NULL argument");
    if (B < 1) return fail(DFM_E_INVALID, "need B >= 1");
    const size_t nb = (size_t)B;
    if (cx->sym_n == 0) {      // nothing stored: zeros, as dfm_restraint_eval
        if (out->theta) std::memset(out->theta, 0, nb * sizeof(double));
        if (out->screw) std::memset(out->screw, 0, nb * sizeof(double));
        if (out->axis) std::memset(out->axis, 0, nb * 3 * sizeof(double));
        if (out->axis_point) std::memset(out->axis_point, 0, nb * 3 * sizeof(double));
        if (out->fit_rmsd) std::memset(out->fit_rmsd, 0, nb * sizeof(double));
        if (out->sym_rmsd) std::memset(out->sym_rmsd, 0, nb * sizeof(double));
        if (out->order_m) std::memset(out->order_m, 0, nb * sizeof(int32_t));
        std::memset(out->step, 0, nb * 6 * sizeof(float));
        return DFM_OK;
    }
    DEVICE_SCOPE(cx->device);
    CallGuard guard(cx->stream);
    DevPool tmp;
    tmp.bind(cx->stream);
    float *lig = nullptr, *st = nullptr;
    double *o = nullptr;
    HIPCHK(tmp.upload_async(&lig, lig_pos, nb * cx->L * 9, cx->stream));
    HIPCHK(tmp.alloc(&o, nb * SYM_OUT));
    HIPCHK(tmp.alloc(&st, nb * 6));
    SymmetryArgs a = symmetry_args(cx, lig);
    a.out = o; a.step_out = st;
    HIPCHK(launch_symmetry(a, B, cx->stream));
    std::vector<double> h(nb * SYM_OUT);
    HIPCHK(hipMemcpyAsync(h.data(), o, h.size() * sizeof(double), hipMemcpyDeviceToHost, cx->stream));
    HIPCHK(hipMemcpyAsync(out->step, st, nb * 6 * sizeof(float), hipMemcpyDeviceToHost, cx->stream));
    HIPCHK(hipStreamSynchronize(cx->stream));
    for (size_t b = 0; b < nb; ++b) {
        const double *r = &h[b * SYM_OUT];
        if (out->theta) out->theta[b] = r[0];
        if (out->screw) out->screw[b] = r[1];
        if (out->axis) std::memcpy(out->axis + b * 3, r + 2, 3 * sizeof(double));
        if (out->axis_point) std::memcpy(out->axis_point + b * 3, r + 5, 3 * sizeof(double));
        if (out->fit_rmsd) out->fit_rmsd[b] = r[8];
        if (out->sym_rmsd) out->sym_rmsd[b] = r[9];
        if (out->order_m) out->order_m[b] = (int32_t)r[10];
    }
    return guard.done(DFM_OK);
}

// ------------------------------------------------------------------------------------------------
// Layer 0 behind the message table: budgets.  The table costs 516 B per intra-chain ordered pair (8 M pairs = 4.1 GB: 2000 + 2000
// residues); beyond it layer 0 is evaluated directly (DFM_L0_TABLE=0 in the environment: always).  Eligibility is a property of the
// COMPLEX alone (r04 also switched to the direct evaluation above 32 M edges per batched evaluation, so a trajectory's bits
// changed with the batch size at B = 890 for 300+300): the per-batch buffers cost 532 B per edge of a batched evaluation (19 MB per
// trajectory at 300+300, next to 14 MB of workspace) for every batch the 2^31-byte guard of ensure_workspace admits; a batch whose
// buffers do not fit fails with DFM_E_OOM - split it, or pass DFM_F_NO_L0_TABLE - instead of silently changing the arithmetic.
constexpr long long L0_MAX_PAIRS = 8ll << 20;
bool dfm::l0_eligible(const dfm_complex *cx)
{
    static const bool env_off = [] { const char *e = getenv("DFM_L0_TABLE"); return e && atoi(e) == 0; }();
    if (env_off || cx->m->hp.depth < 2) return false;      // (a depth-1 model's first layer is its last: it stores messages for the coordinate MLP)
    const long long pairs = (long long)cx->R * cx->R + (long long)cx->L * cx->L;
    return pairs <= L0_MAX_PAIRS;
}

constexpr int MIN_TIME_GRID = 4096;      // smallest time grid the workspace is sized for (dfm_sample grows it for longer schedules)
// t_dev [n], hid_base [n][2][128], step_params [n]: one entry per trajectory (dfm_score) or per step of the time grid (dfm_sample).
// The reference's sampler takes any num_steps (inference_base.py:403-404: np.linspace(1, eps, num_steps)), so does this one.
int dfm::ensure_time_grid(dfm_complex *cx, size_t n)
{
    Workspace &W = cx->ws;
    if (n < (size_t)MIN_TIME_GRID) n = MIN_TIME_GRID;
    if (n <= W.Tcap) return DFM_OK;
    HIPCHK(hipStreamSynchronize(cx->stream));
    W.tpool.release(true);
    W.tpool.bind(cx->stream);
    W.Tcap = 0;
    cx->buf_gen++;
    HIPCHK(W.tpool.alloc(&W.t_dev, n)); HIPCHK(W.tpool.alloc(&W.hid_base, n * 2 * HI)); HIPCHK(W.tpool.alloc(&W.step_params, n));
    W.Tcap = n;
    return DFM_OK;
}

// the per-trajectory buffers of a workspace of capacity B (the caller has released the old ones)
static int alloc_workspace(dfm_complex *cx, int B)
{
    Workspace &W = cx->ws;
    const size_t N = cx->N, L = cx->L, R = cx->R, K = cx->K, b = B;
    HIPCHK(W.pool.alloc(&W.pos, b * N)); HIPCHK(W.pool.alloc(&W.ca4, b * N)); HIPCHK(W.pool.alloc(&W.cb4, b * N));
    HIPCHK(W.pool.alloc(&W.edges, b * N * K)); HIPCHK(W.pool.alloc(&W.codes, b * N * K));
    HIPCHK(W.pool.alloc(&W.radial, b * N * K));
    HIPCHK(W.pool.alloc(&W.h, b * N * H)); HIPCHK(W.pool.alloc(&W.h2, b * N * H));
    HIPCHK(W.pool.alloc(&W.A, b * N * H)); HIPCHK(W.pool.alloc(&W.Bm, b * N * H));
    HIPCHK(W.pool.alloc(&W.Bmb, b * N * H)); HIPCHK(W.pool.alloc(&W.agg, b * N * H));
    HIPCHK(W.pool.alloc(&W.u, b * N * H));
    HIPCHK(W.pool.alloc(&W.gn_shift, b * H)); HIPCHK(W.pool.alloc(&W.gn_den, b * H));
    HIPCHK(W.pool.alloc(&W.gn_part, b * ((N + 31) / 32) * H * 2));      // (mean, M2) per 32-row half of a GEMM tile, trajectory and channel
    const size_t RT = (R + 63) / 64, NP = R > 4 * RT ? R : 4 * RT;     // partial-sum slots per trajectory
    HIPCHK(W.pool.alloc(&W.fvec, b * L * 3)); HIPCHK(W.pool.alloc(&W.en_part, b * NP * 2));
    HIPCHK(W.pool.alloc(&W.clash_part, b * NP)); HIPCHK(W.pool.alloc(&W.scores, b * 8));
    if (cx->m->hp.family == 1) {
        HIPCHK(W.pool.alloc(&W.fpart, b * RT * L * 3)); HIPCHK(W.pool.alloc(&W.cpart, b * RT * 4 * 2));
        HIPCHK(W.pool.alloc(&W.conf, b));
        HIPCHK(W.pool.alloc(&W.pair_s, b * L * (((R + 31) / 32) * 32)));
    }
    HIPCHK(W.pool.alloc(&W.lig_cur, b * L * 9)); HIPCHK(W.pool.alloc(&W.tr_update, b * 3));
    HIPCHK(W.pool.alloc(&W.rot_update, b * 3));
    HIPCHK(W.pool.alloc(&W.step_ctl, 4));
    HIPCHK(W.pool.alloc(&W.task_ctr, 2 * TASK_CTR_WGS));
    HIPCHK(hipMemsetAsync(W.task_ctr, 0, 2 * TASK_CTR_WGS * sizeof(uint32_t), cx->stream));
    return ensure_time_grid(cx, b);
}

// the layer-0 buffers of this batch capacity: all of them or none.  A batch whose row buffers do not fit does not
// leave a half-allocated workspace behind, and the error says how to run it anyway.
static int alloc_l0_buffers(dfm_complex *cx, bool bf16)
{
    Workspace &W = cx->ws;
    const size_t cap = (size_t)W.Bcap * cx->N * cx->K;      // every edge of a batched evaluation may miss the table
    const size_t mark = W.pool.ptrs.size();
    const bool had_src = W.l0_src != nullptr, had_x = W.l0_x != nullptr, had_x32 = W.l0_x32 != nullptr;
    hipError_t e = hipSuccess;
    if (!had_src) {
        cx->buf_gen++;
        e = W.pool.alloc(&W.l0_src, cap);
        if (e == hipSuccess) e = W.pool.alloc(&W.l0_rows, cap);
        if (e == hipSuccess) e = W.pool.alloc(&W.l0_counter, 1);
        if (e == hipSuccess) e = W.pool.alloc(&W.l0_miss_total, 1);
        if (e == hipSuccess) e = hipMemsetAsync(W.l0_counter, 0, sizeof(uint32_t), cx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(W.l0_miss_total, 0, sizeof(unsigned long long), cx->stream);
    }
    if (e == hipSuccess && bf16 && !had_x) { cx->buf_gen++; e = W.pool.alloc(&W.l0_x, (cap + 32) * H); }      // the last tile of the row list stores all of its 32 rows
    if (e == hipSuccess && !bf16 && !had_x32) { cx->buf_gen++; e = W.pool.alloc(&W.l0_x32, cap * H); }         // fp32 engine: only the list's own rows are stored
    if (e == hipSuccess) return DFM_OK;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(cx->stream);
    W.pool.release_tail(mark);
    if (!had_src) { W.l0_src = nullptr; W.l0_rows = nullptr; W.l0_counter = nullptr; W.l0_miss_total = nullptr; }
    if (!had_x) W.l0_x = nullptr;
    if (!had_x32) W.l0_x32 = nullptr;
    char msg[256];
    snprintf(msg, sizeof(msg), "layer-0 message table: the row buffers of a batch of %d (%zu B per edge, %.1f GB) do not fit (%s): split the "
             "batch or evaluate layer 0 directly (DFM_F_NO_L0_TABLE / leave DFM_F_L0_TABLE out)", W.Bcap, bf16 ? (size_t)532 : (size_t)1044,
             (double)cap * (bf16 ? 532.0 : 1044.0) / 1e9, hipGetErrorString(e));
    return fail(e == hipErrorOutOfMemory ? DFM_E_OOM : DFM_E_HIP, msg);
}

int dfm::ensure_workspace(dfm_complex *cx, int B, bool bf16, bool l0)
{
    Workspace &W = cx->ws;
    // the 16-bit message kernel addresses edges / codes / radial through buffer descriptors rooted at the whole [B][N][K] arrays with
    // 32-bit byte offsets: past 2 GiB the loads would silently return 0
    if ((unsigned long long)B * (unsigned long long)cx->N * (unsigned long long)cx->K * 4ull >= (1ull << 31))
        return fail(DFM_E_INVALID, "B * N * K * 4 must stay below 2^31: split the batch");
    const bool wants_mbuf = bf16 && cx->m->hp.family == 0;    // gated messages for the coordinate MLP (family 0 only)
    const bool need_mbuf = wants_mbuf && !W.mbuf;
    const bool need_l0 = l0 && (!W.l0_src || (bf16 ? !W.l0_x : !W.l0_x32));
    if (B <= W.Bcap && !need_mbuf && !need_l0) return DFM_OK;
    if (B > W.Bcap) {
        HIPCHK(hipStreamSynchronize(cx->stream));
        W.pool.release(true); W.tpool.release(true);
        W = Workspace();
        W.pool.bind(cx->stream);
        cx->buf_gen++;
        const int rc = alloc_workspace(cx, B);
        if (rc) return rc;
        W.Bcap = B;
    }
    if (wants_mbuf && !W.mbuf) { HIPCHK(W.pool.alloc(&W.mbuf, (size_t)W.Bcap * cx->L * KPAD * H)); cx->buf_gen++; }
    return l0 ? alloc_l0_buffers(cx, bf16) : DFM_OK;
}

// ------------------------------------------------------------------------------------------------
// operands of layer 0's message kernel in the shipped 16-bit plan: the complex's own, pose-independent A0 / Bm0 (no batch stride)
static EdgeArgs layer0_edge_args(const dfm_complex *cx)
{
    EdgeArgs e;
    std::memset(&e, 0, sizeof(e));
    e.A = cx->A0s; e.Bm = cx->Bm0; e.Bmb = cx->Bmb0; e.Ah = cx->A0h; e.ab_bstride = 0;
    e.B = 1; e.N = cx->N; e.R = cx->R; e.K = cx->K; e.lw = &cx->m->layers[0]; e.f16 = 1;
    return e;
}
static EdgeArgs layer0_edge_args32(const dfm_complex *cx)      // fp32 engine: the complex's own fp32 A0 / Bm0
{
    EdgeArgs e;
    std::memset(&e, 0, sizeof(e));
    e.A = cx->A0; e.Bm = cx->Bm0; e.Bmb = cx->Bmb0; e.ab_bstride = 0;
    e.B = 1; e.N = cx->N; e.R = cx->R; e.K = cx->K; e.lw = &cx->m->layers[0];
    return e;
}

// Builds the layer-0 message table of the complex: every intra-chain ordered pair (i, j) through the edge model once, features from
// the stored pose (any rigid placement of the ligand gives the same intra-chain geometry; k_edge_feat checks the bins per pose).
// Uses trajectory slot 0 of the workspace (ensure_workspace first) and overwrites ws.lig_cur's first pose.  Synchronises.
int dfm::build_l0_table(dfm_complex *cx, float *build_ms, bool fp32)
{
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const size_t R = cx->R, L = cx->L, P = R * R + L * L;
    (fp32 ? cx->l0_valid32 : cx->l0_valid) = false;
    HIPCHK(hipStreamSynchronize(s));
    (fp32 ? cx->l0_pool32 : cx->l0_pool).release(true);
    cx->buf_gen++;
    uint2 *code0 = nullptr;
    if (fp32) {
        HIPCHK(cx->l0_pool32.alloc(&cx->l0_table32, P * H));
        HIPCHK(cx->l0_pool32.alloc(&cx->l0_code0_32, P));
        code0 = cx->l0_code0_32;
    } else {
        HIPCHK(cx->l0_pool.alloc(&cx->l0_table, ((P + 31) / 32 * 32) * H));
        HIPCHK(cx->l0_pool.alloc(&cx->l0_code0, P));
        code0 = cx->l0_code0;
    }
    DevPool tmp;
    tmp.bind(s);
    uint4 *rows = nullptr;
    HIPCHK(tmp.alloc(&rows, P));
    HIPCHK(hipEventRecord(cx->ev_total[0], s));
    HIPCHK(hipMemcpyAsync(W.lig_cur, cx->lig0, L * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(launch_prep_pose(cx->rec_pos, W.lig_cur, 1, cx->R, cx->L, cx->m->hp.family == 1 ? 1 : 0, W.pos, W.ca4, W.cb4, s));
    HIPCHK(launch_l0_pairs(W.pos, W.ca4, W.cb4, cx->R, cx->L, cx->m->hp.mask_dist, code0, rows, s));
    if (fp32) HIPCHK(launch_edge_rows32(layer0_edge_args32(cx), rows, nullptr, (uint32_t)P, cx->l0_table32, s));
    else HIPCHK(launch_edge_rows(layer0_edge_args(cx), rows, nullptr, (uint32_t)P, cx->l0_table, s));
    HIPCHK(hipEventRecord(cx->ev_total[1], s));
    HIPCHK(hipStreamSynchronize(s));
    tmp.release(true);
    if (build_ms) HIPCHK(hipEventElapsedTime(build_ms, cx->ev_total[0], cx->ev_total[1]));
    (fp32 ? cx->l0_valid32 : cx->l0_valid) = true;
    return DFM_OK;
}
