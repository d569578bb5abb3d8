// dfm_engine.h - what the translation units of the engine's host code share (not part of the C ABI): the workspace and the complex
// handle, the options of one score evaluation, and the helpers that cross files.
//   api.hip          globals, device, hyper-parameters, diffusion coefficients, configuration string, cache and diagnostics calls
//   api_model.hip    the weight blob's map, the packers, dfm_model_create / destroy
//   api_complex.hip  the complex handle: lifecycle, pose, homomer flag, restraints, symmetry, workspace, time grid, layer-0 message table
//   api_forward.hip  one batched score evaluation (enqueue_forward), the scaffold of a public call, the profile read-out
//   api_score.hip    dfm_score, dfm_score_distogram, dfm_complex_selfcheck
//   api_sample.hip   the sampler behind dfm_sample and dfm_refine, the IGSO(3) tables, dfm_forward_marginal
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "dfm_host.h"

namespace dfm {

struct Workspace {
    int Bcap = 0;
    DevPool pool;
    float4 *pos = nullptr, *ca4 = nullptr, *cb4 = nullptr;      // centred backbone N / CA / virtual CB of every trajectory, [B][N] each
    int32_t *edges = nullptr; uint32_t *codes = nullptr; float *radial = nullptr;
    float *h = nullptr, *h2 = nullptr, *A = nullptr, *Bm = nullptr, *agg = nullptr, *u = nullptr;
    uint16_t *Bmb = nullptr, *mbuf = nullptr;
    float *gn_shift = nullptr, *gn_den = nullptr, *gn_part = nullptr;
    float *fvec = nullptr, *en_part = nullptr; int32_t *clash_part = nullptr;
    float *fpart = nullptr, *cpart = nullptr, *conf = nullptr;    // family 1: force partials per receptor tile, confidence
    float *pair_s = nullptr;                                      // family 1, 16-bit engines: s(r, l) of one pair head, [B][L][32 ceil(R / 32)]
    float *scores = nullptr, *lig_cur = nullptr, *tr_update = nullptr, *rot_update = nullptr, *t_dev = nullptr;
    float *hid_base = nullptr;       // [max(Bcap, 1024)][2][128]: time-dependent half of the score-scale MLPs (k_time_embed), per trajectory
                                     // (dfm_score) or per step of the time grid (dfm_sample)
    float *ir1 = nullptr, *ir2 = nullptr, *ir3 = nullptr;      // to_ires scratch, allocated on the first DFM_F_IRES call
    // layer 0 behind the message table (allocated on first use): per edge the source of its gated message, the row list of the
    // edges the edge model still evaluates, their messages, the list's length and the running total for the profile
    uint32_t *task_ctr = nullptr;      // per-workgroup task + exit counters of the 16-bit message kernel (dynamic tasks, kernels_edge.hip)
    uint32_t *l0_src = nullptr; uint4 *l0_rows = nullptr; uint16_t *l0_x = nullptr; uint32_t *l0_counter = nullptr;
    float *l0_x32 = nullptr;      // fp32 engine: the row list's messages (1 KiB per row)
    unsigned long long *l0_miss_total = nullptr;
    // replayed step graph: {evaluations started, seed lo, seed hi, num_steps} and the per-step scalars of the call's time grid
    uint32_t *step_ctl = nullptr; StepParams *step_params = nullptr;
    // t_dev / hid_base / step_params live in their own pool, sized for max(Bcap, the longest time grid asked for so far)
    DevPool tpool;
    size_t Tcap = 0;
};

}  // namespace dfm

struct dfm_complex {
    dfm_model *m = nullptr;
    int device = 0;
    int homomer = 0;                 // value of the 67th position channel (positional_embed_dim 67)
    int R = 0, L = 0, N = 0, K = 0, knn = 0, nsamp = 0;
    dfm::DevPool pool;
    float *rec_pos = nullptr, *lig0 = nullptr;
    float *h0 = nullptr, *A0 = nullptr, *Bm0 = nullptr;
    float *A0s = nullptr; uint16_t *Bmb0 = nullptr;   // SILU_S * A0 (fp32), SILU_S * Bm0 (fp16): layer-0 operands of the 16-bit engines
    uint16_t *A0h = nullptr;                          // SILU_S * A0 as fp16 (bf16-operand message kernel)
    dfm::Workspace ws;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;      // profiling events (pairs)
    std::vector<char> ev_lig;        // per pair: the launch covered the ligand nodes only
    size_t ev_used = 0;
    hipEvent_t ev_total[2] = {nullptr, nullptr};
    dfm_profile prof = {};
    unsigned long long *stamp_dev = nullptr;   // [8 waves][4 phases] (diagnostic builds)
    uint32_t fwd_counter = 0;
    // layer-0 message table of the 16-bit engine (kernels_edge.hip: k_l0_gather): gated messages of every intra-chain ordered pair
    // [R*R + L*L][256] fp16 and the feature code each entry was built with; rebuilt after set_pose / set_homomer
    dfm::DevPool l0_pool, l0_pool32;
    uint16_t *l0_table = nullptr; uint2 *l0_code0 = nullptr;
    bool l0_valid = false;
    float *l0_table32 = nullptr; uint2 *l0_code0_32 = nullptr; bool l0_valid32 = false;      // the fp32 engine's table (1 KiB per pair)
    std::vector<hipEvent_t> ev_l0;   // profiling events of the table path (triples: before rows | between | after gather)
    size_t ev_l0_used = 0;
    // One step of dfm_sample (score evaluation + heads + Euler-Maruyama update [+ clash force]) captured as a hipGraph and replayed
    // num_steps times: every per-step / per-call scalar is read from device memory (ws.step_ctl, ws.step_params), so the nodes are
    // the same in every step AND every call - the executable graph is kept until the buffers it points into move
    hipGraphExec_t step_exec = nullptr;
    uint64_t step_key = 0;       // dfm::graph_key the graph was captured for
    uint64_t buf_gen = 0;        // bumped whenever a buffer a captured launch points into is re-allocated (workspace, message table)
    uint64_t step_gen = ~0ull;   // buf_gen at capture
    // interface restraints (dfm_complex_set_restraints): the set in its own pool, replaced as a whole
    dfm::DevPool rs_pool;
    int32_t *rs_gstart = nullptr, *rs_pairs = nullptr, *rs_big = nullptr;
    float *rs_upper = nullptr, *rs_weight = nullptr;
    int rs_G = 0, rs_nbig = 0;
    dfm_restraint_params rs_par = {};
    // Cn symmetry (dfm_complex_set_symmetry): the order (0: none stored) and the step's parameters
    int sym_n = 0;
    dfm_symmetry_params sym_par = {};
};

namespace dfm {

// options of one score evaluation (enqueue_forward)
struct FwdOpts {
    bool bf16 = false, f16 = false, want_energy = false, profile = false;   // bf16: 16-bit MFMA engine; f16: ... with fp32 A_i
    bool bf16_ops = false;                // bf16 MFMA operands in every layer but the last (DFM_F_BF16_OPS)
    bool pose_prepared = false;           // ws.pos / ca4 / cb4 already hold this evaluation's pose (written by the previous step's k_heads)
    uint32_t *ctl = nullptr;              // replayed step graph: device {evaluation index, seed} block (ws.step_ctl) instead of by-value seed / stream id
    bool l0_table = false;                // layer 0 through the complex's message table (cx->l0_valid, workspace l0 buffers allocated)
    bool need_node_out = true;            // false: nobody reads the final node features (no energy / ires / debug tap) - the last layer then
                                          // computes the messages of the ligand nodes only (all the coordinate update reads) and no node model
    const int32_t *edges_dev = nullptr;   // [B][N][K] already on device (or nullptr = sample natively)
    int64_t edges_pitch = 0;              // elements between trajectories in edges_dev
    uint64_t seed = 0;
    float *h_first_out = nullptr;         // device [B][N][H] tap (dfm_score debug)
    // dfm_complex_selfcheck only: running maxima (float bits) [depth + 1][8] = per layer |h in|, |A|, |Bm|, |pre-activation 0|,
    // |pre-activation 2| of the fp32 pass; fp16 values found at the saturation value in A / Bm of a 16-bit pass
    uint32_t *range = nullptr;
    unsigned long long *sat = nullptr;
};
// the engine of `sel`, every other option at its default
inline FwdOpts fwd_opts(const EngineSel &sel)
{
    FwdOpts o;
    o.bf16 = sel.bf16; o.f16 = sel.f16; o.bf16_ops = sel.bf16_ops;
    return o;
}

// Every public call that enqueues on a handle's stream holds one of these from its DEVICE_SCOPE on.  A call that leaves without
// done(DFM_OK) - any early return - drains the stream first: nothing then still reads the call's own buffers or writes the caller's
// arrays.  A call that succeeds has synchronised already and pays nothing.
struct CallGuard {
    hipStream_t s;
    bool ok = false;
    explicit CallGuard(hipStream_t stream) : s(stream) {}
    CallGuard(const CallGuard &) = delete;
    ~CallGuard() { if (!ok) (void)hipStreamSynchronize(s); }
    int done(int rc) { ok = rc == DFM_OK; return rc; }
};

// a zeroed GemmArgs with the operands every GEMM names: C [M][ldc] = A0 [M][lda] (K columns) x W [Nout][ldw]^T + bias
inline GemmArgs gemm_args(const float *A0, int lda, int K, const float *W, int ldw, const float *bias, int M, int Nout, float *C, int ldc)
{
    GemmArgs g;
    std::memset(&g, 0, sizeof(g));
    g.A0 = A0; g.lda = lda; g.K = K; g.W = W; g.ldw = ldw; g.bias = bias; g.M = M; g.Nout = Nout; g.C = C; g.ldc = ldc;
    return g;
}
// 16-bit engines: three-term split-bf16 on the pre-split tiles hi / lo; the fp32 engine: g.W
inline hipError_t launch_gemm(bool bf16, const GemmArgs &g, const uint16_t *hi, const uint16_t *lo, hipStream_t s)
{
    return bf16 ? launch_gemm_split(g, hi, lo, s) : launch_gemm_f32(g, s);
}

// ---- api_model.hip
int64_t blob_floats(const dfm_hparams *hp);      // floats of a weight blob with these hyper-parameters

// ---- api_complex.hip
bool l0_eligible(const dfm_complex *cx);
int ensure_time_grid(dfm_complex *cx, size_t n);
int ensure_workspace(dfm_complex *cx, int B, bool bf16, bool l0);
int build_l0_table(dfm_complex *cx, float *build_ms, bool fp32);
RestraintArgs restraint_args(const dfm_complex *cx, float *lig);
SymmetryArgs symmetry_args(const dfm_complex *cx, float *lig);

// ---- api_forward.hip
// start of a public call: the workspace for B trajectories of this engine (with the layer-0 buffers when l0), the profile, the event
// cursors and the evaluation counter back to zero, the message table built if it is not valid (l0_build_ms), its miss total zeroed
int begin_call(dfm_complex *cx, int B, const EngineSel &sel, bool l0);
// B poses and their times into ws.lig_cur / t_dev, the time embedding of each, and the injected graphs (or nullptr) into `tmp`
int upload_batch(dfm_complex *cx, int B, const float *lig_pos, const float *t, const int32_t *edges, DevPool &tmp, int32_t **edges_dev);
int enqueue_forward(dfm_complex *cx, int B, const FwdOpts &o);
// ws.h [B N][256] through the stacked halves [512][256] of a pair head's first Linear -> (ws.A | ws.Bm)
hipError_t project_ab(dfm_complex *cx, int B, const float *wab, const uint16_t *hi = nullptr, const uint16_t *lo = nullptr, bool bf16 = false);
void fill_head_args(dfm_complex *cx, int B, bool want_energy, HeadArgs *a);
// the [B][8] score block (tr 3 | rot 3 | energy | clashes) into the caller's arrays, any of which may be NULL; tr / rot rows `stride` apart
void unpack_scores(const float *sc, int B, float *tr, float *rot, int stride, float *energy, int32_t *num_clashes);
int finish_profile(dfm_complex *cx);
hipError_t launch_sat_count(const uint16_t *x, long long n, unsigned long long *out, hipStream_t s);

}  // namespace dfm
