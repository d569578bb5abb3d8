// api_forward.hip - one batched score evaluation as a schedule of launches on the handle's stream (enqueue_forward and its pieces: graph,
// messages, node model, next projection, heads), the scaffold every public call is built from (begin_call, upload_batch, project_ab,
// fill_head_args, unpack_scores) and the profile read-out.  The host only enqueues; nothing here synchronises but finish_profile.
#include <cstdio>
#include <cstring>
#include <vector>

#include "dfm_device.h"
#include "dfm_engine.h"

using namespace dfm;

// ------------------------------------------------------------------------------------------------
// the scaffold of a public call
int dfm::begin_call(dfm_complex *cx, int B, const EngineSel &sel, bool l0)
{
    int rc = ensure_workspace(cx, B, sel.bf16, l0);
    if (rc) return rc;
    cx->prof = dfm_profile{};
    cx->ev_used = 0; cx->ev_l0_used = 0;
    cx->fwd_counter = 0;   // RNG streams are a pure function of (seed, trajectory, evaluation index): evaluation i draws its graph from Philox stream i
    if (l0) {
        if (!(sel.bf16 ? cx->l0_valid : cx->l0_valid32)) {
            float bms = 0.f;
            if ((rc = build_l0_table(cx, &bms, !sel.bf16)) != DFM_OK) return rc;
            cx->prof.l0_build_ms = bms;
        }
        HIPCHK(hipMemsetAsync(cx->ws.l0_miss_total, 0, sizeof(unsigned long long), cx->stream));
    }
    return DFM_OK;
}

int dfm::upload_batch(dfm_complex *cx, int B, const float *lig_pos, const float *t, const int32_t *edges, DevPool &tmp, int32_t **edges_dev)
{
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    HIPCHK(hipMemcpyAsync(W.lig_cur, lig_pos, (size_t)B * cx->L * 9 * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(W.t_dev, t, (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(launch_time_embed(W.t_dev, B, &cx->m->heads, W.hid_base, s));      // one entry per trajectory (fill_head_args: stride 2 * HI)
    *edges_dev = nullptr;
    if (edges) {
        const size_t n = (size_t)B * cx->N * cx->K;
        HIPCHK(tmp.alloc(edges_dev, n));
        HIPCHK(hipMemcpyAsync(*edges_dev, edges, n * 4, hipMemcpyHostToDevice, s));
    }
    return DFM_OK;
}

hipError_t dfm::project_ab(dfm_complex *cx, int B, const float *wab, const uint16_t *hi, const uint16_t *lo, bool bf16)
{
    Workspace &W = cx->ws;
    GemmArgs g = gemm_args(W.h, H, H, wab, H, nullptr, B * cx->N, 2 * H, W.A, H);
    g.epi = 2; g.C2 = W.Bm;
    return launch_gemm(bf16, g, hi, lo, cx->stream);
}

void dfm::fill_head_args(dfm_complex *cx, int B, bool want_energy, HeadArgs *a)
{
    Workspace &W = cx->ws;
    std::memset(a, 0, sizeof(*a));
    a->fvec = W.fvec; a->ca4 = W.ca4; a->B = B; a->R = cx->R; a->L = cx->L; a->hid_base = W.hid_base; a->hid_bstride = 2 * HI; a->hw = &cx->m->heads;
    a->scores = W.scores; a->want_energy = want_energy; a->en_part = W.en_part; a->clash_part = W.clash_part;
    a->lig_cur = W.lig_cur; a->tr_update = W.tr_update; a->rot_update = W.rot_update;
    const dfm_hparams &hp = cx->m->hp;
    a->all_atoms = hp.family == 1;
    if (hp.family == 1) {
        a->n_part = 4 * ((cx->R + 63) / 64); a->en_mode = hp.agg_mean ? 1 : 2; a->pool_div = hp.agg_mean ? (float)cx->L : 1.0f;
    } else {
        a->n_part = cx->R; a->en_mode = 0; a->pool_div = (float)cx->L;
    }
}

void dfm::unpack_scores(const float *sc, int B, float *tr, float *rot, int stride, float *energy, int32_t *num_clashes)
{
    for (int b = 0; b < B; ++b) {
        const float *row = sc + (size_t)b * 8;
        if (tr) std::memcpy(tr + (size_t)b * stride, row, 3 * sizeof(float));
        if (rot) std::memcpy(rot + (size_t)b * stride, row + 3, 3 * sizeof(float));
        if (energy) energy[b] = row[6];
        if (num_clashes) num_clashes[b] = (int32_t)row[7];
    }
}

// ------------------------------------------------------------------------------------------------
// selfcheck telemetry
// largest |x| of a buffer -> *out (float bits; non-negative floats order like their bit patterns)
__global__ void k_absmax(const float *__restrict__ x, long long n, uint32_t *__restrict__ out)
{
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}
// fp16 values at +-65504 (where every conversion of the 16-bit engine clamps) or beyond
__global__ void k_sat_count(const uint16_t *__restrict__ x, long long n, unsigned long long *__restrict__ out)
{
    unsigned c = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) c += (x[i] & 0x7fffu) >= 0x7bffu;
    for (int k = 32; k >= 1; k >>= 1) c += __shfl_xor(c, k, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}
static hipError_t launch_absmax(const float *x, long long n, uint32_t *out, hipStream_t s)
{
    const long long want = (n + 255) / 256;
    hipLaunchKernelGGL(k_absmax, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), token_lds(), s, x, n, out);
    return hipGetLastError();
}
hipError_t dfm::launch_sat_count(const uint16_t *x, long long n, unsigned long long *out, hipStream_t s)
{
    const long long want = (n + 255) / 256;
    hipLaunchKernelGGL(k_sat_count, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), token_lds(), s, x, n, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// One evaluation in flight: what the pieces of enqueue_forward share
struct Fwd {
    dfm_complex *cx;
    const FwdOpts &o;
    int B, M;                // trajectories, node rows = B * N
    bool pair_family;        // EGNN_Net: pair heads, update_coords = False in every layer
    bool tile_tasks;         // the 16-bit message launches run tile tasks (a ligand-only last layer decides for itself and zeroes agg if it must)
};

// the next n events of a pool that grows on demand (profiled calls only)
static int take_events(std::vector<hipEvent_t> &pool, size_t &used, int n, hipEvent_t *out)
{
    while (used + n > pool.size()) { hipEvent_t a; HIPCHK(hipEventCreate(&a)); pool.push_back(a); }
    for (int k = 0; k < n; ++k) out[k] = pool[used++];
    return DFM_OK;
}

// the graph of an evaluation: pose preparation, kNN + sampled (or injected) edges, edge features and, behind the table, their classification
static int enqueue_graph(const Fwd &f, uint32_t stream_id)
{
    dfm_complex *cx = f.cx;
    const FwdOpts &o = f.o;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const int B = f.B, N = cx->N, R = cx->R, K = cx->K;
    if (!o.pose_prepared) HIPCHK(launch_prep_pose(cx->rec_pos, W.lig_cur, B, R, cx->L, f.pair_family ? 1 : 0, W.pos, W.ca4, W.cb4, s));
    if (o.edges_dev) {
        HIPCHK(hipMemcpy2DAsync(W.edges, (size_t)N * K * 4, o.edges_dev, (size_t)o.edges_pitch * 4, (size_t)N * K * 4, B,
                                hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(launch_knn_sample(W.ca4, B, N, cx->knn, cx->nsamp, o.seed, stream_id, W.edges, o.ctl, s));
    }
    L0Classify cls;
    std::memset(&cls, 0, sizeof(cls));
    if (o.l0_table) { cls.code0 = o.bf16 ? cx->l0_code0 : cx->l0_code0_32; cls.src = W.l0_src; cls.rows = W.l0_rows; cls.counter = W.l0_counter; }
    HIPCHK(launch_edge_feat(W.pos, W.ca4, W.cb4, W.edges, B, N, R, K, cx->m->hp.mask_dist, W.codes, W.radial, cls, o.ctl, s));
    return DFM_OK;
}

// operands of layer l's message kernel
static EdgeArgs layer_edge_args(const Fwd &f, int l, bool lig_only)
{
    dfm_complex *cx = f.cx;
    const FwdOpts &o = f.o;
    Workspace &W = cx->ws;
    const int N = cx->N, depth = cx->m->hp.depth;
    EdgeArgs e;
    std::memset(&e, 0, sizeof(e));
    if (l == 0) { e.A = o.bf16 ? cx->A0s : cx->A0; e.Bm = cx->Bm0; e.Bmb = cx->Bmb0; e.ab_bstride = 0; }
    else { e.A = W.A; e.Bm = W.Bm; e.Bmb = W.Bmb; e.ab_bstride = (int64_t)N * H; }
    const bool aw16 = o.bf16 && !o.f16;      // A_i is read as fp16
    e.Ah = aw16 ? (l == 0 ? cx->A0h : reinterpret_cast<const uint16_t *>(W.A)) : nullptr;
    e.edges = W.edges; e.codes = W.codes; e.radial = W.radial; e.ca4 = W.ca4;
    e.B = f.B; e.N = N; e.R = cx->R; e.K = cx->K; e.lw = &cx->m->layers[l]; e.agg = W.agg;
    e.last = (l == depth - 1) && !f.pair_family; e.fout = W.fvec; e.mbuf = W.mbuf;
    e.f16 = (o.f16 || !o.bf16_ops || l >= depth - 1) ? 1 : 0;
    e.lig_only = lig_only ? 1 : 0;
    e.agg_is_zero = (l > 0 && f.tile_tasks) ? 1 : 0;      // zeroed by the previous layer's node_mlp.3 GEMM
#if defined(DFM_EDGE_STAMP) || defined(DFM_EDGE_TRACE)
    e.stamp = (o.profile && l == 2) ? cx->stamp_dev : nullptr;
#else
    e.stamp = o.profile ? cx->stamp_dev : nullptr;      // every profiled message launch adds its clock stamps
#endif
    e.task_ctr = W.task_ctr;
    return e;
}

// selfcheck telemetry: what enters layer l (h and the operands of e); the fp32 message kernel adds its pre-activations at e.range
static int enqueue_layer_telemetry(const Fwd &f, int l, const float *h, EdgeArgs &e)
{
    const FwdOpts &o = f.o;
    hipStream_t s = f.cx->stream;
    const long long nrow = l == 0 ? f.cx->N : f.M;      // layer 0's operands are per complex, not per trajectory
    if (o.range) {
        uint32_t *rg = o.range + l * 8;
        HIPCHK(launch_absmax(h, nrow * H, rg + 0, s));
        HIPCHK(launch_absmax(e.A, nrow * H, rg + 1, s));
        HIPCHK(launch_absmax(e.Bm, nrow * H, rg + 2, s));
        e.range = rg + 3;
    }
    if (o.sat) {
        if (e.Ah) HIPCHK(launch_sat_count(e.Ah, nrow * H, o.sat, s));
        HIPCHK(launch_sat_count(e.Bmb, nrow * H, o.sat, s));
    }
    return DFM_OK;
}

// the per-edge message kernel, bracketed by HIP events on this stream when profiling (dfm_get_profile)
static int enqueue_message_launch(const Fwd &f, const EdgeArgs &ea)
{
    dfm_complex *cx = f.cx;
    hipStream_t s = cx->stream;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (f.o.profile) {
        const int rc = take_events(cx->ev, cx->ev_used, 2, ev);
        if (rc) return rc;
        if (cx->ev_lig.size() < cx->ev_used / 2) cx->ev_lig.resize(cx->ev_used / 2);
        cx->ev_lig[cx->ev_used / 2 - 1] = ea.lig_only ? 1 : 0;
        HIPCHK(hipEventRecord(ev[0], s));
    }
    HIPCHK(f.o.bf16 ? launch_edge_bf16(ea, s) : launch_edge_f32(ea, s));
    if (f.o.profile) {
        HIPCHK(hipEventRecord(ev[1], s));
        cx->prof.edge_kernel_launches += 1;
        cx->prof.edge_lig_launches += ea.lig_only ? 1 : 0;
        cx->prof.edge_rows += (int64_t)ea.B * (ea.lig_only ? cx->N - cx->R : cx->N) * cx->K;
    }
    return DFM_OK;
}

// layer 0 behind the message table: the edge model over the row list k_edge_feat left (inter-chain edges + bin mismatches), then
// the K-row gather-sum in slot order from the table and that list's messages
static int enqueue_l0_table(const Fwd &f, const EdgeArgs &e)
{
    dfm_complex *cx = f.cx;
    const FwdOpts &o = f.o;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const int B = f.B, N = cx->N, K = cx->K;
    hipEvent_t t[3] = {nullptr, nullptr, nullptr};
    if (o.profile) {
        const int rc = take_events(cx->ev_l0, cx->ev_l0_used, 3, t);
        if (rc) return rc;
        HIPCHK(hipEventRecord(t[0], s));
    }
    if (o.bf16) HIPCHK(launch_edge_rows(e, W.l0_rows, W.l0_counter, (uint32_t)((size_t)B * N * K), W.l0_x, s));
    else HIPCHK(launch_edge_rows32(e, W.l0_rows, W.l0_counter, (uint32_t)((size_t)B * N * K), W.l0_x32, s));
    if (o.profile) HIPCHK(hipEventRecord(t[1], s));
    if (o.bf16) HIPCHK(launch_l0_gather(cx->l0_table, W.l0_x, W.l0_src, W.agg, B, N, K, W.l0_counter, W.l0_miss_total, s));
    else HIPCHK(launch_l0_gather32(cx->l0_table32, W.l0_x32, W.l0_src, W.agg, B, N, K, W.l0_counter, W.l0_miss_total, s));
    if (o.profile) {
        HIPCHK(hipEventRecord(t[2], s));
        cx->prof.l0_evals += 1; cx->prof.l0_edges += (int64_t)B * N * K;
    }
    return DFM_OK;
}

// the message part of layer l: agg = sum of the gated messages of every node's edges (the last layer of Score_Net: also the
// coordinate update of the ligand nodes).  h: the layer's input node features (telemetry only)
// (Running the last layer in trajectory chunks so that the stored messages stay in the Infinity Cache was measured and
// dropped: 15 extra launch pairs per evaluation cost more - weight refills, partial rounds - than the round trip.)
static int enqueue_messages(const Fwd &f, int l, const float *h, bool lig_only)
{
    EdgeArgs e = layer_edge_args(f, l, lig_only);
    int rc = enqueue_layer_telemetry(f, l, h, e);
    if (rc) return rc;
    rc = (l == 0 && f.o.l0_table) ? enqueue_l0_table(f, e) : enqueue_message_launch(f, e);
    if (rc) return rc;
    if (e.last && f.o.bf16) HIPCHK(launch_coord_bf16(e, f.cx->stream));
    return DFM_OK;
}

// node_model of layer l (egnn.py:106-116): u = Linear(cat[h, agg]); GraphNorm; SiLU; Linear; residual -> hn
static int enqueue_node_model(const Fwd &f, int l, const float *h, float *hn)
{
    dfm_complex *cx = f.cx;
    const FwdOpts &o = f.o;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const LayerDev &Lw = cx->m->layers[l];
    const int N = cx->N;
    const bool last = (l == cx->m->hp.depth - 1);
    GemmArgs g = gemm_args(h, H, 2 * H, Lw.W3, 2 * H, Lw.b3, f.M, H, W.u, H);
    g.A1 = W.agg; g.pro = 1; g.a0_period = l == 0 ? N : 0;
    // 16-bit engines: the GEMM leaves per-tile column sums of u behind, so GraphNorm needs no extra pass over u
    const bool fused_stats = o.bf16 && gemm_rows_per_tile() == 64;
    if (fused_stats) { g.stat_part = W.gn_part; g.rows_per_graph = N; }
    HIPCHK(launch_gemm(o.bf16, g, Lw.W3_hi, Lw.W3_lo, s));
    // fused_stats: the statistics are finished in the prologue of the next GEMM (no k_gn_finish launch)
    if (!fused_stats) HIPCHK(launch_gn_stats(W.u, f.B, N, Lw.gn_ms, W.gn_shift, W.gn_den, o.bf16 ? Lw.gn_w : nullptr, o.bf16 ? Lw.gn_b : nullptr, s));
    g = gemm_args(W.u, H, H, Lw.W4, H, Lw.b4, f.M, H, hn, H);
    g.pro = 2; g.gn_shift = W.gn_shift; g.gn_den = W.gn_den; g.gn_w = Lw.gn_w; g.gn_b = Lw.gn_b; g.rows_per_graph = N;
    if (fused_stats) { g.gn_part = W.gn_part; g.gn_ms = Lw.gn_ms; }
    // tile-task message launches add into a zero agg: its last reader (node_mlp.0) is done, this launch leaves it zeroed for the next layer
    if (o.bf16 && !last && f.tile_tasks) g.zbuf = W.agg;
    g.epi = 1; g.R = h; g.r_period = l == 0 ? N : 0;
    HIPCHK(launch_gemm(o.bf16, g, Lw.W4_hi, Lw.W4_lo, s));
    return DFM_OK;
}

// layer l's per-node halves of edge_mlp.0 from the features h the previous layer left: A = Wa h + b1, Bm = Wb h
static int enqueue_next_ab(const Fwd &f, int l, const float *h)
{
    dfm_complex *cx = f.cx;
    const FwdOpts &o = f.o;
    Workspace &W = cx->ws;
    const LayerDev &Ln = cx->m->layers[l];
    const float *bias = cx->homomer ? (o.bf16 ? Ln.bias_ab_h_s : Ln.bias_ab_h) : (o.bf16 ? Ln.bias_ab_s : Ln.bias_ab);
    GemmArgs g = gemm_args(h, H, H, Ln.Wab, H, bias, f.M, 2 * H, W.A, H);
    g.epi = 2; g.C2 = o.bf16 ? nullptr : W.Bm; g.C2b = W.Bmb;            // 16-bit engines gather the fp16 copy only
    if (o.bf16 && !o.f16) g.Cb = reinterpret_cast<uint16_t *>(W.A);     // ... and, A_i read as fp16, A as fp16 too (same buffer)
    HIPCHK(launch_gemm(o.bf16, g, Ln.Wab_hi, Ln.Wab_lo, cx->stream));
    return DFM_OK;
}

// one pair head of family 1: the projection of every node, then the elementwise pair kernel in `mode`
static int enqueue_pair_head(const Fwd &f, int q, int mode)
{
    dfm_complex *cx = f.cx;
    const dfm_model *m = cx->m;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const int R = cx->R;
    const PairHeadDev &Ph = m->pair[q];
    HIPCHK(project_ab(cx, f.B, Ph.wab, Ph.wab_hi, Ph.wab_lo, f.o.bf16));
    PairArgs a;
    std::memset(&a, 0, sizeof(a));
    a.P = W.A; a.Q = W.Bm; a.ca4 = W.ca4; a.B = f.B; a.R = R; a.L = cx->L; a.w_d = Ph.w_d; a.ln_w = Ph.ln_w; a.ln_b = Ph.ln_b;
    a.w3 = Ph.w3; a.mode = mode; a.cut_off = m->hp.cut_off; a.fpart = W.fpart;
    a.spart = mode == 1 ? W.en_part : W.cpart; a.clash_part = W.clash_part;
    if (f.o.bf16) {      // 16-bit engines: s(r, l) with the rank-4 part on the matrix pipe, then this head's reductions
        a.S = W.pair_s; a.Rp = (R + 31) / 32 * 32;
        HIPCHK(launch_pair_head_m(a, s));
        HIPCHK(launch_pair_finish_s(a, 4 * ((R + 63) / 64), m->hp.agg_mean ? 1.0f / (float)R : 1.0f, W.fvec, W.conf, s));
        return DFM_OK;
    }
    HIPCHK(launch_pair_head(a, s));
    return DFM_OK;
}

// egnn_net.py:430-470: pair heads on cat[h_r, h_l, D].  Per head: one GEMM projects every node through the stacked
// halves of Linear(513 -> 256) (reusing the A / Bm buffers), then the elementwise pair kernel.
// 16-bit engines: k_pair_head_m (LayerNorm statistics from fp32 row moments + a dot product, 1-ulp hardware exp2 / rcp).
// The fp32 engine - the baseline of dfm_complex_selfcheck and the fallback when a check fails - keeps the three-pass
// LayerNorm, expf and IEEE division of k_pair_head: z = P + Q + w_d * D with D up to hundreds of Angstroms, so
// E[z^2] - mean^2 loses digits to cancellation exactly when a trained checkpoint has a large mean / std ratio, which no
// synthetic draw shows.
static int enqueue_pair_heads(const Fwd &f)
{
    dfm_complex *cx = f.cx;
    const dfm_model *m = cx->m;
    Workspace &W = cx->ws;
    int rc = enqueue_pair_head(f, 0, 0);
    if (rc) return rc;
    if (f.o.want_energy) {
        if ((rc = enqueue_pair_head(f, 1, 1)) != DFM_OK) return rc;
        if ((rc = enqueue_pair_head(f, 2, 2)) != DFM_OK) return rc;
    }
    if (!f.o.bf16)
        HIPCHK(launch_pair_finish(W.fpart, f.B, cx->R, cx->L, m->hp.agg_mean ? 1.0f / (float)cx->R : 1.0f, W.fvec, W.cpart,
                                  f.o.want_energy ? W.conf : nullptr, cx->stream));
    return DFM_OK;
}

// to_energy.0 of Score_Net on cat[h_r, h_l] = Wa h_r + Wb h_l: project every node once (reuses A / Bm buffers), then the pair sums
static int enqueue_energy_head(const Fwd &f)
{
    dfm_complex *cx = f.cx;
    const dfm_model *m = cx->m;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    GemmArgs g = gemm_args(W.h, H, H, m->heads.en_wa, 2 * H, nullptr, f.M, H, W.A, H);
    HIPCHK(launch_gemm_f32(g, s));
    g.W = m->heads.en_wb; g.C = W.Bm;
    HIPCHK(launch_gemm_f32(g, s));
    HIPCHK(launch_energy_pairs(W.A, W.Bm, W.ca4, f.B, cx->R, cx->L, m->hp.cut_off, &m->heads, 1, W.en_part, W.clash_part, s));
    return DFM_OK;
}

// One batched score evaluation of the poses in ws.lig_cur at times ws.t_dev; leaves f in ws.fvec, the
// node features in ws.h and (optionally) the energy partials.  Everything is enqueued on cx->stream.
int dfm::enqueue_forward(dfm_complex *cx, int B, const FwdOpts &o)
{
    const dfm_model *m = cx->m;
    Workspace &W = cx->ws;
    hipStream_t s = cx->stream;
    const int depth = m->hp.depth;
    const Fwd f{cx, o, B, B * cx->N, m->hp.family == 1, o.bf16 && edge_msg_tile_tasks(B, cx->N, cx->K)};
    int rc = enqueue_graph(f, cx->fwd_counter++);
    if (rc) return rc;
    // layer 0 reads the node embedding h0 [N][256] of the complex itself - identical for every trajectory - through a row period
    // (GemmArgs::a0_period / r_period) instead of a [B][N][256] copy made per evaluation (r01-r03: k_bcast_rows, 157 MB of writes at C3)
    const float *h = cx->h0;
    float *hn = W.h, *hspare = W.h2;
    for (int l = 0; l < depth; ++l) {
        const bool last = (l == depth - 1);
        // Score_Net reads the last layer's node outputs only in its energy / ires heads (score_net_mlsb.py:383-390); the force comes
        // from pos_out of the LIGAND nodes (:396-398), i.e. from the last layer's messages of ligand nodes alone
        const bool lig_only = last && !f.pair_family && !o.need_node_out;
        if ((rc = enqueue_messages(f, l, h, lig_only)) != DFM_OK) return rc;
        if (lig_only) break;      // the node model of the last layer feeds heads nobody asked for
        if ((rc = enqueue_node_model(f, l, h, hn)) != DFM_OK) return rc;
        { float *done = hn; hn = (l == 0) ? hspare : const_cast<float *>(h); h = done; }
        if (l == 0 && o.h_first_out)
            HIPCHK(hipMemcpyAsync(o.h_first_out, h, (size_t)f.M * H * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (!last && (rc = enqueue_next_ab(f, l + 1, h)) != DFM_OK) return rc;
    }
    // keep the final node features in W.h (depth even).  The pair heads of family 1 read W.h on EVERY evaluation, the heads of
    // family 0 only when somebody asked for the node outputs
    if (o.range && (o.need_node_out || f.pair_family)) HIPCHK(launch_absmax(h, (long long)f.M * H, o.range + depth * 8, s));
    if (h != W.h && (o.need_node_out || f.pair_family))
        HIPCHK(hipMemcpyAsync(W.h, h, (size_t)f.M * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (f.pair_family) return enqueue_pair_heads(f);
    if (o.want_energy) return enqueue_energy_head(f);
    return DFM_OK;
}

// ------------------------------------------------------------------------------------------------
int dfm::finish_profile(dfm_complex *cx)
{
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, cx->ev_total[0], cx->ev_total[1]));
    cx->prof.total_ms = ms;
    for (size_t i = 0; i + 1 < cx->ev_used; i += 2) {
        HIPCHK(hipEventElapsedTime(&ms, cx->ev[i], cx->ev[i + 1]));
        cx->prof.edge_kernel_ms += ms;
        if (i / 2 < cx->ev_lig.size() && cx->ev_lig[i / 2]) cx->prof.edge_lig_ms += ms;
    }
    for (size_t i = 0; i + 2 < cx->ev_l0_used; i += 3) {
        HIPCHK(hipEventElapsedTime(&ms, cx->ev_l0[i], cx->ev_l0[i + 1]));
        cx->prof.l0_rows_ms += ms;
        HIPCHK(hipEventElapsedTime(&ms, cx->ev_l0[i + 1], cx->ev_l0[i + 2]));
        cx->prof.l0_gather_ms += ms;
    }
    if (cx->prof.l0_evals > 0 && cx->ws.l0_miss_total) {
        unsigned long long tot = 0;
        HIPCHK(hipMemcpyAsync(&tot, cx->ws.l0_miss_total, sizeof(tot), hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        cx->prof.l0_miss_rows = (int64_t)tot;
    }
#if !defined(DFM_EDGE_STAMP) && !defined(DFM_EDGE_TRACE)
    if (cx->stamp_dev && cx->ev_used) {      // the clock stamps of this call's message launches (k_edge_msg), then back to zero for the next call
        unsigned long long st[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(st, cx->stamp_dev, sizeof(st), hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipMemsetAsync(cx->stamp_dev, 0, 2 * 8, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        cx->prof.edge_shader_cycles = (double)st[0];
        cx->prof.edge_ref_ticks = (double)st[1];
    }
#endif
#ifdef DFM_EDGE_TRACE      // diagnostic build: raw wave timelines of workgroup 0 -> $DFM_EDGE_TRACE_FILE (tools/edge_trace.py)
    if (cx->stamp_dev && getenv("DFM_EDGE_TRACE_FILE")) {
        static unsigned long long tr[48 + 8 * 130];      // [0..15]: s_memrealtime of every wave at its tiles 0 and 63; [48..]: the timelines
        HIPCHK(hipMemcpyAsync(tr, cx->stamp_dev, sizeof(tr), hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        if (FILE *f = fopen(getenv("DFM_EDGE_TRACE_FILE"), "wb")) { fwrite(tr, 1, sizeof(tr), f); fclose(f); }
    }
#endif
#ifdef DFM_EDGE_STAMP
    if (cx->stamp_dev) {
        unsigned long long st[48];
        HIPCHK(hipMemcpyAsync(st, cx->stamp_dev, sizeof(st), hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        for (int k = 0; k < 16; ++k) cx->prof.slot_cycles[k] = (double)st[32 + k];
        const double tiles = (double)cx->prof.edge_rows / (double)cx->prof.edge_kernel_launches / 32.0 / 2048.0;   // per wave
        for (int k = 0; k < 4; ++k) {
            double s2 = 0;
            for (int w = 0; w < 8; ++w) s2 += (double)st[w * 4 + k];
            cx->prof.phase_cycles[k] = s2 / 8.0 / (tiles > 0 ? tiles : 1.0);
        }
    }
#endif
    return DFM_OK;
}

extern "C" int dfm_get_profile(const dfm_complex *cx, dfm_profile *p)
{
    if (!cx || !p) return fail(DFM_E_INVALID, "NULL argument");
    *p = cx->prof;
    return DFM_OK;
}
