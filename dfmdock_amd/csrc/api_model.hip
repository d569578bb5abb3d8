// api_model.hip - the model handle: the map of the weight blob (state_dict order), the packers that put every weight into the layout
// its kernel reads, dfm_model_create / dfm_model_destroy.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dfm_device.h"
#include "dfm_engine.h"

using namespace dfm;

struct BlobMap {
    const float *single_embed, *spatial_embed, *positional_embed;
    struct Lw {
        const float *e1_w, *e1_b, *e2_w, *e2_b, *n1_w, *n1_b, *gn_w, *gn_b, *gn_ms, *n2_w, *n2_b, *c1_w, *c1_b, *c2_w,
            *att_w, *att_b;
    } layer[8];
    const float *en0_w, *en_ln_w, *en_ln_b, *en3_w;
    struct Ph { const float *w0, *ln_w, *ln_b, *w3; } pair[3], dist;   // family 1: to_force, to_energy, to_confidence; to_dist (w3 is [64][256])
    const float *ir0_w, *ir0_b, *ir2_w, *ir2_b, *ir4_w, *ir4_b;   // to_ires
    const float *t_W, *t_lin, *trs0, *trs_ln_w, *trs_ln_b, *trs4, *rots0, *rots_ln_w, *rots_ln_b, *rots4;
    int64_t total;
};

static void map_blob(const dfm_hparams *hp, const float *blob, BlobMap *w)
{   // state_dict order of Score_Net (score_net_mlsb.py:249-341, egnn.py:37-93) or, family 1, of EGNN_Net
    // (egnn_net.py:296-385); see dfmdock_amd/weights.py
    const int64_t Hh = hp->node_dim, He = hp->edge_dim, Hi = hp->inner_dim;
    const float *p = blob;
    auto take = [&](const float *&dst, int64_t n) { dst = p; p += n; };
    take(w->single_embed, Hh * hp->lm_embed_dim);
    take(w->spatial_embed, He * hp->spatial_embed_dim);
    take(w->positional_embed, He * hp->positional_embed_dim);
    for (int l = 0; l < hp->depth; ++l) {
        auto &Lw = w->layer[l];
        take(Lw.e1_w, Hh * (2 * Hh + 1 + He)); take(Lw.e1_b, Hh);
        take(Lw.e2_w, Hh * Hh); take(Lw.e2_b, Hh);
        take(Lw.n1_w, Hh * 2 * Hh); take(Lw.n1_b, Hh);
        take(Lw.gn_w, Hh); take(Lw.gn_b, Hh); take(Lw.gn_ms, Hh);
        take(Lw.n2_w, Hh * Hh); take(Lw.n2_b, Hh);
        if (l == hp->depth - 1 && hp->family == 0) { take(Lw.c1_w, Hh * Hh); take(Lw.c1_b, Hh); take(Lw.c2_w, Hh); }
        else Lw.c1_w = Lw.c1_b = Lw.c2_w = nullptr;
        take(Lw.att_w, Hh); take(Lw.att_b, 1);
    }
    if (hp->family == 1) {   // to_energy, to_force, to_dist, to_confidence on cat[h_r, h_l, D]
        auto head = [&](BlobMap::Ph &h) { take(h.w0, Hh * (2 * Hh + 1)); take(h.ln_w, Hh); take(h.ln_b, Hh); take(h.w3, Hh); };
        head(w->pair[1]); head(w->pair[0]);
        take(w->dist.w0, Hh * (2 * Hh + 1)); take(w->dist.ln_w, Hh); take(w->dist.ln_b, Hh); take(w->dist.w3, 64 * Hh);
        head(w->pair[2]);
        w->en0_w = w->en_ln_w = w->en_ln_b = w->en3_w = nullptr;
    } else {
        take(w->en0_w, Hh * 2 * Hh); take(w->en_ln_w, Hh); take(w->en_ln_b, Hh); take(w->en3_w, Hh);
        for (auto &h : w->pair) h.w0 = h.ln_w = h.ln_b = h.w3 = nullptr;
        w->dist.w0 = w->dist.ln_w = w->dist.ln_b = w->dist.w3 = nullptr;
    }
    take(w->ir0_w, 2 * Hh * Hh); take(w->ir0_b, 2 * Hh); take(w->ir2_w, 4 * Hh * Hh); take(w->ir2_b, 2 * Hh);   // to_ires.{0,2}
    take(w->ir4_w, 2 * Hh); take(w->ir4_b, 1);                                                                  // to_ires.4
    take(w->t_W, Hi / 2); take(w->t_lin, Hi * Hi);
    take(w->trs0, Hi * (Hi + 1)); take(w->trs_ln_w, Hi); take(w->trs_ln_b, Hi); take(w->trs4, Hi);
    take(w->rots0, Hi * (Hi + 1)); take(w->rots_ln_w, Hi); take(w->rots_ln_b, Hi); take(w->rots4, Hi);
    w->total = (int64_t)(p - blob);
}

int64_t dfm::blob_floats(const dfm_hparams *hp)
{
    BlobMap w;
    map_blob(hp, nullptr, &w);
    return w.total;
}

// ------------------------------------------------------------------------------------------------
static std::vector<uint16_t> pack_frags(const float *W /*[256 out][256 in]*/, bool f16 = false)
{   // 16-bit B-operand fragments of v_mfma_f32_32x32x16_bf16: [kk][nt][lane][e] = W[nt*32 + lane%32][chan(kk, lane/32, e)]
    std::vector<uint16_t> f((size_t)16 * 8 * 64 * 8);
    for (int kk = 0; kk < 16; ++kk)
        for (int nt = 0; nt < 8; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int n = nt * 32 + (lane & 31), k = frag_channel(kk, lane >> 5, e);
                    f[(((size_t)kk * 8 + nt) * 64 + lane) * 8 + e] = f16 ? f2h(W[(size_t)n * H + k]) : f2bf(W[(size_t)n * H + k]);
                }
    return f;
}
// split-bf16 operands of k_gemm_split, tiled in K-stage order: [K/32][4 k-groups][Nout][8] (W is [Nout][K] row-major)
static void split_bf16(const float *W, int Nout, int K, std::vector<uint16_t> &hi, std::vector<uint16_t> &lo)
{
    hi.resize((size_t)Nout * K); lo.resize((size_t)Nout * K);
    for (int o = 0; o < Nout; ++o)
        for (int k = 0; k < K; ++k) {
            const float w = W[(size_t)o * K + k];
            const size_t d = (((size_t)(k / 32) * 4 + (k % 32) / 8) * Nout + o) * 8 + (k % 8);
            hi[d] = f2bf(w);
            lo[d] = f2bf(w - bf2f(hi[d]));
        }
}
// SILU_S * bias as packed (hi | lo << 16) 16-bit pairs: the B operand of the bias k-step of the MFMA edge kernels
static std::vector<uint32_t> pack_bias(const float *bias, bool f16)
{
    std::vector<uint32_t> v(2 * H, 0u);      // [8 n-tiles][64 lanes]: lanes 0..31 = columns, lanes 32..63 = 0 (k >= 8)
    for (int c = 0; c < H; ++c) {
        const float x = SILU_S * bias[c];
        uint16_t hi, lo;
        if (f16) { hi = f2h(x); lo = f2h(x - h2f(hi)); }
        else { hi = f2bf(x); lo = f2bf(x - bf2f(hi)); }
        v[(c / 32) * 64 + (c % 32)] = (uint32_t)hi | ((uint32_t)lo << 16);
    }
    return v;
}
static std::vector<float> transpose256(const float *W)
{
    std::vector<float> t((size_t)H * H);
    for (int o = 0; o < H; ++o)
        for (int k = 0; k < H; ++k) t[(size_t)k * H + o] = W[(size_t)o * H + k];
    return t;
}

// the argument checks of dfm_model_create, the blob's map and the empty handle on the current device
static dfm_model *new_model(const float *blob, size_t n_floats, const dfm_hparams *hp, BlobMap &w)
{
    if (!blob || !hp) { fail(DFM_E_INVALID, "blob or hp is NULL"); return nullptr; }
    if (hp->node_dim != H || hp->edge_dim != HE || hp->inner_dim != HI || hp->spatial_embed_dim != 100 ||
        (hp->positional_embed_dim != 66 && hp->positional_embed_dim != 67) || hp->depth < 1 || hp->depth > 8 || hp->knn < 1 || hp->n_sample < 0 ||
        hp->knn + hp->n_sample > 60 || hp->lm_embed_dim < 1 || hp->family < 0 || hp->family > 1) {
        fail(DFM_E_INVALID, "unsupported hyper-parameters (kernels are built for node 256 / edge 128 / inner 128, degree <= 60)");
        return nullptr;
    }
    map_blob(hp, blob, &w);
    if ((int64_t)n_floats != w.total) {
        fail(DFM_E_INVALID, "blob has " + std::to_string(n_floats) + " floats, expected " + std::to_string(w.total));
        return nullptr;
    }
    dfm_model *m = new dfm_model();
    m->hp = *hp;
    if (hipGetDevice(&m->device) != hipSuccess) { fail(DFM_E_NODEVICE, "no current HIP device"); delete m; return nullptr; }
    return m;
}

// uploads into the model's pool; the first failure sticks
struct Uploader {
    DevPool &P;
    bool ok = true;
    void f32(float **dst, const float *src, size_t n) { ok = ok && P.upload(dst, src, n) == hipSuccess; }
    void u16(uint16_t **dst, const std::vector<uint16_t> &v) { ok = ok && P.upload(dst, v.data(), v.size()) == hipSuccess; }
    void u32(uint32_t **dst, const std::vector<uint32_t> &v) { ok = ok && P.upload(dst, v.data(), v.size()) == hipSuccess; }
};

// the node embedding and, per layer, every operand of its message kernel and node-model GEMMs in the layout the kernel reads
static void pack_layers(dfm_model *m, const BlobMap &w, Uploader &U)
{
    const dfm_hparams *hp = &m->hp;
    const int Pd = hp->positional_embed_dim;
    const int Kin1 = 2 * H + 1 + HE;
    U.f32(&m->single_embed, w.single_embed, (size_t)H * hp->lm_embed_dim);
    for (int l = 0; l < hp->depth && U.ok; ++l) {
        const auto &Lw = w.layer[l];
        LayerDev &D = m->layers[l];
        std::memset(&D, 0, sizeof(D));
        std::vector<float> Wab((size_t)2 * H * H), bias_ab(2 * H, 0.f), w_r(H);
        for (int c = 0; c < H; ++c) {
            std::memcpy(&Wab[(size_t)c * H], Lw.e1_w + (size_t)c * Kin1, H * sizeof(float));
            std::memcpy(&Wab[(size_t)(H + c) * H], Lw.e1_w + (size_t)c * Kin1 + H, H * sizeof(float));
            bias_ab[c] = Lw.e1_b[c];
            w_r[c] = Lw.e1_w[(size_t)c * Kin1 + 2 * H];
        }
        // T[idx][c] = sum_k We[c][k] * SP[k][idx]  (one_hot @ spatial/positional_embed^T then We: a row gather)
        std::vector<double> Td((size_t)NTAB * H);
        std::vector<float> T((size_t)NTAB * H);
        for (int idx = 0; idx < NTAB; ++idx)
            for (int c = 0; c < H; ++c) {
                double s = 0;
                for (int k = 0; k < HE; ++k) {
                    const float sp = idx < 100 ? w.spatial_embed[(size_t)k * 100 + idx]
                                               : w.positional_embed[(size_t)k * Pd + (idx - 100)];
                    s += (double)Lw.e1_w[(size_t)c * Kin1 + 2 * H + 1 + k] * sp;
                }
                Td[(size_t)idx * H + c] = s;
                T[(size_t)idx * H + c] = (float)s;
            }
        // merged fp16 tables of the 16-bit MFMA kernel, pre-multiplied by SILU_S like every other SiLU input there
        const double S = (double)SILU_S;
        std::vector<uint16_t> T2b((size_t)NTAB2 * H);
        double tmax[2] = {0, 0};      // range telemetry of dfm_complex_selfcheck
        for (int om = 0; om < 24; ++om)
            for (int th = 0; th < 24; ++th)
                for (int ph = 0; ph < 12; ++ph) {
                    uint16_t *row = &T2b[(size_t)((om * 24 + th) * 12 + ph) * H];
                    const double *a = &Td[(size_t)(40 + om) * H], *b = &Td[(size_t)(64 + th) * H], *c3 = &Td[(size_t)(88 + ph) * H];
                    for (int c = 0; c < H; ++c) { const double v = S * (a[c] + b[c] + c3[c]); tmax[0] = std::fmax(tmax[0], std::fabs(v)); row[c] = f2h((float)v); }
                }
        for (int rp = 0; rp < 66; ++rp)
            for (int d = 0; d < 40; ++d) {
                uint16_t *row = &T2b[(size_t)(6912 + rp * 40 + d) * H];
                const double *a = &Td[(size_t)(100 + rp) * H], *b = &Td[(size_t)d * H];
                for (int c = 0; c < H; ++c) { const double v = S * (a[c] + b[c]); tmax[1] = std::fmax(tmax[1], std::fabs(v)); row[c] = f2h((float)v); }
            }
        m->tab_max[l][0] = (float)tmax[0]; m->tab_max[l][1] = (float)tmax[1];
        {
            std::vector<float> wrs(H), babs(2 * H), wc2s(H);
            for (int c = 0; c < H; ++c) wrs[c] = SILU_S * w_r[c];
            for (int c = 0; c < 2 * H; ++c) babs[c] = SILU_S * bias_ab[c];
            U.f32(&D.w_r_s, wrs.data(), H); U.f32(&D.bias_ab_s, babs.data(), 2 * H);
            U.u32(&D.b2p, pack_bias(Lw.e2_b, false)); U.u32(&D.b2p16, pack_bias(Lw.e2_b, true));
            if (Lw.c1_w) {
                for (int c = 0; c < H; ++c) wc2s[c] = Lw.c2_w[c] / SILU_S;
                U.f32(&D.wc2_s, wc2s.data(), H);
                U.u32(&D.bc1p, pack_bias(Lw.c1_b, false)); U.u32(&D.bc1p16, pack_bias(Lw.c1_b, true));
            }
        }
        if (Pd == 67) {   // "sym" channel: one_hot-free constant column of the position matrix -> We . P[:, 66] on every edge
            std::vector<float> bh(bias_ab), bhs(2 * H);
            for (int c = 0; c < H; ++c) {
                double s2 = 0;
                for (int k = 0; k < HE; ++k) s2 += (double)Lw.e1_w[(size_t)c * Kin1 + 2 * H + 1 + k] * w.positional_embed[(size_t)k * Pd + 66];
                bh[c] = (float)((double)bias_ab[c] + s2);
            }
            for (int c = 0; c < 2 * H; ++c) bhs[c] = SILU_S * bh[c];
            U.f32(&D.bias_ab_h, bh.data(), 2 * H); U.f32(&D.bias_ab_h_s, bhs.data(), 2 * H);
        }
        U.f32(&D.Wab, Wab.data(), Wab.size()); U.f32(&D.bias_ab, bias_ab.data(), bias_ab.size());
        U.f32(&D.w_r, w_r.data(), w_r.size()); U.f32(&D.T, T.data(), T.size()); U.u16(&D.T2b, T2b);
        const std::vector<float> W2t = transpose256(Lw.e2_w);
        U.f32(&D.W2t, W2t.data(), W2t.size()); U.u16(&D.W2f, pack_frags(Lw.e2_w)); U.u16(&D.W2f16, pack_frags(Lw.e2_w, true));
        U.f32(&D.b2, Lw.e2_b, H); U.f32(&D.att_w, Lw.att_w, H); D.att_b = Lw.att_b[0];
        U.f32(&D.W3, Lw.n1_w, (size_t)H * 2 * H); U.f32(&D.b3, Lw.n1_b, H);
        U.f32(&D.gn_w, Lw.gn_w, H); U.f32(&D.gn_b, Lw.gn_b, H); U.f32(&D.gn_ms, Lw.gn_ms, H);
        U.f32(&D.W4, Lw.n2_w, (size_t)H * H); U.f32(&D.b4, Lw.n2_b, H);
        {
            std::vector<uint16_t> hi, lo;
            std::vector<float> Wabs(Wab.size());      // [Wa|Wb] of the 16-bit engine: scaled by SILU_S (A, Bm feed a SiLU)
            for (size_t q = 0; q < Wab.size(); ++q) Wabs[q] = SILU_S * Wab[q];
            split_bf16(Wabs.data(), 2 * H, H, hi, lo); U.u16(&D.Wab_hi, hi); U.u16(&D.Wab_lo, lo);
            split_bf16(Lw.n1_w, H, 2 * H, hi, lo); U.u16(&D.W3_hi, hi); U.u16(&D.W3_lo, lo);
            split_bf16(Lw.n2_w, H, H, hi, lo); U.u16(&D.W4_hi, hi); U.u16(&D.W4_lo, lo);
        }
        if (Lw.c1_w) {
            const std::vector<float> Wc1t = transpose256(Lw.c1_w);
            U.f32(&D.Wc1t, Wc1t.data(), Wc1t.size()); U.u16(&D.Wc1f, pack_frags(Lw.c1_w)); U.u16(&D.Wc1f16, pack_frags(Lw.c1_w, true));
            U.f32(&D.bc1, Lw.c1_b, H); U.f32(&D.wc2, Lw.c2_w, H);
        }
    }
}

// the heads: pair heads and to_dist (family 1) or to_energy (family 0), to_ires, the time embedding and the score-scale MLPs
static void pack_heads(dfm_model *m, const BlobMap &w, Uploader &U)
{
    const dfm_hparams *hp = &m->hp;
    HeadsDev &Hd = m->heads;
    std::memset(&Hd, 0, sizeof(Hd));
    std::memset(m->pair, 0, sizeof(m->pair));
    if (hp->family == 1) {
        const int Kp = 2 * H + 1;
        for (int q = 0; q < 3 && U.ok; ++q) {
            const auto &src = w.pair[q];
            std::vector<float> wab((size_t)2 * H * H), wd(H);
            for (int c = 0; c < H; ++c) {      // rows 0..255: receptor half W[:, :256]; rows 256..511: ligand half W[:, 256:512]
                std::memcpy(&wab[(size_t)c * H], src.w0 + (size_t)c * Kp, H * sizeof(float));
                std::memcpy(&wab[(size_t)(H + c) * H], src.w0 + (size_t)c * Kp + H, H * sizeof(float));
                wd[c] = src.w0[(size_t)c * Kp + 2 * H];
            }
            PairHeadDev &D = m->pair[q];
            std::vector<uint16_t> hi, lo;
            U.f32(&D.wab, wab.data(), wab.size());
            split_bf16(wab.data(), 2 * H, H, hi, lo); U.u16(&D.wab_hi, hi); U.u16(&D.wab_lo, lo);
            U.f32(&D.w_d, wd.data(), H); U.f32(&D.ln_w, src.ln_w, H); U.f32(&D.ln_b, src.ln_b, H); U.f32(&D.w3, src.w3, H);
        }
        if (U.ok) {      // to_dist: fp32 projection only (evaluated on request, DFM_F_DIST), Linear(256 -> 64) stored transposed
            const auto &src = w.dist;
            std::vector<float> wab((size_t)2 * H * H), wd(H), w3t((size_t)H * 64);
            for (int c = 0; c < H; ++c) {
                std::memcpy(&wab[(size_t)c * H], src.w0 + (size_t)c * Kp, H * sizeof(float));
                std::memcpy(&wab[(size_t)(H + c) * H], src.w0 + (size_t)c * Kp + H, H * sizeof(float));
                wd[c] = src.w0[(size_t)c * Kp + 2 * H];
                for (int o = 0; o < 64; ++o) w3t[(size_t)c * 64 + o] = src.w3[(size_t)o * H + c];
            }
            PairHeadDev &D = m->dist;
            std::memset(&D, 0, sizeof(D));
            U.f32(&D.wab, wab.data(), wab.size()); U.f32(&D.w_d, wd.data(), H); U.f32(&D.ln_w, src.ln_w, H); U.f32(&D.ln_b, src.ln_b, H);
            U.f32(&D.w3, w3t.data(), w3t.size());
            std::vector<float> w3f((size_t)64 * H);      // A operands of the 256 -> 64 projection: [out block][channel quad][out row][4]
            for (int ob = 0; ob < 2; ++ob)
                for (int c4 = 0; c4 < H / 4; ++c4)
                    for (int mrow = 0; mrow < 32; ++mrow)
                        for (int e = 0; e < 4; ++e)
                            w3f[(((size_t)ob * (H / 4) + c4) * 32 + mrow) * 4 + e] = src.w3[(size_t)(ob * 32 + mrow) * H + c4 * 4 + e] * (1.0f / SILU_S);
            U.f32(&m->dist_w3f, w3f.data(), w3f.size());
        }
    } else {
        U.f32(&m->en0_w, w.en0_w, (size_t)H * 2 * H);
        Hd.en_wa = m->en0_w; Hd.en_wb = m->en0_w ? m->en0_w + H : nullptr;
        U.f32(&Hd.en_ln_w, w.en_ln_w, H); U.f32(&Hd.en_ln_b, w.en_ln_b, H); U.f32(&Hd.en_w3, w.en3_w, H);
    }
    U.f32(&m->ir0_w, w.ir0_w, (size_t)2 * H * H); U.f32(&m->ir0_b, w.ir0_b, 2 * H); U.f32(&m->ir2_w, w.ir2_w, (size_t)4 * H * H);
    U.f32(&m->ir2_b, w.ir2_b, 2 * H); U.f32(&m->ir4_w, w.ir4_w, 2 * H); U.f32(&m->ir4_b, w.ir4_b, 1);
    U.f32(&Hd.t_W, w.t_W, HI / 2); U.f32(&Hd.t_lin, w.t_lin, (size_t)HI * HI);
    U.f32(&Hd.trs0, w.trs0, (size_t)HI * (HI + 1)); U.f32(&Hd.trs_ln_w, w.trs_ln_w, HI); U.f32(&Hd.trs_ln_b, w.trs_ln_b, HI);
    U.f32(&Hd.trs4, w.trs4, HI);
    U.f32(&Hd.rots0, w.rots0, (size_t)HI * (HI + 1)); U.f32(&Hd.rots_ln_w, w.rots_ln_w, HI); U.f32(&Hd.rots_ln_b, w.rots_ln_b, HI);
    U.f32(&Hd.rots4, w.rots4, HI);
}

extern "C" dfm_model *dfm_model_create(const float *blob, size_t n_floats, const dfm_hparams *hp)
{
    BlobMap w;
    dfm_model *m = new_model(blob, n_floats, hp, w);
    if (!m) return nullptr;
    Uploader U{m->pool};
    pack_layers(m, w, U);
    pack_heads(m, w, U);
    if (!U.ok) {
        fail(DFM_E_HIP, std::string("weight upload failed: ") + hipGetErrorString(hipGetLastError()));
        delete m;
        return nullptr;
    }
    return m;
}

extern "C" void dfm_model_destroy(dfm_model *m)
{
    if (!m) return;
    DeviceScope ds(m->device);
    delete m;
}
