// api.hip - C ABI of the engine (include/dfmdock_amd.h): what belongs to no handle - the thread's last error, the block cache and the
// allocator diagnostics, the device calls, the hyper-parameters, the diffusion coefficients and the configuration string.  The
// handles and the calls on them are in the other api_*.hip files (dfm_engine.h lists them); what every file needs is in dfm_host.h.
#include <cstring>
#include <string>

#include "dfm_engine.h"

using namespace dfm;

// ------------------------------------------------------------------------------------------------
// the single definitions of what dfm_host.h declares
thread_local std::string dfm::g_err;
extern "C" const char *dfm_last_error(void) { return g_err.c_str(); }
BlockCache &dfm::g_block_cache = *new BlockCache;
AllocDiag dfm::g_alloc_diag;

// ------------------------------------------------------------------------------------------------
extern "C" void dfm_default_hparams(dfm_hparams *hp)
{
    hp->lm_embed_dim = 1301; hp->positional_embed_dim = 66; hp->spatial_embed_dim = 100;
    hp->node_dim = 256; hp->edge_dim = 128; hp->inner_dim = 128; hp->depth = 6; hp->knn = 20; hp->n_sample = 40;
    hp->cut_off = 20.0f; hp->mask_dist = 22.0f;
    hp->r3_min_sigma = 0.1; hp->r3_max_sigma = 30.0; hp->so3_min_sigma = 0.1; hp->so3_max_sigma = 1.5;
    hp->family = 0; hp->agg_mean = 1;
}

extern "C" int64_t dfm_param_count(const dfm_hparams *hp)
{
    if (!hp || hp->depth < 1 || hp->depth > 8 || hp->family < 0 || hp->family > 1) return -1;
    return blob_floats(hp);
}

extern "C" int dfm_device_count(int *count)
{
    if (!count) return fail(DFM_E_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(DFM_E_NODEVICE, hipGetErrorString(e)); }
    *count = n;
    return DFM_OK;
}

extern "C" int dfm_set_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(DFM_E_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(DFM_E_INVALID, "device index out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DFM_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    return DFM_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int dfm_diffusion_coef(const dfm_hparams *hp, int which, double t, double *g_out, double *sigma_out)
{
    if (!hp) return fail(DFM_E_INVALID, "hp is NULL");
    if (which != 0 && which != 1) return fail(DFM_E_INVALID, "which must be 0 (R^3) or 1 (SO(3))");
    if (diffusion_coef(*hp, which, t, g_out, sigma_out) != DFM_OK) return fail(DFM_E_INVALID, "Invalid t (so3 sigma needs 0 <= t <= 1)");
    return DFM_OK;
}

extern "C" long long dfm_trim_cache(int device)
{
    if (device >= MAX_DEVICES) return 0;      // no such device: nothing parked there (a negative index means every device)
    return (long long)g_block_cache.trim(device < 0 ? -1 : device);
}

extern "C" int dfm_alloc_diag(int64_t out[6])
{
    if (!out) return fail(DFM_E_INVALID, "NULL argument");
    const AllocDiag &d = g_alloc_diag;
    out[0] = d.blocks.load(std::memory_order_relaxed); out[1] = d.poisoned.load(std::memory_order_relaxed);
    out[2] = d.bands.load(std::memory_order_relaxed); out[3] = d.damaged.load(std::memory_order_relaxed);
    out[4] = d.first_size.load(std::memory_order_relaxed); out[5] = d.first_off.load(std::memory_order_relaxed);
    return DFM_OK;
}

// Precision plan of the 16-bit MFMA engine (DFM_F_MFMA16).  Chosen on FOUR weight draws run through the reference - three
// seeds and one draw with every edge / node / coordinate MLP Linear times 3 (tests/golden/make_golden_draws.py,
// profiles/r03_exp_draw_knobs*.txt) - at SURVEY 8(d)'s gates (1e-2 on f / scores, 3e-2 on energy):
//   * per-edge contractions: fp16 operands in EVERY layer (same MFMA rate as bf16, 3 more mantissa bits).  With bf16 operands in
//     layers 0..4 (the r02 plan, now opt-in: DFM_F_BF16_OPS) the 3x-scaled draw reaches 1.5e-2 on f and 1.4e-2 on rot_score: the
//     rounding of the 256 x 256 weights to 8 bits is coherent over all edges and does not average out.  fp16 has no range cost
//     here: the gathered operands (Wb h_j, the lookup tables) are stored as fp16 in either plan.
//   * A_i = Wa h_i + b1 is read as fp16 in every layer (it joins Bm_j and the tables; fp32 A_i changes no worst case); the f16
//     engine (DFM_F_F16) keeps fp32.
//   * node-level GEMMs: three terms on split-bf16 operands (~1e-5).  The two-term fp16 form of r02 (weights as ONE fp16 tile) was
//     13 % faster per launch but its 2.4e-4 weight rounding is again coherent: 9.2e-3 on tr_score of the second family (seed 1);
//     it is gone.
extern "C" const char *dfm_config_string(void)
{
    static const std::string v = [] {
        std::string c = "mfma16: per-edge operands fp16 in every layer (DFM_F_BF16_OPS: bf16 in layers 0..depth-2), A_i fp16 "
                        "(DFM_F_F16: fp32), gathered Bm / tables fp16, node GEMMs ";
        c += "three-term split-bf16";
        c += ", fp32 accumulate / geometry / GraphNorm statistics / heads / SDE step";
        c += "; layer 0 through the per-complex message table in dfm_sample (DFM_F_NO_L0_TABLE: direct), on request in dfm_score (DFM_F_L0_TABLE)";
        c += "; dfm_refine: start from a given pose at t_begin (IGSO(3) cdf tables in float64, cached per sigma index), then dfm_sample's steps";
        std::string env;
        for (const char *k : {"DFM_EDGE_SPLIT", "DFM_GEMM_NARROW_MAXWG", "DFM_GEMM_QUARTER_MAXWG", "DFM_L0_TABLE", "DFM_GRAPH", "DFM_ALLOC_CACHE", "DFM_ALLOC_CACHE_FRAC", "DFM_ALLOC_POISON", "DFM_ALLOC_GUARD", "DFM_LIB"}) {
            const char *e = getenv(k);
            if (e) env += std::string(env.empty() ? "" : " ") + k + "=" + e;
        }
        c += "; env: " + (env.empty() ? std::string("none") : env);
        return c;
    }();
    return v.c_str();
}
