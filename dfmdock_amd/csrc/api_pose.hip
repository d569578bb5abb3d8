// api_pose.hip - the pose calls of the C ABI (include/dfmdock_amd.h): pose clustering, docking metrics, consensus contacts and the six
// rigid-pose families (sterics, buried surface, interface energy, residue contacts, hydrogen bonds, tabulated pair potential), the rigid pose fit and the density fit.  Every call owns a non-blocking
// stream and its temporaries; the handles are bound to the model handle's device only.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "dfm_host.h"
#include "dfm_poseprep.h"

using namespace dfm;

// ------------------------------------------------------------------------------------------------
// Pose clustering (kernels_cluster.hip).  Bound to the model handle: the drivers close a complex right after sampling, and clustering
// runs later, on the post-processing thread.  Every call owns a non-blocking stream and its temporaries (block cache), so calls from
// several host threads, and next to that model's complex handles, do not share any state.
// the two millisecond figures of this thread's last call of each kind, behind the dfm_*_last_timing getters: k_pose_dist and the
// clustering kernels for MS_CLUSTER, host-to-device copies and kernels for the others
enum { MS_CLUSTER, MS_METRICS, MS_CONSENSUS, MS_STERICS, MS_BSA, MS_IFACE, MS_RESCON, MS_HBOND, MS_PAIRPOT, MS_FIT, MS_DENSITY, MS_KINDS };
static thread_local double g_last_ms[MS_KINDS][2] = {};

static void set_last_ms(int kind, double a, double b)
{
    g_last_ms[kind][0] = a;
    g_last_ms[kind][1] = b;
}

static int last_timing(int kind, double *a, double *b)
{
    if (!a || !b) return fail(DFM_E_INVALID, "NULL argument");
    *a = g_last_ms[kind][0];
    *b = g_last_ms[kind][1];
    return DFM_OK;
}

static int check_pose_args(int B, int L, const float *lig_pos, const int32_t *residues, int n_res, std::vector<int32_t> *res_out)
{
    if (!lig_pos) return fail(DFM_E_INVALID, "lig_pos is NULL");
    if (B < 1 || L < 1) return fail(DFM_E_INVALID, "need B >= 1 and L >= 1");
    if (B > CL_MAX_POSES) return fail(DFM_E_INVALID, "at most " + std::to_string(CL_MAX_POSES) + " poses per call");
    if ((int64_t)L * 9 > INT32_MAX / 2) return fail(DFM_E_INVALID, "L too large");
    res_out->clear();
    if (residues) {
        if (n_res < 1 || n_res > L) return fail(DFM_E_INVALID, "need 1 <= n_res <= L");
        std::vector<char> seen((size_t)L, 0);
        for (int i = 0; i < n_res; ++i) {
            const int r = residues[i];
            if (r < 0 || r >= L) return fail(DFM_E_INVALID, "residue " + std::to_string(r) + " outside [0, " + std::to_string(L) + ")");
            if (seen[(size_t)r]) return fail(DFM_E_INVALID, "residue " + std::to_string(r) + " listed twice");
            seen[(size_t)r] = 1;
        }
        res_out->assign(residues, residues + n_res);
    }
    return DFM_OK;
}

// the call's stream and temporaries; the pool goes back to the block cache after the stream has drained
struct PoseCall {
    hipStream_t s = nullptr;
    DevPool tmp;
    hipEvent_t ev[4] = {};
    ~PoseCall()
    {
        if (s) (void)hipStreamSynchronize(s);
        tmp.release(true);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t open()
    {
        hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) { s = nullptr; return e; }
        tmp.bind(s);
        for (hipEvent_t &v : ev)
            if ((e = hipEventCreate(&v)) != hipSuccess) { v = nullptr; return e; }
        return hipSuccess;
    }
    // uploads lig_pos and the subset; radius > 0 with rmsd == nullptr: the bitmask
    hipError_t dist(int B, int L, const float *lig_pos, const std::vector<int32_t> &res, float radius, float *rmsd, uint32_t **mask)
    {
        float *X = nullptr;
        int32_t *r = nullptr;
        hipError_t e = tmp.upload_async(&X, lig_pos, (size_t)B * L * 9, s);
        if (e == hipSuccess && !res.empty()) e = tmp.upload_async(&r, res.data(), res.size(), s);
        const int W = (B + 31) / 32;
        if (e == hipSuccess && !rmsd) e = tmp.alloc(mask, (size_t)B * W);
        if (e == hipSuccess) e = hipEventRecord(ev[0], s);
        if (e == hipSuccess) e = launch_pose_dist(X, B, L * 9, r, res.empty() ? L : (int)res.size(), radius, rmsd, rmsd ? nullptr : *mask, s);
        if (e == hipSuccess) e = hipEventRecord(ev[1], s);
        return e;
    }
};

// the per-phase kernel milliseconds of this thread's last call of the kinds that split them (MS_RESCON, MS_HBOND, MS_PAIRPOT), summed over the call's
// chunks: the memsets | the pose kernel and the cell walk | the finishing kernel
static thread_local double g_phase_ms[MS_KINDS][3] = {};

static int last_phases(int kind, double *zero_ms, double *walk_ms, double *finish_ms)
{
    if (!zero_ms || !walk_ms || !finish_ms) return fail(DFM_E_INVALID, "NULL argument");
    *zero_ms = g_phase_ms[kind][0];
    *walk_ms = g_phase_ms[kind][1];
    *finish_ms = g_phase_ms[kind][2];
    return DFM_OK;
}
#define DFM_LAST_TIMING(name, kind) \
    extern "C" int name(double *copy_ms, double *kernel_ms) { return last_timing(kind, copy_ms, kernel_ms); }

// ------------------------------------------------------------------------------------------------
// The rigid-pose calls (sterics, buried surface, interface energy, residue contacts, hydrogen bonds, pair potential).  A handle holds what the two atom
// sets and the rotation centre fix - the receptor's cell grid, the ligand in blocks of 64 neighbours, that family's per-atom arrays -
// and is read-only after creation; like a dfm_native it is bound to the model handle's device only, and every call owns its stream and
// temporaries.  What the six handles share:
struct PoseHandle {
    int device = 0, n_cells = 0, max_cell_atoms = 0;
    int default_chunk = 0;      // poses of a chunk when neither the call nor the creator names one (the surface works it out per call)
    float cell_edge = 0.f;
    DevPool pool;      // unbound: released under a device-wide wait, like a model's
    float *rec = nullptr, *lig = nullptr, *sphere = nullptr;
    int32_t *cell_start = nullptr;
    void set_grid(int dev, const WalkGrid &g, int max_cell, float edge)
    {
        device = dev; n_cells = g.nx * g.ny * g.nz; max_cell_atoms = max_cell; cell_edge = edge;
    }
    // the first three fields of every dfm_*_info
    void grid_info(int32_t *cells, int32_t *max_cell, float *edge) const
    {
        if (cells) *cells = n_cells;
        if (max_cell) *max_cell = max_cell_atoms;
        if (edge) *edge = cell_edge;
    }
};

template <class H> static void pose_destroy(H *h)
{
    if (!h) return;
    DeviceScope ds(h->device);
    h->pool.release();
    delete h;
}

// the uploads of a creator into its handle's pool, in the order they are named, on the creating call's stream; after a failure the rest
// are skipped
struct PoseUploads {
    DevPool &pool;
    hipStream_t s;
    hipError_t e;
    template <class T> PoseUploads &operator()(T **dst, const std::vector<T> &host)
    {
        if (e == hipSuccess) e = pool.upload_async(dst, host.data(), host.size(), s);
        return *this;
    }
};

// the tail of a creator: on the handle's device, run `uploads` on a stream of its own and wait for it; a failure releases and deletes the
// handle and is reported through the creator's own `bad` as "<creator>: <HIP's text>"
template <class H, class Bad, class Uploads> static H *pose_finish_create(H *h, const char *creator, Bad bad, Uploads uploads)
{
    DeviceScope ds(h->device);
    if (ds.err != hipSuccess) { delete h; return bad(DFM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(ds.err)); }
    hipError_t e = hipSuccess;
    {
        PoseCall c;
        e = c.open();
        PoseUploads up{h->pool, c.s, e};
        uploads(up);
        e = up.e;
        if (e == hipSuccess) e = hipStreamSynchronize(c.s);
    }      // the call's stream has drained: the host vectors it read may go
    if (e != hipSuccess) {
        h->pool.release(); delete h;
        return bad(e == hipErrorOutOfMemory ? DFM_E_OOM : DFM_E_HIP, std::string(creator) + ": " + hipGetErrorString(e));
    }
    return h;
}

// A rigid-pose call: its argument checks, device scope, stream and temporaries (begin), the chunk size and the chunk's (rot, tr) and
// transforms T on the device (alloc), and the call's copy / kernel milliseconds from its own events.  Per chunk: upload, the caller's
// memsets and launches, kernels_done, the caller's downloads, finish.  A call that splits its kernel time marks `zeroed` after its
// memsets and `walked` after its cell walk: ev[1] .. zeroed .. ev[3] (walked) .. ev[2].  done() leaves the figures for the getters.
struct PoseChunks {
    std::optional<DeviceScope> ds;      // declared first: the caller's device comes back after the stream has drained
    PoseCall c;
    const float *rot = nullptr, *tr = nullptr;
    float *d_rot = nullptr, *d_tr = nullptr;
    double *T = nullptr;
    int P = 0, Pc = 0;
    double copy_ms = 0.0, kernel_ms = 0.0, phase[3] = {0.0, 0.0, 0.0};
    hipEvent_t zeroed = nullptr;
    ~PoseChunks() { if (zeroed) (void)hipEventDestroy(zeroed); }
    // `name`: the handle's in the NULL message; max_P: the most poses of a call, 0 for no limit
    int begin(const PoseHandle *h, const char *name, int P_, int max_P, const float *rot_, const float *tr_, const void *out, int chunk_poses)
    {
        if (!h) return fail(DFM_E_INVALID, std::string(name) + " is NULL");
        if (!rot_) return fail(DFM_E_INVALID, "rot is NULL");
        if (!tr_) return fail(DFM_E_INVALID, "tr is NULL");
        if (!out) return fail(DFM_E_INVALID, "out is NULL");
        if (P_ < 1 || (max_P && P_ > max_P)) return fail(DFM_E_INVALID, max_P ? "need 1 <= P <= " + std::to_string(max_P) : std::string("need P >= 1"));
        if (chunk_poses < 0) return fail(DFM_E_INVALID, "chunk_poses must be >= 0");
        if (int rc = open(h->device, P_)) return rc;
        rot = rot_; tr = tr_;
        return DFM_OK;
    }
    // the device scope, stream and temporaries alone, for a call whose poses are not (rot, tr) (dfm_pose_fit): it uploads between
    // copies_begin and copies_done, and from kernels_done on the chunk runs as every other
    int open(int device, int P_)
    {
        ds.emplace(device);
        if (ds->err != hipSuccess) return fail(DFM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(ds->err));
        HIPCHK(c.open());
        P = P_;
        return DFM_OK;
    }
    hipError_t copies_begin() { return hipEventRecord(c.ev[0], c.s); }
    hipError_t copies_done() { return hipEventRecord(c.ev[1], c.s); }
    // the chunk: `want` poses if one was asked for (at most the launch's `cap`), else `fallback`
    int alloc(int want, int fallback, int cap)
    {
        Pc = std::min(P, want > 0 ? std::min(want, cap) : fallback);
        HIPCHK(c.tmp.alloc(&d_rot, (size_t)Pc * 3));
        HIPCHK(c.tmp.alloc(&d_tr, (size_t)Pc * 3));
        HIPCHK(c.tmp.alloc(&T, (size_t)Pc * 12));
        return DFM_OK;
    }
    hipError_t upload(int p0, int n)
    {
        hipError_t e = copies_begin();
        if (e == hipSuccess) e = hipMemcpyAsync(d_rot, rot + (size_t)p0 * 3, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c.s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tr, tr + (size_t)p0 * 3, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c.s);
        if (e == hipSuccess) e = copies_done();
        return e;
    }
    hipError_t mark_zeroed()
    {
        if (!zeroed)
            if (hipError_t e = hipEventCreate(&zeroed); e != hipSuccess) { zeroed = nullptr; return e; }
        return hipEventRecord(zeroed, c.s);
    }
    hipError_t mark_walked() { return hipEventRecord(c.ev[3], c.s); }
    hipError_t kernels_done() { return hipEventRecord(c.ev[2], c.s); }
    hipError_t finish()
    {
        const hipError_t e = hipStreamSynchronize(c.s);
        if (e != hipSuccess) return e;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c.ev[0], c.ev[1]) == hipSuccess) copy_ms += ms;
        if (hipEventElapsedTime(&ms, c.ev[1], c.ev[2]) == hipSuccess) kernel_ms += ms;
        if (zeroed) {
            if (hipEventElapsedTime(&ms, c.ev[1], zeroed) == hipSuccess) phase[0] += ms;
            if (hipEventElapsedTime(&ms, zeroed, c.ev[3]) == hipSuccess) phase[1] += ms;
            if (hipEventElapsedTime(&ms, c.ev[3], c.ev[2]) == hipSuccess) phase[2] += ms;
        }
        return e;
    }
    int done(int kind)
    {
        set_last_ms(kind, copy_ms, kernel_ms);
        if (zeroed)
            for (int k = 0; k < 3; ++k) g_phase_ms[kind][k] = phase[k];
        return DFM_OK;
    }
};

extern "C" int dfm_pose_rmsd(dfm_model *m, int B, int L, const float *lig_pos, const int32_t *residues, int n_res, float *rmsd)
{
    if (!m || !rmsd) return fail(DFM_E_INVALID, "NULL argument");
    std::vector<int32_t> res;
    if (int rc = check_pose_args(B, L, lig_pos, residues, n_res, &res)) return rc;
    DEVICE_SCOPE(m->device);
    PoseCall c;
    HIPCHK(c.open());
    float *d = nullptr;
    HIPCHK(c.tmp.alloc(&d, (size_t)B * B));
    HIPCHK(c.dist(B, L, lig_pos, res, 1.0f, d, nullptr));
    HIPCHK(hipMemcpyAsync(rmsd, d, (size_t)B * B * sizeof(float), hipMemcpyDeviceToHost, c.s));
    HIPCHK(hipStreamSynchronize(c.s));
    float ms = 0.f;
    set_last_ms(MS_CLUSTER, hipEventElapsedTime(&ms, c.ev[0], c.ev[1]) == hipSuccess ? ms : -1.0, 0.0);
    return DFM_OK;
}

extern "C" int dfm_pose_cluster(dfm_model *m, int B, int L, const float *lig_pos, const int32_t *residues, int n_res, const float *key,
                                float radius, int rule, int max_clusters, int32_t *n_clusters, int32_t *center, int32_t *size,
                                int32_t *cluster_of)
{
    if (!m || !n_clusters || !center || !size || !cluster_of) return fail(DFM_E_INVALID, "NULL argument");
    std::vector<int32_t> res;
    if (int rc = check_pose_args(B, L, lig_pos, residues, n_res, &res)) return rc;
    if (!(radius > 0.f) || !std::isfinite(radius)) return fail(DFM_E_INVALID, "radius must be finite and > 0");
    if (rule != DFM_CLUSTER_ENERGY && rule != DFM_CLUSTER_SIZE) return fail(DFM_E_INVALID, "rule must be 0 (energy) or 1 (size)");
    if (max_clusters < 1) return fail(DFM_E_INVALID, "max_clusters must be >= 1");
    const int maxc = max_clusters < B ? max_clusters : B;
    // key order on the host: lower key first, ties to the lower index, NaN last (dfmdock_amd/cluster.py: rank_order)
    std::vector<int32_t> order((size_t)B), pos((size_t)B);
    for (int i = 0; i < B; ++i) order[(size_t)i] = i;
    if (key) {
        std::stable_sort(order.begin(), order.end(), [key](int32_t a, int32_t b) {
            const bool na = std::isnan(key[a]), nb = std::isnan(key[b]);
            if (na != nb) return nb;
            return !na && key[a] < key[b];
        });
    }
    for (int i = 0; i < B; ++i) pos[(size_t)order[(size_t)i]] = i;
    DEVICE_SCOPE(m->device);
    PoseCall c;
    HIPCHK(c.open());
    uint32_t *mask = nullptr;
    int32_t *d_order = nullptr, *d_out = nullptr;
    const size_t out_n = (size_t)B + 2 * (size_t)maxc + 4;      // cluster_of | center | size | state
    HIPCHK(c.tmp.upload_async(&d_order, order.data(), order.size(), c.s));
    HIPCHK(c.tmp.alloc(&d_out, out_n));
    HIPCHK(c.dist(B, L, lig_pos, res, radius, nullptr, &mask));
    int32_t *d_of = d_out, *d_center = d_out + B, *d_size = d_center + maxc, *d_state = d_size + maxc;
    if (rule == DFM_CLUSTER_ENERGY) {
        HIPCHK(launch_cluster_leader(mask, B, d_order, maxc, d_of, d_center, d_size, d_state, c.s));
    } else {
        int32_t *d_pos = nullptr, *counts = nullptr, *mlist = nullptr;
        uint32_t *U = nullptr;
        HIPCHK(c.tmp.upload_async(&d_pos, pos.data(), pos.size(), c.s));
        HIPCHK(c.tmp.alloc(&counts, (size_t)B));
        HIPCHK(c.tmp.alloc(&mlist, (size_t)B));
        HIPCHK(c.tmp.alloc(&U, (size_t)(B + 31) / 32));
        HIPCHK(launch_cluster_count(mask, B, counts, U, d_of, d_state, c.s));
        // one pick + decrement per cluster; the steps after the last pose is assigned return at once.  Every 64 clusters the host
        // looks at the done flag, so a run that ends early does not enqueue max_clusters steps.
        int32_t st[3] = {0, 0, 0};
        for (int k = 0; k < maxc; ++k) {
            HIPCHK(launch_cluster_step(mask, B, counts, d_pos, d_order, U, d_of, d_center, d_size, mlist, d_state, c.s));
            if ((k & 63) == 63 && k + 1 < maxc) {
                HIPCHK(hipMemcpyAsync(st, d_state, sizeof(st), hipMemcpyDeviceToHost, c.s));
                HIPCHK(hipStreamSynchronize(c.s));
                if (st[1]) break;
            }
        }
    }
    HIPCHK(hipEventRecord(c.ev[2], c.s));
    std::vector<int32_t> h(out_n);
    HIPCHK(hipMemcpyAsync(h.data(), d_out, out_n * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    HIPCHK(hipStreamSynchronize(c.s));
    const int n = h[(size_t)B + 2 * maxc];
    if (n < 0 || n > maxc) return fail(DFM_E_HIP, "clustering kernel returned " + std::to_string(n) + " clusters");
    *n_clusters = n;
    std::memcpy(cluster_of, h.data(), (size_t)B * sizeof(int32_t));
    std::memcpy(center, h.data() + B, (size_t)n * sizeof(int32_t));
    std::memcpy(size, h.data() + B + maxc, (size_t)n * sizeof(int32_t));
    float ms = 0.f;
    const double dist_ms = hipEventElapsedTime(&ms, c.ev[0], c.ev[1]) == hipSuccess ? ms : -1.0;
    set_last_ms(MS_CLUSTER, dist_ms, hipEventElapsedTime(&ms, c.ev[1], c.ev[2]) == hipSuccess ? ms : -1.0);
    return DFM_OK;
}

extern "C" int dfm_pose_last_timing(double *dist_ms, double *cluster_ms)
{
    return last_timing(MS_CLUSTER, dist_ms, cluster_ms);
}

// ------------------------------------------------------------------------------------------------
// Docking metrics (kernels_metrics.hip).  A dfm_native holds what the native alone fixes and is read-only after creation; like the
// clustering calls it is bound to the model handle's device only, and every dfm_pose_metrics call owns its stream and temporaries.
constexpr size_t METRICS_CHUNK_BYTES = (size_t)64 << 20;      // poses uploaded and evaluated per chunk of a call

struct dfm_native {
    int device = 0, R = 0, L = 0;
    DevPool pool;      // unbound: released under a device-wide wait, like a model's
    float *rec = nullptr, *lig = nullptr;
    uint8_t *frec = nullptr, *flig = nullptr;
    int32_t *contacts = nullptr;
    double *rec_const = nullptr;      // the receptor's sums with the native receptor as its own model (k_metrics_reduce)
    MetricsConst mc = {};
    std::vector<int32_t> iface_rec, iface_lig, pairs;
};

extern "C" void dfm_native_destroy(dfm_native *nat)
{
    if (!nat) return;
    DeviceScope ds(nat->device);
    nat->pool.release();
    delete nat;
}

extern "C" dfm_native *dfm_native_create(dfm_model *m, const float *rec_pos, const float *lig_pos, int R, int L, float iface_cutoff,
                                         float contact_cutoff)
{
    auto bad = [](int code, const std::string &msg) -> dfm_native * { (void)fail(code, msg); return nullptr; };
    if (!m || !rec_pos || !lig_pos) return bad(DFM_E_INVALID, "NULL argument");
    if (R < 1 || L < 1) return bad(DFM_E_INVALID, "need R >= 1 and L >= 1");
    if ((int64_t)R * L > ((int64_t)1 << 27)) return bad(DFM_E_INVALID, "R x L exceeds 2^27 residue pairs");
    if (!std::isfinite(iface_cutoff) || !std::isfinite(contact_cutoff)) return bad(DFM_E_INVALID, "cutoffs must be finite");
    DeviceScope ds(m->device);
    if (ds.err != hipSuccess) return bad(DFM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(ds.err));
    dfm_native *nat = new dfm_native;
    nat->device = m->device; nat->R = R; nat->L = L;
    hipError_t e = hipSuccess;
    {
        PoseCall c;
        uint8_t *d_pairs = nullptr;
        std::vector<uint8_t> pm((size_t)R * L);
        e = c.open();
        if (e == hipSuccess) e = nat->pool.upload_async(&nat->rec, rec_pos, (size_t)R * 9, c.s);
        if (e == hipSuccess) e = nat->pool.upload_async(&nat->lig, lig_pos, (size_t)L * 9, c.s);
        if (e == hipSuccess) e = c.tmp.alloc(&d_pairs, pm.size());
        if (e == hipSuccess) e = launch_native_pairs(nat->rec, nat->lig, R, L, (double)iface_cutoff, (double)contact_cutoff, d_pairs, c.s);
        if (e == hipSuccess) e = hipMemcpyAsync(pm.data(), d_pairs, pm.size(), hipMemcpyDeviceToHost, c.s);
        if (e == hipSuccess) e = hipStreamSynchronize(c.s);
        std::vector<uint8_t> fr((size_t)R, 0), fl((size_t)L, 0);
        MetricsConst &mc = nat->mc;
        if (e == hipSuccess) {
            for (int i = 0; i < R; ++i)
                for (int j = 0; j < L; ++j) {
                    const uint8_t b = pm[(size_t)i * L + j];
                    if (b & 1) { fr[(size_t)i] = 1; fl[(size_t)j] = 1; }
                    if (b & 2) { nat->pairs.push_back(i); nat->pairs.push_back(j); }
                }
            for (int i = 0; i < R; ++i) if (fr[(size_t)i]) nat->iface_rec.push_back(i);
            for (int j = 0; j < L; ++j) if (fl[(size_t)j]) nat->iface_lig.push_back(j);
            // the shift: the all-atom centroid rounded to fp32 (p - o is then exact in fp64 for every fp32 coordinate near the complex)
            double cen[3] = {0.0, 0.0, 0.0};
            for (int i = 0; i < R * 9; ++i) cen[i % 3] += (double)rec_pos[i];
            for (int i = 0; i < L * 9; ++i) cen[i % 3] += (double)lig_pos[i];
            for (int k = 0; k < 3; ++k) {
                const float of = (float)(cen[k] / (3.0 * ((double)R + (double)L)));
                mc.o[k] = std::isfinite(of) ? (double)of : 0.0;
            }
            for (int i = 0; i < R; ++i)
                for (int k = 0; k < 9; ++k) {
                    const double q = (double)rec_pos[(size_t)i * 9 + k] - mc.o[k % 3];
                    mc.T_rec[k % 3] += q;
                    if (fr[(size_t)i]) mc.T_rec_iface[k % 3] += q;
                }
            for (int j = 0; j < L; ++j)
                for (int k = 0; k < 9; ++k) {
                    const double q = (double)lig_pos[(size_t)j * 9 + k] - mc.o[k % 3];
                    mc.T_lig[k % 3] += q;
                    if (fl[(size_t)j]) mc.T_lig_iface[k % 3] += q;
                }
            mc.n_rec = R; mc.n_lig = L;
            mc.n_rec_iface = (int)nat->iface_rec.size(); mc.n_lig_iface = (int)nat->iface_lig.size();
            mc.n_contacts = (int)(nat->pairs.size() / 2);
            mc.rec_moves = 0;
            mc.contact_cutoff = (double)contact_cutoff;
            e = nat->pool.upload_async(&nat->frec, fr.data(), fr.size(), c.s);
        }
        if (e == hipSuccess) e = nat->pool.upload_async(&nat->flig, fl.data(), fl.size(), c.s);
        if (e == hipSuccess) e = nat->pool.upload_async(&nat->contacts, nat->pairs.data(), nat->pairs.size(), c.s);
        if (e == hipSuccess) e = nat->pool.alloc(&nat->rec_const, 24);
        if (e == hipSuccess) {
            const MetricsChain rc = {nat->rec, nat->rec, nat->frec, R};
            e = launch_metrics_reduce(rc, rc, 1, 1, mc, nat->rec_const, c.s);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c.s);
    }      // the call's stream has drained: the host vectors it read may go
    if (e != hipSuccess) {
        nat->pool.release();
        delete nat;
        return bad(e == hipErrorOutOfMemory ? DFM_E_OOM : DFM_E_HIP, std::string("dfm_native_create: ") + hipGetErrorString(e));
    }
    return nat;
}

extern "C" int dfm_native_info(const dfm_native *nat, int32_t *n_iface_rec, int32_t *n_iface_lig, int32_t *n_contacts, int32_t *iface_rec,
                               int32_t *iface_lig, int32_t *contacts)
{
    if (!nat) return fail(DFM_E_INVALID, "NULL argument");
    if (n_iface_rec) *n_iface_rec = (int32_t)nat->iface_rec.size();
    if (n_iface_lig) *n_iface_lig = (int32_t)nat->iface_lig.size();
    if (n_contacts) *n_contacts = (int32_t)(nat->pairs.size() / 2);
    if (iface_rec && !nat->iface_rec.empty()) std::memcpy(iface_rec, nat->iface_rec.data(), nat->iface_rec.size() * sizeof(int32_t));
    if (iface_lig && !nat->iface_lig.empty()) std::memcpy(iface_lig, nat->iface_lig.data(), nat->iface_lig.size() * sizeof(int32_t));
    if (contacts && !nat->pairs.empty()) std::memcpy(contacts, nat->pairs.data(), nat->pairs.size() * sizeof(int32_t));
    return DFM_OK;
}

// Python's round(x, 6): the correctly rounded six-decimal string, read back
static double round6(double x)
{
    if (!std::isfinite(x)) return x;
    char buf[64];
    snprintf(buf, sizeof(buf), "%.6f", x);
    return strtod(buf, nullptr);
}
// libm's pow through a pointer the compiler cannot fold: metrics.py's `** 2` is that call, and the results are compared bit for bit
static double (*volatile g_pow)(double, double) = static_cast<double (*)(double, double)>(std::pow);

extern "C" int dfm_pose_metrics(dfm_native *nat, int P, const float *lig_pos, const float *rec_pos, dfm_metrics_out *out)
{
    if (!nat || !out) return fail(DFM_E_INVALID, "NULL argument");
    if (!lig_pos) return fail(DFM_E_INVALID, "lig_pos is NULL");
    if (P < 1) return fail(DFM_E_INVALID, "need P >= 1");
    DEVICE_SCOPE(nat->device);
    PoseCall c;
    HIPCHK(c.open());
    const int R = nat->R, L = nat->L, chains = rec_pos ? 2 : 1;
    const size_t lig_n = (size_t)L * 9, rec_n = (size_t)R * 9, per_pose = (lig_n + (rec_pos ? rec_n : 0)) * sizeof(float);
    const int Pc = (int)std::min<size_t>((size_t)P, std::max<size_t>(1, METRICS_CHUNK_BYTES / per_pose));
    float *X = nullptr, *Xr = nullptr;
    double *sums = nullptr, *xf = nullptr, *d_rmsd = nullptr;
    int32_t *d_cnt = nullptr;
    HIPCHK(c.tmp.alloc(&X, (size_t)Pc * lig_n));
    if (rec_pos) HIPCHK(c.tmp.alloc(&Xr, (size_t)Pc * rec_n));
    HIPCHK(c.tmp.alloc(&sums, (size_t)Pc * chains * 24));
    HIPCHK(c.tmp.alloc(&xf, (size_t)Pc * 36));
    HIPCHK(c.tmp.alloc(&d_rmsd, (size_t)Pc * 3));
    HIPCHK(c.tmp.alloc(&d_cnt, (size_t)Pc));
    MetricsConst mc = nat->mc;
    mc.rec_moves = rec_pos ? 1 : 0;
    const MetricsChain lig = {X, nat->lig, nat->flig, L}, rec = {rec_pos ? Xr : nat->rec, nat->rec, nat->frec, R};
    std::vector<double> h_rmsd((size_t)P * 3);
    std::vector<int32_t> h_cnt((size_t)P);
    double copy_ms = 0.0, kernel_ms = 0.0;
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(hipEventRecord(c.ev[0], c.s));
        HIPCHK(hipMemcpyAsync(X, lig_pos + (size_t)p0 * lig_n, (size_t)n * lig_n * sizeof(float), hipMemcpyHostToDevice, c.s));
        if (rec_pos) HIPCHK(hipMemcpyAsync(Xr, rec_pos + (size_t)p0 * rec_n, (size_t)n * rec_n * sizeof(float), hipMemcpyHostToDevice, c.s));
        HIPCHK(hipEventRecord(c.ev[1], c.s));
        HIPCHK(launch_metrics_reduce(lig, rec, chains, n, mc, sums, c.s));
        HIPCHK(launch_metrics_finish(lig, rec, sums, chains, nat->rec_const, mc, nat->contacts, n, xf, d_rmsd, d_cnt, c.s));
        HIPCHK(hipEventRecord(c.ev[2], c.s));
        HIPCHK(hipMemcpyAsync(h_rmsd.data() + (size_t)p0 * 3, d_rmsd, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, c.s));
        HIPCHK(hipMemcpyAsync(h_cnt.data() + p0, d_cnt, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(hipStreamSynchronize(c.s));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c.ev[0], c.ev[1]) == hipSuccess) copy_ms += ms;
        if (hipEventElapsedTime(&ms, c.ev[1], c.ev[2]) == hipSuccess) kernel_ms += ms;
    }
    set_last_ms(MS_METRICS, copy_ms, kernel_ms);
    const double nc = (double)mc.n_contacts;
    for (int p = 0; p < P; ++p) {
        const double cr = h_rmsd[(size_t)p * 3], ir = h_rmsd[(size_t)p * 3 + 1], lr = h_rmsd[(size_t)p * 3 + 2];
        const double fnat = round6((double)h_cnt[(size_t)p] / (nc + 1e-6));
        if (out->c_rmsd) out->c_rmsd[p] = cr;
        if (out->i_rmsd) out->i_rmsd[p] = ir;
        if (out->l_rmsd) out->l_rmsd[p] = lr;
        if (out->fnat) out->fnat[p] = fnat;
        if (out->dockq) out->dockq[p] = (fnat + 1.0 / (1.0 + g_pow(ir / 1.5, 2.0)) + 1.0 / (1.0 + g_pow(lr / 8.5, 2.0))) / 3.0;
        if (out->n_recovered) out->n_recovered[p] = h_cnt[(size_t)p];
    }
    return DFM_OK;
}

extern "C" int dfm_metrics_last_timing(double *copy_ms, double *kernel_ms)
{
    return last_timing(MS_METRICS, copy_ms, kernel_ms);
}

// ------------------------------------------------------------------------------------------------
// Consensus contact scoring (kernels_consensus.hip).  Bound to the model handle's device only, like the clustering calls; every call owns
// its stream and temporaries.  A chunk holds its poses and their contact bits; a call of one chunk keeps the bits between the counting
// and the scoring pass, a longer call uploads and evaluates every chunk again in the scoring pass.
constexpr size_t CONSENSUS_CHUNK_BYTES = (size_t)256 << 20;
constexpr int CONSENSUS_MAX_POSES = 65536;

extern "C" int dfm_consensus_chunk_poses(int R, int L)
{
    if (R < 1 || L < 1) return 0;
    const size_t per_pose = (size_t)L * 9 * sizeof(float) + (size_t)R * (size_t)((L + 63) / 64) * sizeof(uint64_t);
    return (int)std::min<size_t>(32768, std::max<size_t>(1, CONSENSUS_CHUNK_BYTES / per_pose));      // (a launch takes 65535 poses)
}

extern "C" int dfm_pose_consensus(dfm_model *m, int P, int R, int L, const float *rec_pos, const float *lig_pos, const uint8_t *member,
                                  float cutoff, dfm_consensus_out *out)
{
    if (!m) return fail(DFM_E_INVALID, "m is NULL");
    if (!rec_pos) return fail(DFM_E_INVALID, "rec_pos is NULL");
    if (!lig_pos) return fail(DFM_E_INVALID, "lig_pos is NULL");
    if (!out) return fail(DFM_E_INVALID, "out is NULL");
    if (P < 1 || P > CONSENSUS_MAX_POSES) return fail(DFM_E_INVALID, "P must be in 1 .. " + std::to_string(CONSENSUS_MAX_POSES));
    if (R < 1 || L < 1) return fail(DFM_E_INVALID, "need R >= 1 and L >= 1");
    if ((int64_t)R * L > ((int64_t)1 << 27)) return fail(DFM_E_INVALID, "R x L exceeds 2^27 residue pairs");
    if (!std::isfinite(cutoff) || !(cutoff > 0.f)) return fail(DFM_E_INVALID, "cutoff must be finite and > 0");
    std::vector<uint8_t> mem((size_t)P, 1);
    if (member) {
        size_t M = 0;
        for (int p = 0; p < P; ++p) M += (mem[(size_t)p] = member[p] ? 1 : 0);
        if (M == 0) return fail(DFM_E_INVALID, "member: no pose is a member");
    }
    DEVICE_SCOPE(m->device);
    PoseCall c;
    HIPCHK(c.open());
    const int W = (L + 63) / 64, Pc = std::min(P, dfm_consensus_chunk_poses(R, L));
    const size_t lig_n = (size_t)L * 9, words = (size_t)W * R, RL = (size_t)R * L;
    const bool one_chunk = Pc >= P, want_count = out->count || out->rec_count || out->lig_count || out->score_sum;
    const bool want_pose = out->n_contacts || out->score_sum;
    float *d_rec = nullptr, *X = nullptr;
    uint8_t *d_mem = nullptr;
    uint64_t *d_bits = nullptr;
    int32_t *d_count = nullptr, *d_marg = nullptr, *d_n = nullptr;
    int64_t *d_sum = nullptr;
    HIPCHK(c.tmp.upload_async(&d_rec, rec_pos, (size_t)R * 9, c.s));
    HIPCHK(c.tmp.upload_async(&d_mem, mem.data(), mem.size(), c.s));
    HIPCHK(c.tmp.alloc(&X, (size_t)Pc * lig_n));
    HIPCHK(c.tmp.alloc(&d_bits, (size_t)Pc * words));
    HIPCHK(c.tmp.alloc(&d_count, RL));
    HIPCHK(c.tmp.alloc(&d_marg, (size_t)R + L));      // rec_count | lig_count
    HIPCHK(c.tmp.alloc(&d_n, (size_t)Pc));
    HIPCHK(c.tmp.alloc(&d_sum, (size_t)Pc));
    HIPCHK(hipMemsetAsync(d_count, 0, RL * sizeof(int32_t), c.s));
    HIPCHK(hipMemsetAsync(d_marg, 0, ((size_t)R + L) * sizeof(int32_t), c.s));
    std::vector<uint64_t> h_bits(out->bits ? (size_t)Pc * words : 0);
    double copy_ms = 0.0, kernel_ms = 0.0;
    // pass 0: bits and counts of every chunk; pass 1: per-pose sums against the finished counts
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && !want_pose) break;
        for (int p0 = 0; p0 < P; p0 += Pc) {
            const int n = std::min(Pc, P - p0);
            HIPCHK(hipEventRecord(c.ev[0], c.s));
            if (pass == 0 || !one_chunk)
                HIPCHK(hipMemcpyAsync(X, lig_pos + (size_t)p0 * lig_n, (size_t)n * lig_n * sizeof(float), hipMemcpyHostToDevice, c.s));
            HIPCHK(hipEventRecord(c.ev[1], c.s));
            if (pass == 0 || !one_chunk) HIPCHK(launch_contact_bits(d_rec, X, n, R, L, cutoff, d_bits, c.s));
            if (pass == 0 && want_count) HIPCHK(launch_contact_count(d_bits, d_mem + p0, n, R, L, d_count, d_marg, d_marg + R, c.s));
            if (pass == 1) HIPCHK(launch_contact_score(d_bits, d_count, n, R, L, d_n, d_sum, c.s));
            HIPCHK(hipEventRecord(c.ev[2], c.s));
            if (pass == 0 && out->bits)
                HIPCHK(hipMemcpyAsync(h_bits.data(), d_bits, (size_t)n * words * sizeof(uint64_t), hipMemcpyDeviceToHost, c.s));
            if (pass == 1 && out->n_contacts)
                HIPCHK(hipMemcpyAsync(out->n_contacts + p0, d_n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
            if (pass == 1 && out->score_sum)
                HIPCHK(hipMemcpyAsync(out->score_sum + p0, d_sum, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
            HIPCHK(hipStreamSynchronize(c.s));
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c.ev[0], c.ev[1]) == hipSuccess) copy_ms += ms;
            if (hipEventElapsedTime(&ms, c.ev[1], c.ev[2]) == hipSuccess) kernel_ms += ms;
            if (pass == 0 && out->bits)      // device [n][W][R] -> the ABI's [P][R][W]
                for (int p = 0; p < n; ++p)
                    for (int w = 0; w < W; ++w) {
                        const uint64_t *src = h_bits.data() + ((size_t)p * W + w) * R;
                        uint64_t *dst = out->bits + (size_t)(p0 + p) * words + w;
                        for (int i = 0; i < R; ++i) dst[(size_t)i * W] = src[i];
                    }
        }
    }
    if (out->count) HIPCHK(hipMemcpyAsync(out->count, d_count, RL * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    if (out->rec_count) HIPCHK(hipMemcpyAsync(out->rec_count, d_marg, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    if (out->lig_count) HIPCHK(hipMemcpyAsync(out->lig_count, d_marg + R, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    HIPCHK(hipStreamSynchronize(c.s));
    set_last_ms(MS_CONSENSUS, copy_ms, kernel_ms);
    return DFM_OK;
}

DFM_LAST_TIMING(dfm_consensus_last_timing, MS_CONSENSUS)

// ------------------------------------------------------------------------------------------------
// All-atom clash / contact screen (kernels_sterics.hip): the receptor's grid of cells of the contact cutoff.
constexpr size_t STERICS_CHUNK_BYTES = (size_t)64 << 20;      // per-atom output of one chunk of a call
constexpr int STERICS_MAX_CHUNK = 32768;                      // poses per launch (gridDim.y)
static thread_local int g_sterics_count = 0;                  // dfm_sterics_exit_counts: count the early exits of this thread's calls
static thread_local uint64_t g_sterics_exits[3] = {0, 0, 0};  // waves, left at the sphere test, left at the box test

struct dfm_atoms : PoseHandle {
    int Ar = 0, Al = 0;
    int chunk_poses = 0;      // the creator's chunk (0: none given); default_chunk: poses whose per-atom output fills STERICS_CHUNK_BYTES
    int32_t *lig_index = nullptr;
    StericsConst sc = {};
};

extern "C" void dfm_atoms_destroy(dfm_atoms *a) { pose_destroy(a); }

extern "C" dfm_atoms *dfm_atoms_create(dfm_model *m, int Ar, const float *rec_atoms, int Al, const float *lig_atoms, const float center[3],
                                       const dfm_sterics_params *p_or_null)
{
    auto bad = [](int code, const std::string &msg) -> dfm_atoms * { (void)fail(code, msg); return nullptr; };
    if (!m) return bad(DFM_E_INVALID, "m is NULL");
    if (const std::string msg = check_atom_sets(Ar, rec_atoms, Al, lig_atoms, center); !msg.empty()) return bad(DFM_E_INVALID, msg);
    dfm_sterics_params prm = {3.0f, 5.0f, 0};
    if (p_or_null) prm = *p_or_null;
    if (!std::isfinite(prm.clash_cutoff) || !std::isfinite(prm.contact_cutoff) || !(prm.clash_cutoff > 0.f) || !(prm.contact_cutoff > 0.f))
        return bad(DFM_E_INVALID, "cutoffs must be finite and > 0");
    if (prm.contact_cutoff < prm.clash_cutoff) return bad(DFM_E_INVALID, "contact_cutoff must be >= clash_cutoff");
    if (prm.chunk_poses < 0) return bad(DFM_E_INVALID, "chunk_poses must be >= 0");
    PoseFrame f;
    if (const std::string msg = build_pose_frame(Ar, rec_atoms, Al, lig_atoms, center, prm.contact_cutoff, "contact cutoff", f); !msg.empty())
        return bad(DFM_E_INVALID, msg);
    const std::vector<float> rec4 = gather4(f.gr.order, rec_atoms, nullptr), lig4 = gather4(f.lb.index, lig_atoms, nullptr);
    dfm_atoms *a = new dfm_atoms;
    a->set_grid(m->device, f.g, f.gr.max_cell, prm.contact_cutoff);
    a->Ar = Ar; a->Al = Al;
    a->sc.g = f.g;
    a->sc.contact = (double)prm.contact_cutoff;
    a->sc.clash = (double)prm.clash_cutoff;
    a->sc.reject2 = f.reject2;
    a->chunk_poses = prm.chunk_poses;
    a->default_chunk = (int)std::min<size_t>(STERICS_MAX_CHUNK, std::max<size_t>(1, STERICS_CHUNK_BYTES / ((size_t)Al * 2 * sizeof(int32_t))));
    return pose_finish_create(a, "dfm_atoms_create", bad, [&](PoseUploads &up) {
        up(&a->rec, rec4)(&a->cell_start, f.gr.start)(&a->lig, lig4)(&a->sphere, f.lb.sphere)(&a->lig_index, f.lb.index);
    });
}

extern "C" int dfm_atoms_info(const dfm_atoms *a, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge)
{
    if (!a) return fail(DFM_E_INVALID, "NULL argument");
    a->grid_info(n_cells, max_cell_atoms, cell_edge);
    return DFM_OK;
}

extern "C" int dfm_pose_sterics_chunked(dfm_atoms *a, int P, const float *rot, const float *tr, int chunk_poses, dfm_sterics_out *out)
{
    PoseChunks ch;
    if (int rc = ch.begin(a, "a", P, 0, rot, tr, out, chunk_poses)) return rc;
    PoseCall &c = ch.c;
    const bool per_atom = out->lig_clash || out->lig_contact;
    // the call's chunk, else the creator's, else the default: without per-atom output a chunk is bounded by the launch alone
    if (int rc = ch.alloc(chunk_poses > 0 ? chunk_poses : a->chunk_poses, per_atom ? a->default_chunk : STERICS_MAX_CHUNK, STERICS_MAX_CHUNK)) return rc;
    const int Pc = ch.Pc;
    const size_t Al = (size_t)a->Al;
    int32_t *d_cnt = nullptr, *d_lc = nullptr, *d_lt = nullptr;
    uint64_t *d_min = nullptr, *d_exits = nullptr;
    HIPCHK(c.tmp.alloc(&d_cnt, (size_t)Pc * 2));      // n_clash | n_contact
    HIPCHK(c.tmp.alloc(&d_min, (size_t)Pc));
    if (out->lig_clash) HIPCHK(c.tmp.alloc(&d_lc, (size_t)Pc * Al));
    if (out->lig_contact) HIPCHK(c.tmp.alloc(&d_lt, (size_t)Pc * Al));
    if (g_sterics_count) {
        HIPCHK(c.tmp.alloc(&d_exits, 2));
        HIPCHK(hipMemsetAsync(d_exits, 0, 2 * sizeof(uint64_t), c.s));
    }
    const StericsAtoms at = {a->rec, a->lig, a->sphere, a->cell_start, a->lig_index, a->sc, a->Ar, a->Al};
    std::vector<int32_t> h_cnt((size_t)Pc * 2);
    std::vector<uint64_t> h_min((size_t)Pc);
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.upload(p0, n));
        if (d_lc) HIPCHK(hipMemsetAsync(d_lc, 0, (size_t)n * Al * sizeof(int32_t), c.s));
        if (d_lt) HIPCHK(hipMemsetAsync(d_lt, 0, (size_t)n * Al * sizeof(int32_t), c.s));
        HIPCHK(launch_sterics_pose(ch.d_rot, ch.d_tr, n, ch.T, d_cnt, d_cnt + Pc, d_min, c.s));
        HIPCHK(launch_sterics(at, ch.T, n, d_cnt, d_cnt + Pc, d_min, d_lc, d_lt, d_exits, c.s));
        HIPCHK(ch.kernels_done());
        HIPCHK(hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)Pc * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(hipMemcpyAsync(h_min.data(), d_min, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, c.s));
        if (d_lc) HIPCHK(hipMemcpyAsync(out->lig_clash + (size_t)p0 * Al, d_lc, (size_t)n * Al * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_lt) HIPCHK(hipMemcpyAsync(out->lig_contact + (size_t)p0 * Al, d_lt, (size_t)n * Al * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
        for (int p = 0; p < n; ++p) {
            if (out->n_clash) out->n_clash[p0 + p] = h_cnt[(size_t)p];
            if (out->n_contact) out->n_contact[p0 + p] = h_cnt[(size_t)Pc + p];
            if (out->min_dist) std::memcpy(out->min_dist + p0 + p, &h_min[(size_t)p], sizeof(double));
        }
    }
    if (d_exits) {
        uint64_t h[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h, d_exits, sizeof(h), hipMemcpyDeviceToHost, c.s));
        HIPCHK(hipStreamSynchronize(c.s));
        g_sterics_exits[0] = (uint64_t)P * (uint64_t)((a->Al + 63) / 64);
        g_sterics_exits[1] = h[0];
        g_sterics_exits[2] = h[1];
    }
    return ch.done(MS_STERICS);
}

extern "C" int dfm_pose_sterics(dfm_atoms *a, int P, const float *rot, const float *tr, dfm_sterics_out *out)
{
    return dfm_pose_sterics_chunked(a, P, rot, tr, 0, out);
}

DFM_LAST_TIMING(dfm_sterics_last_timing, MS_STERICS)

extern "C" int dfm_sterics_exit_counts(int enable, uint64_t *counts_or_null)
{
    if (counts_or_null) std::memcpy(counts_or_null, g_sterics_exits, sizeof(g_sterics_exits));
    g_sterics_count = enable ? 1 : 0;
    return DFM_OK;
}

// ------------------------------------------------------------------------------------------------
// Buried surface area (kernels_surface.hip).  Beyond the shared part a dfm_surface holds what the radii, the probe and the sphere points
// fix: every atom's radius class and isolated exposure mask.  Its cell edge comes from the radii, not from a cutoff, so its creator
// keeps its own frame arithmetic.
constexpr size_t SURFACE_CHUNK_BYTES = (size_t)64 << 20;      // receptor masks and per-atom output of one chunk of a call

struct dfm_surface : PoseHandle {
    int Ar = 0, Al = 0, K = 0, n_classes = 0, chunk_poses = 0;
    float probe = 0.f, class_radius[16] = {};
    double sasa[2] = {0.0, 0.0};
    std::vector<int32_t> exposed[2];      // exposed points per atom, caller's order: receptor, ligand
    float *dirs = nullptr;
    int32_t *rec_index = nullptr, *lig_index = nullptr, *rec_class = nullptr, *lig_class = nullptr;
    uint64_t *rec_exp = nullptr, *lig_exp = nullptr;
    SurfaceConst sc = {};
};

extern "C" void dfm_surface_destroy(dfm_surface *s) { pose_destroy(s); }

extern "C" dfm_surface *dfm_surface_create(dfm_model *m, int Ar, const float *rec_atoms, const float *rec_radius, int Al,
                                           const float *lig_atoms, const float *lig_radius, const float center[3],
                                           const dfm_surface_params *p_or_null)
{
    auto bad = [](int code, const std::string &msg) -> dfm_surface * { (void)fail(code, msg); return nullptr; };
    if (!m) return bad(DFM_E_INVALID, "m is NULL");
    if (const std::string msg = check_atom_sets(Ar, rec_atoms, Al, lig_atoms, center); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (!rec_radius) return bad(DFM_E_INVALID, "rec_radius is NULL");
    if (!lig_radius) return bad(DFM_E_INVALID, "lig_radius is NULL");
    dfm_surface_params prm = {1.4f, 128, nullptr, 0};
    if (p_or_null) prm = *p_or_null;
    if (!std::isfinite(prm.probe) || !(prm.probe > 0.f)) return bad(DFM_E_INVALID, "probe must be finite and > 0");
    if (prm.K < 64 || prm.K > 256 || prm.K % 64) return bad(DFM_E_INVALID, "K must be a multiple of 64 in 64 .. 256");
    if (prm.chunk_poses < 0) return bad(DFM_E_INVALID, "chunk_poses must be >= 0");
    const int K = prm.K, G = K / 64;
    std::vector<float> dirs((size_t)K * 3);
    for (int k = 0; k < K; ++k) {
        if (prm.dirs) {
            for (int c = 0; c < 3; ++c) dirs[(size_t)k * 3 + c] = prm.dirs[(size_t)k * 3 + c];
        } else {
            const double z = 1.0 - (2.0 * k + 1.0) / K, r = std::sqrt(1.0 - z * z), phi = k * (M_PI * (3.0 - std::sqrt(5.0)));
            dirs[(size_t)k * 3] = (float)(r * std::cos(phi)); dirs[(size_t)k * 3 + 1] = (float)(r * std::sin(phi)); dirs[(size_t)k * 3 + 2] = (float)z;
        }
    }
    for (float v : dirs)
        if (!std::isfinite(v)) return bad(DFM_E_INVALID, "dirs is not finite");
    // the radius classes: the distinct fp32 values of both chains in ascending order (positive floats order like their bit patterns)
    std::vector<float> values;
    for (int side = 0; side < 2; ++side) {
        const float *rad = side ? lig_radius : rec_radius;
        for (int i = 0; i < (side ? Al : Ar); ++i) {
            if (!std::isfinite(rad[i]) || !(rad[i] > 0.f))
                return bad(DFM_E_INVALID, std::string(side ? "lig_radius" : "rec_radius") + ": atom " + std::to_string(i) + " is not finite and > 0");
            if (std::find(values.begin(), values.end(), rad[i]) == values.end()) {
                if (values.size() == 16) return bad(DFM_E_INVALID, "more than 16 radius classes");
                values.push_back(rad[i]);
            }
        }
    }
    std::sort(values.begin(), values.end());
    auto class_of = [&](float v) { return (int32_t)(std::lower_bound(values.begin(), values.end(), v) - values.begin()); };
    const double probe = (double)prm.probe, Rmax = (double)values.back() + probe;
    // one grid edge for the receptor's device grid and both host exposure grids: at least 2 Rmax, grown as dfm_posewalk.h grows a
    // reach - by the factor 1.0001 and the slack - which is also the fp32 pair test's allowance
    double maxabs = 0.0;
    for (size_t i = 0; i < (size_t)Ar * 3; ++i) maxabs = std::max(maxabs, std::fabs((double)rec_atoms[i]));
    for (size_t i = 0; i < (size_t)Al * 3; ++i) maxabs = std::max(maxabs, std::fabs((double)lig_atoms[i]));
    maxabs += 4.0 * Rmax + 1.0;
    const float slack = pose_slack(maxabs), thr = (float)(2.0 * Rmax) * 1.0001f + slack;
    if (!std::isfinite(thr)) return bad(DFM_E_INVALID, "radii and probe must be finite and > 0");
    const double edge = (double)thr, pad = 1e-6 + 1e-12 * maxabs;
    CellGrid gr, gl;
    if (!build_cell_grid(Ar, rec_atoms, edge, gr)) return bad(DFM_E_INVALID, "the receptor's bounding box needs more than 2^24 cells");
    if (!build_cell_grid(Al, lig_atoms, edge, gl)) return bad(DFM_E_INVALID, "the ligand's bounding box needs more than 2^24 cells");
    std::vector<uint64_t> rexp((size_t)Ar * G), lexp((size_t)Al * G);
    surface_exposure(Ar, rec_atoms, rec_radius, probe, K, dirs.data(), gr.lo, gr.dims, edge, pad, gr.start.data(), gr.order.data(), rexp.data());
    surface_exposure(Al, lig_atoms, lig_radius, probe, K, dirs.data(), gl.lo, gl.dims, edge, pad, gl.start.data(), gl.order.data(), lexp.data());
    dfm_surface *sf = new dfm_surface;
    sf->Ar = Ar; sf->Al = Al; sf->K = K; sf->probe = prm.probe; sf->chunk_poses = prm.chunk_poses;
    sf->n_classes = (int)values.size();
    for (size_t c = 0; c < values.size(); ++c) sf->class_radius[c] = values[c];
    // exposed points per atom and the isolated SASA: class sums in ascending order, left to right
    for (int side = 0; side < 2; ++side) {
        const int n = side ? Al : Ar;
        const float *rad = side ? lig_radius : rec_radius;
        const std::vector<uint64_t> &ex = side ? lexp : rexp;
        int64_t per_class[16] = {};
        sf->exposed[side].resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            int c = 0;
            for (int g = 0; g < G; ++g) c += __builtin_popcountll(ex[(size_t)i * G + g]);
            sf->exposed[side][(size_t)i] = c;
            per_class[class_of(rad[i])] += c;
        }
        double s = 0.0;
        for (size_t c = 0; c < values.size(); ++c) {
            const double R = (double)values[c] + probe;
            s = s + (double)per_class[c] * (4.0 * M_PI * R * R / K);
        }
        sf->sasa[side] = s;
    }
    SurfaceConst sc = {};
    sc.g = walk_grid(gr, edge, edge, center);
    sc.probe = probe; sc.slack = slack; sc.G = G;
    sf->sc = sc;
    sf->set_grid(m->device, sc.g, gr.max_cell, thr);
    // the ligand in blocks of 64 neighbours; both chains' per-atom arrays in their device order
    const LigandBlocks lb = build_ligand_blocks(Al, lig_atoms, gl.lo, edge, sc.g.center);
    if (!lb.finite) { delete sf; return bad(DFM_E_INVALID, "lig_atoms / center: the ligand's extent about the centre overflows fp32"); }
    const std::vector<float> rec4 = gather4(gr.order, rec_atoms, rec_radius), lig4 = gather4(lb.index, lig_atoms, lig_radius);
    std::vector<int32_t> rec_class((size_t)Ar), lig_class((size_t)Al);
    std::vector<uint64_t> rexp_s((size_t)Ar * G), lexp_s((size_t)Al * G);
    for (int q = 0; q < Ar; ++q) {
        const int32_t src = gr.order[(size_t)q];
        rec_class[(size_t)q] = class_of(rec_radius[src]);
        for (int g = 0; g < G; ++g) rexp_s[(size_t)q * G + g] = rexp[(size_t)src * G + g];
    }
    for (int q = 0; q < Al; ++q) {
        const int32_t src = lb.index[(size_t)q];
        lig_class[(size_t)q] = class_of(lig_radius[src]);
        for (int g = 0; g < G; ++g) lexp_s[(size_t)q * G + g] = lexp[(size_t)src * G + g];
    }
    return pose_finish_create(sf, "dfm_surface_create", bad, [&](PoseUploads &up) {
        up(&sf->rec, rec4)(&sf->cell_start, gr.start)(&sf->rec_index, gr.order)(&sf->rec_class, rec_class)(&sf->rec_exp, rexp_s);
        up(&sf->lig, lig4)(&sf->sphere, lb.sphere)(&sf->lig_index, lb.index)(&sf->lig_class, lig_class)(&sf->lig_exp, lexp_s)(&sf->dirs, dirs);
    });
}

extern "C" int dfm_surface_info(const dfm_surface *s, double *sasa_rec, double *sasa_lig, int32_t *rec_exposed, int32_t *lig_exposed,
                                int32_t *n_classes, float *class_radius, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge)
{
    if (!s) return fail(DFM_E_INVALID, "NULL argument");
    if (sasa_rec) *sasa_rec = s->sasa[0];
    if (sasa_lig) *sasa_lig = s->sasa[1];
    if (rec_exposed) std::memcpy(rec_exposed, s->exposed[0].data(), (size_t)s->Ar * sizeof(int32_t));
    if (lig_exposed) std::memcpy(lig_exposed, s->exposed[1].data(), (size_t)s->Al * sizeof(int32_t));
    if (n_classes) *n_classes = s->n_classes;
    if (class_radius) std::memcpy(class_radius, s->class_radius, sizeof(s->class_radius));
    s->grid_info(n_cells, max_cell_atoms, cell_edge);
    return DFM_OK;
}

extern "C" int dfm_pose_bsa_chunked(dfm_surface *sf, int P, const float *rot, const float *tr, int chunk_poses, dfm_bsa_out *out)
{
    PoseChunks ch;
    if (int rc = ch.begin(sf, "s", P, 0, rot, tr, out, chunk_poses)) return rc;
    PoseCall &c = ch.c;
    const size_t Ar = (size_t)sf->Ar, Al = (size_t)sf->Al, G = (size_t)sf->sc.G;
    // the call's chunk, else the creator's, else as many poses as fill SURFACE_CHUNK_BYTES of masks and per-atom output
    const size_t per_pose = Ar * G * sizeof(uint64_t) + (out->lig_buried ? Al * sizeof(int32_t) : 0) + (out->rec_buried ? Ar * sizeof(int32_t) : 0);
    const int fill = (int)std::min<size_t>(STERICS_MAX_CHUNK, std::max<size_t>(1, SURFACE_CHUNK_BYTES / per_pose));
    if (int rc = ch.alloc(chunk_poses > 0 ? chunk_poses : sf->chunk_poses, fill, STERICS_MAX_CHUNK)) return rc;
    const int Pc = ch.Pc;
    int32_t *d_cls = nullptr, *d_lb = nullptr, *d_rb = nullptr;
    uint64_t *d_mask = nullptr;
    HIPCHK(c.tmp.alloc(&d_cls, (size_t)Pc * 32));
    HIPCHK(c.tmp.alloc(&d_mask, (size_t)Pc * Ar * G));
    if (out->lig_buried) HIPCHK(c.tmp.alloc(&d_lb, (size_t)Pc * Al));
    if (out->rec_buried) HIPCHK(c.tmp.alloc(&d_rb, (size_t)Pc * Ar));
    const SurfaceAtoms at = {sf->rec, sf->lig, sf->sphere, sf->dirs, sf->cell_start, sf->rec_index, sf->lig_index, sf->rec_class, sf->lig_class,
                             sf->rec_exp, sf->lig_exp, sf->sc, sf->Ar, sf->Al};
    std::vector<int32_t> h_cls((size_t)Pc * 32);
    double area[16] = {};
    for (int k = 0; k < sf->n_classes; ++k) {
        const double R = (double)sf->class_radius[k] + (double)sf->probe;
        area[k] = 4.0 * M_PI * R * R / sf->K;
    }
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.upload(p0, n));
        HIPCHK(hipMemsetAsync(d_mask, 0, (size_t)n * Ar * G * sizeof(uint64_t), c.s));
        if (d_lb) HIPCHK(hipMemsetAsync(d_lb, 0, (size_t)n * Al * sizeof(int32_t), c.s));
        HIPCHK(launch_surface_pose(ch.d_rot, ch.d_tr, n, ch.T, d_cls, c.s));
        HIPCHK(launch_surface(at, ch.T, n, d_mask, d_lb, d_rb, d_cls, c.s));
        HIPCHK(ch.kernels_done());
        HIPCHK(hipMemcpyAsync(h_cls.data(), d_cls, (size_t)n * 32 * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_lb) HIPCHK(hipMemcpyAsync(out->lig_buried + (size_t)p0 * Al, d_lb, (size_t)n * Al * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_rb) HIPCHK(hipMemcpyAsync(out->rec_buried + (size_t)p0 * Ar, d_rb, (size_t)n * Ar * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
        for (int p = 0; p < n; ++p) {
            const int32_t *cp = h_cls.data() + (size_t)p * 32;
            int32_t side[2] = {0, 0};
            double s = 0.0;
            for (int ch = 0; ch < 2; ++ch)
                for (int k = 0; k < sf->n_classes; ++k) {
                    side[ch] += cp[ch * 16 + k];
                    s = s + (double)cp[ch * 16 + k] * area[k];
                }
            if (out->rec_points) out->rec_points[p0 + p] = side[0];
            if (out->lig_points) out->lig_points[p0 + p] = side[1];
            if (out->class_points) std::memcpy(out->class_points + (size_t)(p0 + p) * 32, cp, 32 * sizeof(int32_t));
            if (out->bsa) out->bsa[p0 + p] = s;
        }
    }
    return ch.done(MS_BSA);
}

extern "C" int dfm_pose_bsa(dfm_surface *s, int P, const float *rot, const float *tr, dfm_bsa_out *out)
{
    return dfm_pose_bsa_chunked(s, P, rot, tr, 0, out);
}

DFM_LAST_TIMING(dfm_bsa_last_timing, MS_BSA)

// ------------------------------------------------------------------------------------------------
// Interface energy (kernels_iface.hip): the receptor's grid of cells of the cutoff, each atom's (rmin_half, sqrt_eps, charge) at its
// sorted place.
constexpr size_t IFACE_CHUNK_BYTES = (size_t)64 << 20;      // per-atom output of one chunk of a call
constexpr int IFACE_MAX_CHUNK = 32768;                      // poses per launch (gridDim.y)

struct dfm_iface : PoseHandle {
    int Ar = 0, Al = 0;
    double sum_bound = 0.0;
    float *rec_par = nullptr, *lig_par = nullptr;
    int32_t *lig_index = nullptr;
    IfaceConst sc = {};
};

extern "C" void dfm_iface_destroy(dfm_iface *h) { pose_destroy(h); }

extern "C" dfm_iface *dfm_iface_create(dfm_model *m, int Ar, const float *rec_atoms, const float *rec_rmin_half, const float *rec_sqrt_eps,
                                       const float *rec_charge, int Al, const float *lig_atoms, const float *lig_rmin_half,
                                       const float *lig_sqrt_eps, const float *lig_charge, const float center[3], float cutoff, float soft,
                                       float elec_min_dist, float dielectric_slope)
{
    auto bad = [](int code, const std::string &msg) -> dfm_iface * { (void)fail(code, msg); return nullptr; };
    if (!m) return bad(DFM_E_INVALID, "m is NULL");
    if (const std::string msg = check_atom_sets(Ar, rec_atoms, Al, lig_atoms, center); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_iface_atoms("rec", Ar, rec_rmin_half, rec_sqrt_eps, rec_charge); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_iface_atoms("lig", Al, lig_rmin_half, lig_sqrt_eps, lig_charge); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_iface_scalars(cutoff, soft, elec_min_dist, dielectric_slope); !msg.empty()) return bad(DFM_E_INVALID, msg);
    PoseFrame f;
    const std::string frame_msg = build_pose_frame(Ar, rec_atoms, Al, lig_atoms, center, cutoff, "cutoff", f);
    if (f.gr.order.empty()) return bad(DFM_E_INVALID, frame_msg);      // no grid: the bound below needs its fullest cell
    const IfaceBound bound = iface_sum_bound(Ar, rec_sqrt_eps, rec_charge, Al, lig_sqrt_eps, lig_charge, f.gr.max_cell, soft, elec_min_dist,
                                             dielectric_slope);
    if (!bound.ok) {
        char buf[160];
        snprintf(buf, sizeof(buf), "the energy sums could reach 2^62 quanta: %.3g pairs of at most %.3g kcal/mol", bound.pairs, bound.term_kcal);
        return bad(DFM_E_INVALID, buf);
    }
    if (!frame_msg.empty()) return bad(DFM_E_INVALID, frame_msg);
    const std::vector<float> rec4 = gather4(f.gr.order, rec_atoms, nullptr), lig4 = gather4(f.lb.index, lig_atoms, nullptr);
    const std::vector<float> recp = gather_iface(f.gr.order, rec_rmin_half, rec_sqrt_eps, rec_charge);
    const std::vector<float> ligp = gather_iface(f.lb.index, lig_rmin_half, lig_sqrt_eps, lig_charge);
    dfm_iface *h = new dfm_iface;
    h->set_grid(m->device, f.g, f.gr.max_cell, cutoff);
    h->Ar = Ar; h->Al = Al;
    h->sc.g = f.g;
    h->sc.cut2 = (double)cutoff * (double)cutoff;
    h->sc.soft = (double)soft;
    h->sc.min2 = (double)elec_min_dist * (double)elec_min_dist;
    h->sc.kc = 332.0637 / (double)dielectric_slope;
    h->sc.reject2 = f.reject2;
    h->sum_bound = bound.sum_quanta;
    h->default_chunk = (int)std::min<size_t>(IFACE_MAX_CHUNK, std::max<size_t>(1, IFACE_CHUNK_BYTES / ((size_t)Al * 2 * sizeof(int64_t))));
    return pose_finish_create(h, "dfm_iface_create", bad, [&](PoseUploads &up) {
        up(&h->rec, rec4)(&h->rec_par, recp)(&h->cell_start, f.gr.start)(&h->lig, lig4)(&h->lig_par, ligp)(&h->sphere, f.lb.sphere)(&h->lig_index, f.lb.index);
    });
}

extern "C" int dfm_iface_info(const dfm_iface *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, double *sum_bound_q)
{
    if (!h) return fail(DFM_E_INVALID, "NULL argument");
    h->grid_info(n_cells, max_cell_atoms, cell_edge);
    if (sum_bound_q) *sum_bound_q = h->sum_bound;
    return DFM_OK;
}

extern "C" int dfm_pose_iface_energy_chunked(dfm_iface *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_iface_out *out)
{
    PoseChunks ch;
    if (int rc = ch.begin(h, "h", P, 0, rot, tr, out, chunk_poses)) return rc;
    PoseCall &c = ch.c;
    const bool per_atom = out->lig_vdw_q || out->lig_elec_q;
    // the call's chunk, else the default: without per-atom output a chunk is bounded by the launch alone
    if (int rc = ch.alloc(chunk_poses, per_atom ? h->default_chunk : IFACE_MAX_CHUNK, IFACE_MAX_CHUNK)) return rc;
    const int Pc = ch.Pc;
    const size_t Al = (size_t)h->Al;
    int64_t *d_tot = nullptr, *d_lv = nullptr, *d_le = nullptr;
    HIPCHK(c.tmp.alloc(&d_tot, (size_t)Pc * 4));      // rep_q | att_q | elec_q | n_pairs of each pose
    if (out->lig_vdw_q) HIPCHK(c.tmp.alloc(&d_lv, (size_t)Pc * Al));
    if (out->lig_elec_q) HIPCHK(c.tmp.alloc(&d_le, (size_t)Pc * Al));
    const IfaceAtoms at = {h->rec, h->rec_par, h->lig, h->lig_par, h->sphere, h->cell_start, h->lig_index, h->sc, h->Ar, h->Al};
    std::vector<int64_t> h_tot((size_t)Pc * 4);
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.upload(p0, n));
        if (d_lv) HIPCHK(hipMemsetAsync(d_lv, 0, (size_t)n * Al * sizeof(int64_t), c.s));
        if (d_le) HIPCHK(hipMemsetAsync(d_le, 0, (size_t)n * Al * sizeof(int64_t), c.s));
        HIPCHK(launch_iface_pose(ch.d_rot, ch.d_tr, n, ch.T, d_tot, c.s));
        HIPCHK(launch_iface(at, ch.T, n, d_tot, d_lv, d_le, c.s));
        HIPCHK(ch.kernels_done());
        HIPCHK(hipMemcpyAsync(h_tot.data(), d_tot, (size_t)n * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (d_lv) HIPCHK(hipMemcpyAsync(out->lig_vdw_q + (size_t)p0 * Al, d_lv, (size_t)n * Al * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (d_le) HIPCHK(hipMemcpyAsync(out->lig_elec_q + (size_t)p0 * Al, d_le, (size_t)n * Al * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
        for (int p = 0; p < n; ++p) {
            if (out->rep_q) out->rep_q[p0 + p] = h_tot[(size_t)p * 4];
            if (out->att_q) out->att_q[p0 + p] = h_tot[(size_t)p * 4 + 1];
            if (out->elec_q) out->elec_q[p0 + p] = h_tot[(size_t)p * 4 + 2];
            if (out->n_pairs) out->n_pairs[p0 + p] = h_tot[(size_t)p * 4 + 3];
        }
    }
    return ch.done(MS_IFACE);
}

extern "C" int dfm_pose_iface_energy(dfm_iface *h, int P, const float *rot, const float *tr, dfm_iface_out *out)
{
    return dfm_pose_iface_energy_chunked(h, P, rot, tr, 0, out);
}

DFM_LAST_TIMING(dfm_iface_last_timing, MS_IFACE)

// ------------------------------------------------------------------------------------------------
// Residue contacts (kernels_rescon.hip): the receptor's grid of cells of the cutoff, each atom's residue index in its float4, the
// receptor's class masks; every call also owns its bitmap.
struct dfm_rescon : PoseHandle {
    int Ar = 0, Al = 0, Rr = 0, Lr = 0, W = 0;
    int32_t *lig_class = nullptr;
    uint32_t *class_mask = nullptr;
    ResconConst sc = {};
};

extern "C" void dfm_rescon_destroy(dfm_rescon *h) { pose_destroy(h); }

extern "C" dfm_rescon *dfm_rescon_create(dfm_model *m, int Ar, const float *rec_atoms, const int32_t *rec_res, int Rr, const uint8_t *rec_class,
                                         int Al, const float *lig_atoms, const int32_t *lig_res, int Lr, const uint8_t *lig_class,
                                         const float center[3], float cutoff)
{
    auto bad = [](int code, const std::string &msg) -> dfm_rescon * { (void)fail(code, msg); return nullptr; };
    if (!m) return bad(DFM_E_INVALID, "m is NULL");
    if (const std::string msg = check_atom_sets(Ar, rec_atoms, Al, lig_atoms, center); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_rescon_chain("rec", Ar, rec_res, Rr, rec_class); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_rescon_chain("lig", Al, lig_res, Lr, lig_class); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_rescon_cutoff(cutoff); !msg.empty()) return bad(DFM_E_INVALID, msg);
    PoseFrame f;
    if (const std::string msg = build_pose_frame(Ar, rec_atoms, Al, lig_atoms, center, cutoff, "cutoff", f); !msg.empty()) return bad(DFM_E_INVALID, msg);
    const std::vector<float> rec4 = gather4_res(f.gr.order, rec_atoms, rec_res), lig4 = gather4_res(f.lb.index, lig_atoms, lig_res);
    const std::vector<uint32_t> masks = rescon_class_masks(Rr, rec_class);
    const std::vector<int32_t> lcls(lig_class, lig_class + Lr);
    dfm_rescon *h = new dfm_rescon;
    h->set_grid(m->device, f.g, f.gr.max_cell, cutoff);
    h->Ar = Ar; h->Al = Al; h->Rr = Rr; h->Lr = Lr; h->W = rescon_words(Rr);
    h->sc.g = f.g;
    h->sc.cutoff = (double)cutoff;
    h->sc.reject2 = f.reject2;
    h->default_chunk = rescon_chunk_poses(Lr, Rr);
    return pose_finish_create(h, "dfm_rescon_create", bad, [&](PoseUploads &up) {
        up(&h->rec, rec4)(&h->cell_start, f.gr.start)(&h->lig, lig4)(&h->sphere, f.lb.sphere)(&h->class_mask, masks)(&h->lig_class, lcls);
    });
}

extern "C" int dfm_rescon_info(const dfm_rescon *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, int32_t *row_words,
                               int32_t *chunk_poses)
{
    if (!h) return fail(DFM_E_INVALID, "NULL argument");
    h->grid_info(n_cells, max_cell_atoms, cell_edge);
    if (row_words) *row_words = h->W;
    if (chunk_poses) *chunk_poses = h->default_chunk;
    return DFM_OK;
}

extern "C" int dfm_pose_rescon_chunked(dfm_rescon *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_rescon_out *out)
{
    PoseChunks ch;
    if (int rc = ch.begin(h, "h", P, RESCON_MAX_POSES, rot, tr, out, chunk_poses)) return rc;
    PoseCall &c = ch.c;
    // the call's chunk, else as many poses as fill RESCON_SCRATCH_BYTES of bitmap
    if (int rc = ch.alloc(chunk_poses, h->default_chunk, RESCON_MAX_CHUNK)) return rc;
    const int Pc = ch.Pc;
    const size_t Rr = (size_t)h->Rr, Lr = (size_t)h->Lr, row = Lr * (size_t)h->W;
    uint32_t *d_bits = nullptr;
    int32_t *d_tot = nullptr, *d_rd = nullptr, *d_ld = nullptr;
    HIPCHK(c.tmp.alloc(&d_bits, (size_t)Pc * row));
    HIPCHK(c.tmp.alloc(&d_tot, (size_t)Pc * 9));
    if (out->rec_degree) HIPCHK(c.tmp.alloc(&d_rd, (size_t)Pc * Rr));
    if (out->lig_degree) HIPCHK(c.tmp.alloc(&d_ld, (size_t)Pc * Lr));
    const ResconAtoms at = {h->rec, h->lig, h->sphere, h->cell_start, h->lig_class, h->class_mask, h->sc, h->Ar, h->Al, h->Rr, h->Lr, h->W};
    std::vector<int32_t> h_tot((size_t)Pc * 9);
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.upload(p0, n));
        HIPCHK(hipMemsetAsync(d_bits, 0, (size_t)n * row * sizeof(uint32_t), c.s));
        HIPCHK(ch.mark_zeroed());
        HIPCHK(launch_rescon_pose(ch.d_rot, ch.d_tr, n, ch.T, c.s));
        HIPCHK(launch_rescon(at, ch.T, n, d_bits, c.s));
        HIPCHK(ch.mark_walked());
        HIPCHK(launch_rescon_finish(at, d_bits, n, d_tot, d_rd, d_ld, c.s));
        HIPCHK(ch.kernels_done());
        HIPCHK(hipMemcpyAsync(h_tot.data(), d_tot, (size_t)n * 9 * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_rd) HIPCHK(hipMemcpyAsync(out->rec_degree + (size_t)p0 * Rr, d_rd, (size_t)n * Rr * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_ld) HIPCHK(hipMemcpyAsync(out->lig_degree + (size_t)p0 * Lr, d_ld, (size_t)n * Lr * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (out->contact_bits)
            HIPCHK(hipMemcpyAsync(out->contact_bits + (size_t)p0 * row, d_bits, (size_t)n * row * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
        for (int p = 0; p < n; ++p) {
            const int32_t *t = h_tot.data() + (size_t)p * 9;
            if (out->ic) std::memcpy(out->ic + (size_t)(p0 + p) * 6, t, 6 * sizeof(int32_t));
            if (out->n_pairs) out->n_pairs[p0 + p] = t[6];
            if (out->n_rec_res) out->n_rec_res[p0 + p] = t[7];
            if (out->n_lig_res) out->n_lig_res[p0 + p] = t[8];
        }
    }
    return ch.done(MS_RESCON);
}

extern "C" int dfm_pose_rescon(dfm_rescon *h, int P, const float *rot, const float *tr, dfm_rescon_out *out)
{
    return dfm_pose_rescon_chunked(h, P, rot, tr, 0, out);
}

DFM_LAST_TIMING(dfm_rescon_last_timing, MS_RESCON)

// zeroing the bitmap, k_rescon_pose + k_rescon, k_rescon_finish of this thread's last dfm_pose_rescon, summed over its chunks
extern "C" int dfm_rescon_last_phases(double *zero_ms, double *walk_ms, double *finish_ms)
{
    return last_phases(MS_RESCON, zero_ms, walk_ms, finish_ms);
}

// ------------------------------------------------------------------------------------------------
// Hydrogen bonds and salt bridges (kernels_hbond.hip).  The atoms are the POLAR atoms of the two chains: the receptor's grid of cells of
// the larger cutoff with each atom's antecedent beside it, each atom's role and charged-residue number in its float4; every call also
// owns its bitmap.
struct dfm_hbond : PoseHandle {
    int Nr = 0, Nl = 0, Rc = 0, Lc = 0, Wc = 0;
    float *rec_ante = nullptr, *lig_ante = nullptr;
    int32_t *rec_index = nullptr, *lig_index = nullptr;
    HbondConst sc = {};
};

extern "C" void dfm_hbond_destroy(dfm_hbond *h) { pose_destroy(h); }

extern "C" dfm_hbond *dfm_hbond_create(dfm_model *m, int Nr, const float *rec_xyz, const float *rec_ante, const uint8_t *rec_role,
                                       const int32_t *rec_res, int n_rec_res, int Nl, const float *lig_xyz, const float *lig_ante,
                                       const uint8_t *lig_role, const int32_t *lig_res, int n_lig_res, const float center[3], float hb_cutoff,
                                       double min_cos2, float salt_cutoff, int *status)
{
    auto bad = [status](int code, const std::string &msg) -> dfm_hbond * {
        (void)fail(code, msg);
        if (status) *status = code;
        return nullptr;
    };
    if (status) *status = DFM_OK;
    if (!m) return bad(DFM_E_INVALID, "m is NULL");
    if (const std::string msg = check_atom_sets(Nr, rec_xyz, Nl, lig_xyz, center); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_hbond_chain("rec", Nr, rec_ante, rec_role, rec_res, n_rec_res); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_hbond_chain("lig", Nl, lig_ante, lig_role, lig_res, n_lig_res); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_hbond_scalars(hb_cutoff, min_cos2, salt_cutoff); !msg.empty()) return bad(DFM_E_INVALID, msg);
    const float reach = std::max(hb_cutoff, salt_cutoff);
    PoseFrame f;
    if (const std::string msg = build_pose_frame(Nr, rec_xyz, Nl, lig_xyz, center, reach, "larger cutoff", f, "lig_xyz"); !msg.empty())
        return bad(DFM_E_INVALID, msg);
    std::vector<int32_t> rcomp, lcomp;
    const int Rc = hbond_charged_residues(Nr, rec_role, rec_res, n_rec_res, rcomp);
    const int Lc = hbond_charged_residues(Nl, lig_role, lig_res, n_lig_res, lcomp);
    const std::vector<float> rec4 = gather4_hbond(f.gr.order, rec_xyz, rec_role, rec_res, rcomp), ra4 = gather4(f.gr.order, rec_ante, nullptr);
    const std::vector<float> lig4 = gather4_hbond(f.lb.index, lig_xyz, lig_role, lig_res, lcomp), la4 = gather4(f.lb.index, lig_ante, nullptr);
    dfm_hbond *h = new dfm_hbond;
    h->set_grid(m->device, f.g, f.gr.max_cell, reach);
    h->Nr = Nr; h->Nl = Nl; h->Rc = Rc; h->Lc = Lc; h->Wc = rescon_words(Rc);
    h->sc.g = f.g;
    h->sc.hb2 = (double)hb_cutoff * (double)hb_cutoff;
    h->sc.salt2 = (double)salt_cutoff * (double)salt_cutoff;
    h->sc.c2 = min_cos2;
    h->sc.reject2 = f.reject2;
    h->default_chunk = hbond_chunk_poses(Lc, Rc);
    return pose_finish_create(h, "dfm_hbond_create", bad, [&](PoseUploads &up) {
        up(&h->rec, rec4)(&h->rec_ante, ra4)(&h->cell_start, f.gr.start)(&h->rec_index, f.gr.order);
        up(&h->lig, lig4)(&h->lig_ante, la4)(&h->lig_index, f.lb.index)(&h->sphere, f.lb.sphere);
    });
}

extern "C" int dfm_hbond_info(const dfm_hbond *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, int32_t *n_rec_charged,
                              int32_t *n_lig_charged, int32_t *chunk_poses)
{
    if (!h) return fail(DFM_E_INVALID, "NULL argument");
    h->grid_info(n_cells, max_cell_atoms, cell_edge);
    if (n_rec_charged) *n_rec_charged = h->Rc;
    if (n_lig_charged) *n_lig_charged = h->Lc;
    if (chunk_poses) *chunk_poses = h->default_chunk;
    return DFM_OK;
}

extern "C" int dfm_pose_hbonds_chunked(dfm_hbond *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_hbond_out *out)
{
    PoseChunks ch;
    if (int rc = ch.begin(h, "h", P, HBOND_MAX_POSES, rot, tr, out, chunk_poses)) return rc;
    PoseCall &c = ch.c;
    // the call's chunk, else as many poses as fill RESCON_SCRATCH_BYTES of bitmap
    if (int rc = ch.alloc(chunk_poses, h->default_chunk, RESCON_MAX_CHUNK)) return rc;
    const int Pc = ch.Pc;
    const size_t Nr = (size_t)h->Nr, Nl = (size_t)h->Nl, words = (size_t)h->Lc * (size_t)h->Wc;
    uint32_t *d_bits = nullptr;
    int32_t *d_tot = nullptr;
    // the per-atom outputs asked for, in one block so that one memset zeroes them: rec_hb, rec_sb [Pc][Nr], lig_hb, lig_sb [Pc][Nl]
    int32_t *d_atom = nullptr, *d_rh = nullptr, *d_rs = nullptr, *d_lh = nullptr, *d_ls = nullptr;
    const size_t n_atom = (size_t)Pc * ((out->rec_hb ? Nr : 0) + (out->rec_sb ? Nr : 0) + (out->lig_hb ? Nl : 0) + (out->lig_sb ? Nl : 0));
    HIPCHK(c.tmp.alloc(&d_bits, std::max<size_t>(1, (size_t)Pc * words)));      // never empty: the kernel forms a row pointer into it
    HIPCHK(c.tmp.alloc(&d_tot, (size_t)Pc * 5));
    if (n_atom) {
        HIPCHK(c.tmp.alloc(&d_atom, n_atom));
        int32_t *q = d_atom;
        if (out->rec_hb) { d_rh = q; q += (size_t)Pc * Nr; }
        if (out->rec_sb) { d_rs = q; q += (size_t)Pc * Nr; }
        if (out->lig_hb) { d_lh = q; q += (size_t)Pc * Nl; }
        if (out->lig_sb) { d_ls = q; q += (size_t)Pc * Nl; }
    }
    const HbondAtoms at = {h->rec, h->rec_ante, h->lig, h->lig_ante, h->sphere, h->cell_start, h->rec_index, h->lig_index, h->sc,
                           h->Nr, h->Nl, h->Rc, h->Lc, h->Wc};
    std::vector<int32_t> h_tot((size_t)Pc * 5);
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.upload(p0, n));
        if (words) HIPCHK(hipMemsetAsync(d_bits, 0, (size_t)n * words * sizeof(uint32_t), c.s));
        if (n_atom) HIPCHK(hipMemsetAsync(d_atom, 0, n_atom * sizeof(int32_t), c.s));
        HIPCHK(ch.mark_zeroed());
        HIPCHK(launch_hbond_pose(ch.d_rot, ch.d_tr, n, ch.T, d_tot, c.s));
        HIPCHK(launch_hbond(at, ch.T, n, d_tot, d_bits, d_rh, d_rs, d_lh, d_ls, c.s));
        HIPCHK(ch.mark_walked());
        HIPCHK(launch_hbond_finish(at, d_bits, n, d_tot, c.s));
        HIPCHK(ch.kernels_done());
        HIPCHK(hipMemcpyAsync(h_tot.data(), d_tot, (size_t)n * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_rh) HIPCHK(hipMemcpyAsync(out->rec_hb + (size_t)p0 * Nr, d_rh, (size_t)n * Nr * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_rs) HIPCHK(hipMemcpyAsync(out->rec_sb + (size_t)p0 * Nr, d_rs, (size_t)n * Nr * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_lh) HIPCHK(hipMemcpyAsync(out->lig_hb + (size_t)p0 * Nl, d_lh, (size_t)n * Nl * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (d_ls) HIPCHK(hipMemcpyAsync(out->lig_sb + (size_t)p0 * Nl, d_ls, (size_t)n * Nl * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
        for (int p = 0; p < n; ++p) {
            const int32_t *t = h_tot.data() + (size_t)p * 5;
            if (out->n_hbond) out->n_hbond[p0 + p] = (t[0] + t[1]) + t[2];
            if (out->hb_kind) std::memcpy(out->hb_kind + (size_t)(p0 + p) * 3, t, 3 * sizeof(int32_t));
            if (out->n_salt_atoms) out->n_salt_atoms[p0 + p] = t[3];
            if (out->n_salt) out->n_salt[p0 + p] = t[4];
        }
    }
    return ch.done(MS_HBOND);
}

extern "C" int dfm_pose_hbonds(dfm_hbond *h, int P, const float *rot, const float *tr, dfm_hbond_out *out)
{
    return dfm_pose_hbonds_chunked(h, P, rot, tr, 0, out);
}

DFM_LAST_TIMING(dfm_hbond_last_timing, MS_HBOND)

// the memsets, k_hbond_pose + k_hbond, k_hbond_finish of this thread's last dfm_pose_hbonds, summed over its chunks
extern "C" int dfm_hbond_last_phases(double *zero_ms, double *walk_ms, double *finish_ms)
{
    return last_phases(MS_HBOND, zero_ms, walk_ms, finish_ms);
}

// ------------------------------------------------------------------------------------------------
// Tabulated pair potential (kernels_pairpot.hip): the receptor's grid of cells of the last bin edge, each receptor atom's type and slab
// offset beside it, the ligand's types at their sorted places, the squared edges and the quantised table in (receptor type, ligand
// type, bin) order.
// dfm_pairpot_create refuses in this order: m; the atom sets (check_atom_sets); rec_type / lig_type NULL; T; NB and the edges
// (check_pairpot_edges); the table (check_pairpot_table); a type out of range, receptor first; chunk_poses; the receptor's box of more
// than 2^24 cells; the pair bound; the ligand's extent about the centre.
struct dfm_pairpot : PoseHandle {
    int Ar = 0, Al = 0, T = 0, NB = 0;
    int chunk_poses = 0;      // the creator's chunk (0: none given)
    double pair_bound = 0.0;
    float *rec_par = nullptr;
    int32_t *lig_index = nullptr, *lig_type = nullptr, *table_q = nullptr;
    double *e2 = nullptr;
    PairpotConst sc = {};
};

extern "C" void dfm_pairpot_destroy(dfm_pairpot *h) { pose_destroy(h); }

extern "C" dfm_pairpot *dfm_pairpot_create(dfm_model *m, int Ar, const float *rec_atoms, const int32_t *rec_type, int Al, const float *lig_atoms,
                                           const int32_t *lig_type, const float center[3], int T, int NB, const float *edges,
                                           const float *table, int chunk_poses)
{
    auto bad = [](int code, const std::string &msg) -> dfm_pairpot * { (void)fail(code, msg); return nullptr; };
    if (!m) return bad(DFM_E_INVALID, "m is NULL");
    if (const std::string msg = check_atom_sets(Ar, rec_atoms, Al, lig_atoms, center); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (!rec_type) return bad(DFM_E_INVALID, "rec_type is NULL");
    if (!lig_type) return bad(DFM_E_INVALID, "lig_type is NULL");
    if (T < 1 || T > PAIRPOT_MAX_TYPES) return bad(DFM_E_INVALID, "need 1 <= T <= " + std::to_string(PAIRPOT_MAX_TYPES));
    if (const std::string msg = check_pairpot_edges(NB, edges); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_pairpot_table(T, NB, table); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_pairpot_types("rec", Ar, rec_type, T); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_pairpot_types("lig", Al, lig_type, T); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (chunk_poses < 0) return bad(DFM_E_INVALID, "chunk_poses must be >= 0");
    const float cutoff = edges[NB];
    PoseFrame f;
    const std::string frame_msg = build_pose_frame(Ar, rec_atoms, Al, lig_atoms, center, cutoff, "last edge", f);
    if (f.gr.order.empty()) return bad(DFM_E_INVALID, frame_msg);      // no grid: the bound below needs its fullest cell
    const PairpotBound bound = pairpot_pair_bound(Ar, Al, f.gr.max_cell);
    if (!bound.ok) {
        char buf[160];
        snprintf(buf, sizeof(buf), "a pose could have %.4g atom pairs in range, more than 2^31 - 1", bound.pairs);
        return bad(DFM_E_INVALID, buf);
    }
    if (!frame_msg.empty()) return bad(DFM_E_INVALID, frame_msg);
    const std::vector<float> rec4 = gather4(f.gr.order, rec_atoms, nullptr), lig4 = gather4(f.lb.index, lig_atoms, nullptr);
    const std::vector<float> recp = gather4_pairpot(f.gr.order, rec_type, T, NB);
    std::vector<int32_t> ltype((size_t)Al);
    for (int i = 0; i < Al; ++i) ltype[(size_t)i] = lig_type[f.lb.index[(size_t)i]];
    const std::vector<int32_t> tq = quantise_pairpot(T, NB, table);
    const std::vector<double> e2 = pairpot_edges2(NB, edges);
    dfm_pairpot *h = new dfm_pairpot;
    h->set_grid(m->device, f.g, f.gr.max_cell, cutoff);
    h->Ar = Ar; h->Al = Al; h->T = T; h->NB = NB;
    h->chunk_poses = chunk_poses;
    h->pair_bound = bound.pairs;
    h->sc.g = f.g;
    h->sc.lo2 = e2[0];
    h->sc.cut2 = e2[(size_t)NB];
    h->sc.reject2 = f.reject2;
    h->sc.T = T; h->sc.NB = NB;
    h->sc.top = 1;
    while (h->sc.top * 2 <= NB) h->sc.top *= 2;
    return pose_finish_create(h, "dfm_pairpot_create", bad, [&](PoseUploads &up) {
        up(&h->rec, rec4)(&h->rec_par, recp)(&h->cell_start, f.gr.start)(&h->lig, lig4)(&h->sphere, f.lb.sphere);
        up(&h->lig_index, f.lb.index)(&h->lig_type, ltype)(&h->table_q, tq)(&h->e2, e2);
    });
}

extern "C" int dfm_pairpot_info(const dfm_pairpot *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, double *pair_bound,
                                int32_t *T, int32_t *NB)
{
    if (!h) return fail(DFM_E_INVALID, "NULL argument");
    h->grid_info(n_cells, max_cell_atoms, cell_edge);
    if (pair_bound) *pair_bound = h->pair_bound;
    if (T) *T = h->T;
    if (NB) *NB = h->NB;
    return DFM_OK;
}

extern "C" int dfm_pose_pairpot_chunked(dfm_pairpot *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_pairpot_out *out)
{
    PoseChunks ch;
    if (int rc = ch.begin(h, "h", P, 0, rot, tr, out, chunk_poses)) return rc;
    PoseCall &c = ch.c;
    // the call's chunk, else the creator's, else as many poses as fill PAIRPOT_CHUNK_BYTES of counts plus per-atom output
    if (int rc = ch.alloc(chunk_poses > 0 ? chunk_poses : h->chunk_poses,
                          pairpot_chunk_poses(h->Al, h->T, h->NB, out->lig_q != nullptr, out->counts != nullptr), PAIRPOT_MAX_CHUNK))
        return rc;
    const int Pc = ch.Pc;
    const size_t Al = (size_t)h->Al, hist = (size_t)h->T * h->T * h->NB;
    int64_t *d_tot = nullptr, *d_lq = nullptr;
    int32_t *d_cnt = nullptr;
    HIPCHK(c.tmp.alloc(&d_tot, (size_t)Pc * 2));      // energy_q | n_pairs of each pose
    if (out->lig_q) HIPCHK(c.tmp.alloc(&d_lq, (size_t)Pc * Al));
    if (out->counts) HIPCHK(c.tmp.alloc(&d_cnt, (size_t)Pc * hist));
    const PairpotAtoms at = {h->rec, h->rec_par, h->lig, h->sphere, h->cell_start, h->lig_index, h->lig_type, h->table_q, h->e2, h->sc,
                             h->Ar, h->Al};
    std::vector<int64_t> h_tot((size_t)Pc * 2);
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.upload(p0, n));
        if (d_lq) HIPCHK(hipMemsetAsync(d_lq, 0, (size_t)n * Al * sizeof(int64_t), c.s));
        if (d_cnt) HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)n * hist * sizeof(int32_t), c.s));
        HIPCHK(ch.mark_zeroed());
        HIPCHK(launch_pairpot_pose(ch.d_rot, ch.d_tr, n, ch.T, d_tot, c.s));
        HIPCHK(launch_pairpot(at, ch.T, n, d_tot, d_lq, d_cnt, c.s));
        HIPCHK(ch.mark_walked());
        HIPCHK(ch.kernels_done());      // no finishing kernel: the third phase is empty
        HIPCHK(hipMemcpyAsync(h_tot.data(), d_tot, (size_t)n * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (d_lq) HIPCHK(hipMemcpyAsync(out->lig_q + (size_t)p0 * Al, d_lq, (size_t)n * Al * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (d_cnt) HIPCHK(hipMemcpyAsync(out->counts + (size_t)p0 * hist, d_cnt, (size_t)n * hist * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
        for (int p = 0; p < n; ++p) {
            if (out->energy_q) out->energy_q[p0 + p] = h_tot[(size_t)p * 2];
            if (out->n_pairs) out->n_pairs[p0 + p] = h_tot[(size_t)p * 2 + 1];
        }
    }
    return ch.done(MS_PAIRPOT);
}

extern "C" int dfm_pose_pairpot(dfm_pairpot *h, int P, const float *rot, const float *tr, dfm_pairpot_out *out)
{
    return dfm_pose_pairpot_chunked(h, P, rot, tr, 0, out);
}

DFM_LAST_TIMING(dfm_pairpot_last_timing, MS_PAIRPOT)

// the memsets of the per-atom output and of counts, k_pairpot_pose + k_pairpot, and nothing (the call has no finishing kernel) of this
// thread's last dfm_pose_pairpot, summed over its chunks
extern "C" int dfm_pairpot_last_phases(double *zero_ms, double *walk_ms, double *finish_ms)
{
    return last_phases(MS_PAIRPOT, zero_ms, walk_ms, finish_ms);
}

// ------------------------------------------------------------------------------------------------
// Density fit (kernels_density.hip): the grid as one float4 per node, the ligand's atoms with their weights in the caller's order and
// the grid's geometry as doubles.  No receptor and no cell grid: the PoseHandle's grid fields stay 0.
// The definition (dfmdock_amd/density.py is the float64 numpy statement of it).  The receptor's frame is the map's; pose p of ligand
// atom a is (a - center) R(rot_p)^T + center + tr_p in fp64, as for every other rigid-pose call.  C channels (1 to 4) of float32 on one
// orthogonal grid [nz][ny][nx], node (iz, iy, ix) at origin + (ix, iy, iz) * voxel, origin / voxel float32 (x, y, z).  One atom, one
// channel, everything widened to fp64, in this order, nothing contracted:
//   ux = (x - ox) / vx ; ix = floor(ux) ; fx = ux - ix        (same for y, z)
//   inside  iff 0 <= ux < nx-1 and 0 <= uy < ny-1 and 0 <= uz < nz-1   (NaN is outside)
//   c00 = c000 + fx*(c100 - c000) ; c10 = c010 + fx*(c110 - c010)
//   c01 = c001 + fx*(c101 - c001) ; c11 = c011 + fx*(c111 - c011)
//   c0  = c00  + fy*(c10 - c00)   ; c1  = c01  + fy*(c11 - c01)
//   val = c0   + fz*(c1 - c0)
//   term_q = int64(rint((w_a * val) * 2^20))      ties to even; 0 for an outside atom
// sum_q [P,C] = the sums of term_q, n_inside [P], n_above [P] = the inside atoms whose channel-0 val >= threshold, atom_q [P,Al] = term_q
// of channel 0.  A pose with a non-finite transform gets zeros.
// dfm_density_create refuses in this order: m; C, the axes, NULL origin / voxel / grids, a non-finite origin, a voxel outside (0, 16], a
// grid value that is not finite or above 2^10 in magnitude (check_density_grid); NULL lig_atoms / lig_w / center, Al, a non-finite atom,
// a weight that is not finite or above 2^7 in magnitude, a non-finite centre (check_density_atoms); a threshold that is not finite; the
// sum bound (density_sum_bound).
struct dfm_density : PoseHandle {
    int nx = 0, ny = 0, nz = 0, C = 0, Al = 0;
    double sum_bound = 0.0;
    float *grid = nullptr;
    double *geo = nullptr;
};

extern "C" void dfm_density_destroy(dfm_density *h) { pose_destroy(h); }

extern "C" dfm_density *dfm_density_create(dfm_model *m, int nx, int ny, int nz, const float origin[3], const float voxel[3], int C,
                                           const float *grids, int Al, const float *lig_atoms, const float *lig_w, const float center[3],
                                           float threshold, int *err)
{
    auto bad = [err](int code, const std::string &msg) -> dfm_density * {
        (void)fail(code, msg);
        if (err) *err = code;
        return nullptr;
    };
    if (err) *err = DFM_OK;
    if (!m) return bad(DFM_E_INVALID, "m is NULL");
    if (const std::string msg = check_density_grid(nx, ny, nz, origin, voxel, C, grids); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (const std::string msg = check_density_atoms(Al, lig_atoms, lig_w, center); !msg.empty()) return bad(DFM_E_INVALID, msg);
    if (!std::isfinite(threshold)) return bad(DFM_E_INVALID, "threshold is not finite");
    const DensityBound bound = density_sum_bound(Al);
    if (!bound.ok) {
        char buf[160];
        snprintf(buf, sizeof(buf), "a pose's sums could reach %.4g quanta, 2^62 or more", bound.quanta);
        return bad(DFM_E_INVALID, buf);
    }
    std::vector<float> g4, lig4;
    try {
        g4 = interleave_density(nx, ny, nz, C, grids);
        lig4 = gather4_density(Al, lig_atoms, lig_w);
    } catch (const std::bad_alloc &) {
        return bad(DFM_E_OOM, "dfm_density_create: the host copy of the grid does not fit");
    }
    const std::vector<double> geo = {(double)origin[0], (double)origin[1], (double)origin[2], (double)voxel[0], (double)voxel[1],
                                     (double)voxel[2], (double)center[0], (double)center[1], (double)center[2], (double)threshold,
                                     (double)(nx - 1), (double)(ny - 1), (double)(nz - 1), 0.0, 0.0, 0.0};
    static_assert(DENSITY_GEO_SLOTS == 16, "geo holds 16 doubles");
    dfm_density *h = new dfm_density;
    h->device = m->device;
    h->nx = nx; h->ny = ny; h->nz = nz; h->C = C; h->Al = Al;
    h->sum_bound = bound.quanta;
    return pose_finish_create(h, "dfm_density_create", bad, [&](PoseUploads &up) { up(&h->grid, g4)(&h->lig, lig4)(&h->geo, geo); });
}

extern "C" int dfm_density_info(const dfm_density *h, int32_t *nx, int32_t *ny, int32_t *nz, int32_t *C, int32_t *chunk_poses,
                                double *sum_bound)
{
    if (!h) return fail(DFM_E_INVALID, "NULL argument");
    if (nx) *nx = h->nx;
    if (ny) *ny = h->ny;
    if (nz) *nz = h->nz;
    if (C) *C = h->C;
    if (chunk_poses) *chunk_poses = density_chunk_poses(h->Al, true);
    if (sum_bound) *sum_bound = h->sum_bound;
    return DFM_OK;
}

extern "C" int dfm_pose_density_chunked(dfm_density *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_density_out *out)
{
    PoseChunks ch;
    if (int rc = ch.begin(h, "h", P, 0, rot, tr, out, chunk_poses)) return rc;
    PoseCall &c = ch.c;
    // the call's chunk, else as many poses as fill DENSITY_CHUNK_BYTES of per-atom output
    if (int rc = ch.alloc(chunk_poses, density_chunk_poses(h->Al, out->atom_q != nullptr), DENSITY_MAX_CHUNK)) return rc;
    const int Pc = ch.Pc, C = h->C;
    const size_t Al = (size_t)h->Al;
    int64_t *d_tot = nullptr, *d_aq = nullptr;
    HIPCHK(c.tmp.alloc(&d_tot, (size_t)Pc * DENSITY_TOT));
    if (out->atom_q) HIPCHK(c.tmp.alloc(&d_aq, (size_t)Pc * Al));
    const DensityAtoms at = {h->grid, h->lig, h->geo, h->nx, h->ny, h->nz, h->C, h->Al};
    std::vector<int64_t> h_tot((size_t)Pc * DENSITY_TOT);
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.upload(p0, n));
        HIPCHK(launch_density_pose(ch.d_rot, ch.d_tr, n, ch.T, d_tot, c.s));
        HIPCHK(launch_density(at, ch.T, n, d_tot, d_aq, c.s));
        HIPCHK(ch.kernels_done());
        HIPCHK(hipMemcpyAsync(h_tot.data(), d_tot, (size_t)n * DENSITY_TOT * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (d_aq) HIPCHK(hipMemcpyAsync(out->atom_q + (size_t)p0 * Al, d_aq, (size_t)n * Al * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
        for (int p = 0; p < n; ++p) {
            const int64_t *t = &h_tot[(size_t)p * DENSITY_TOT];
            if (out->sum_q)
                for (int k = 0; k < C; ++k) out->sum_q[(size_t)(p0 + p) * C + k] = t[k];
            if (out->n_inside) out->n_inside[p0 + p] = (int32_t)t[4];
            if (out->n_above) out->n_above[p0 + p] = (int32_t)t[5];
        }
    }
    return ch.done(MS_DENSITY);
}

extern "C" int dfm_pose_density(dfm_density *h, int P, const float *rot, const float *tr, dfm_density_out *out)
{
    return dfm_pose_density_chunked(h, P, rot, tr, 0, out);
}

DFM_LAST_TIMING(dfm_density_last_timing, MS_DENSITY)

// ------------------------------------------------------------------------------------------------
// Rigid pose fit (kernels_fit.hip): from decoy coordinates back to the sampler's (rot_update, tr_update).  Bound to the model handle's
// device only, like the clustering calls; the call's scaffold and chunk loop are PoseChunks', its poses are coordinates.
constexpr size_t FIT_CHUNK_BYTES = (size_t)64 << 20;      // poses uploaded and fitted per chunk of a call
constexpr int FIT_MAX_CHUNK = 1 << 20;                    // poses per launch

extern "C" int dfm_pose_fit_chunked(dfm_model *m, int P, int L, const float *lig_ref, const float *lig_pos, int R, const float *rec_ref,
                                    const float *rec_pos, const float center[3], int chunk_poses, dfm_fit_out *out)
{
    if (!m) return fail(DFM_E_INVALID, "m is NULL");
    if (!lig_ref) return fail(DFM_E_INVALID, "lig_ref is NULL");
    if (!lig_pos) return fail(DFM_E_INVALID, "lig_pos is NULL");
    if (!center) return fail(DFM_E_INVALID, "center is NULL");
    if (!out || !out->rot || !out->tr || !out->rmsd) return fail(DFM_E_INVALID, "out, out->rot, out->tr or out->rmsd is NULL");
    if (P < 1) return fail(DFM_E_INVALID, "need P >= 1");
    if (L < 1) return fail(DFM_E_INVALID, "need L >= 1");
    if ((rec_ref == nullptr) != (rec_pos == nullptr)) return fail(DFM_E_INVALID, "rec_ref and rec_pos must be given together");
    const bool with_rec = rec_ref != nullptr;
    if (with_rec && R < 1) return fail(DFM_E_INVALID, "need R >= 1 with a receptor");
    if (with_rec && !out->rec_rmsd_or_null) return fail(DFM_E_INVALID, "out->rec_rmsd_or_null is NULL with a receptor");
    if (chunk_poses < 0) return fail(DFM_E_INVALID, "chunk_poses must be >= 0");
    if ((int64_t)L * 9 > INT32_MAX / 2 || (with_rec && (int64_t)R * 9 > INT32_MAX / 2)) return fail(DFM_E_INVALID, "L or R too large");
    const int Rn = with_rec ? R : 0, chains = with_rec ? 2 : 1;
    PoseChunks ch;
    if (int rc = ch.open(m->device, P)) return rc;
    PoseCall &c = ch.c;
    const size_t lig_n = (size_t)L * 9, rec_n = (size_t)Rn * 9, per_pose = (lig_n + rec_n) * sizeof(float);
    const int by_memory = (int)std::min<size_t>(FIT_MAX_CHUNK, std::max<size_t>(1, FIT_CHUNK_BYTES / per_pose));
    const int Pc = std::min(P, chunk_poses > 0 ? std::min(chunk_poses, FIT_MAX_CHUNK) : by_memory);
    // the shift is the rotation centre itself: an fp32 triple, so p - o is exact in fp64, and tr is the shifted frame's t
    const double o[3] = {(double)center[0], (double)center[1], (double)center[2]};
    float *d_lref = nullptr, *d_rref = nullptr, *X = nullptr, *Xr = nullptr, *d_rot = nullptr, *d_tr = nullptr;
    double *sums = nullptr, *xf = nullptr, *d_rmsd = nullptr;      // d_rmsd: rmsd [Pc] | rec_rmsd [Pc]
    HIPCHK(c.tmp.upload_async(&d_lref, lig_ref, lig_n, c.s));
    if (with_rec) HIPCHK(c.tmp.upload_async(&d_rref, rec_ref, rec_n, c.s));
    HIPCHK(c.tmp.alloc(&X, (size_t)Pc * lig_n));
    if (with_rec) HIPCHK(c.tmp.alloc(&Xr, (size_t)Pc * rec_n));
    HIPCHK(c.tmp.alloc(&sums, (size_t)Pc * chains * 15));
    HIPCHK(c.tmp.alloc(&xf, (size_t)Pc * 24));
    HIPCHK(c.tmp.alloc(&d_rot, (size_t)Pc * 3));
    HIPCHK(c.tmp.alloc(&d_tr, (size_t)Pc * 3));
    HIPCHK(c.tmp.alloc(&d_rmsd, (size_t)Pc * 2));
    const FitChain lig = {X, d_lref, L}, rec = {Xr, d_rref, Rn};
    for (int p0 = 0; p0 < P; p0 += Pc) {
        const int n = std::min(Pc, P - p0);
        HIPCHK(ch.copies_begin());
        HIPCHK(hipMemcpyAsync(X, lig_pos + (size_t)p0 * lig_n, (size_t)n * lig_n * sizeof(float), hipMemcpyHostToDevice, c.s));
        if (with_rec) HIPCHK(hipMemcpyAsync(Xr, rec_pos + (size_t)p0 * rec_n, (size_t)n * rec_n * sizeof(float), hipMemcpyHostToDevice, c.s));
        HIPCHK(ch.copies_done());
        HIPCHK(launch_fit_reduce(lig, rec, n, o, sums, c.s));
        HIPCHK(launch_fit_solve(sums, L, Rn, n, xf, d_rot, d_tr, c.s));
        HIPCHK(launch_fit_resid(lig, rec, xf, n, o, d_rmsd, d_rmsd + Pc, c.s));
        HIPCHK(ch.kernels_done());
        HIPCHK(hipMemcpyAsync(out->rot + (size_t)p0 * 3, d_rot, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c.s));
        HIPCHK(hipMemcpyAsync(out->tr + (size_t)p0 * 3, d_tr, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c.s));
        HIPCHK(hipMemcpyAsync(out->rmsd + p0, d_rmsd, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.s));
        if (with_rec) HIPCHK(hipMemcpyAsync(out->rec_rmsd_or_null + p0, d_rmsd + Pc, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.s));
        HIPCHK(ch.finish());
    }
    return ch.done(MS_FIT);
}

extern "C" int dfm_pose_fit(dfm_model *m, int P, int L, const float *lig_ref, const float *lig_pos, int R, const float *rec_ref,
                            const float *rec_pos, const float center[3], dfm_fit_out *out)
{
    return dfm_pose_fit_chunked(m, P, L, lig_ref, lig_pos, R, rec_ref, rec_pos, center, 0, out);
}

DFM_LAST_TIMING(dfm_fit_last_timing, MS_FIT)
