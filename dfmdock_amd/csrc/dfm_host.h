// dfm_host.h - private host-side plumbing shared by the api_*.hip files (the engine's: dfm_engine.h) and api_pose.hip: the thread's last error, the HIP error and device-scope
// macros, the device block cache and the pools that draw on it, the allocator diagnostics, and the model handle.  The objects
// behind the `extern` declarations are defined once, in api.hip.
#pragma once

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "dfm_guardscan.h"
#include "dfm_internal.h"

namespace dfm {

extern thread_local std::string g_err;      // this thread's last error (dfm_last_error); defined in api.hip

inline int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            return fail(_e == hipErrorOutOfMemory ? DFM_E_OOM : DFM_E_HIP,                         \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                       \
        }                                                                                         \
    } while (0)

// Every handle belongs to one device (dfm_model: the device current at creation; dfm_complex: its model's).  Entry points
// run under a DeviceScope: switch to the handle's device, restore the caller's on the way out.
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};
#define DEVICE_SCOPE(dev)                                                                          \
    DeviceScope _ds(dev);                                                                          \
    if (_ds.err != hipSuccess) return fail(DFM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_ds.err))

// ------------------------------------------------------------------------------------------------
// Device blocks released by one handle and wanted by the next: a set driver creates and destroys a complex (about forty buffers, some of them
// gigabytes) every few hundred milliseconds, and hipMalloc / hipFree of that size cost milliseconds each (hipFree also drains the device).
// Released blocks are kept per device, up to a quarter of its memory, and handed out again to requests of at most twice-smaller size;
// DFM_ALLOC_CACHE=0 turns the cache off.
struct BlockCache {
    std::mutex m;
    std::multimap<size_t, void *> free_blocks[MAX_DEVICES];
    size_t bytes[MAX_DEVICES] = {};
    size_t cap[MAX_DEVICES] = {};
    static bool enabled()
    {
        static const bool on = [] { const char *e = getenv("DFM_ALLOC_CACHE"); return !(e && atoi(e) == 0); }();
        return on;
    }
    static double fraction()      // share of a device's memory the cache may park (DFM_ALLOC_CACHE_FRAC, default 0.25)
    {
        static const double f = [] {
            const char *e = getenv("DFM_ALLOC_CACHE_FRAC");
            const double v = e ? atof(e) : 0.25;
            return v < 0.0 ? 0.0 : (v > 0.9 ? 0.9 : v);
        }();
        return f;
    }
    bool give(int dev, void *p, size_t size)
    {
        std::lock_guard<std::mutex> g(m);
        if (!cap[dev]) {
            size_t fr = 0, tot = 0;
            DeviceScope ds(dev);      // the memory of the block's OWN device, whatever the calling thread's current device is
            if (ds.err != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) tot = 0;
            cap[dev] = (size_t)((double)tot * fraction()) + 1;
        }
        if (bytes[dev] + size > cap[dev]) return false;
        free_blocks[dev].emplace(size, p);
        bytes[dev] += size;
        return true;
    }
    // hand every parked block of `dev` (all devices: dev < 0) back to the driver; returns the bytes freed
    size_t trim(int dev)
    {
        std::vector<std::pair<int, void *>> drop;
        size_t freed = 0;
        {
            std::lock_guard<std::mutex> g(m);
            for (int d = 0; d < MAX_DEVICES; ++d) {
                if (dev >= 0 && d != dev) continue;
                for (auto &kv : free_blocks[d]) drop.emplace_back(d, kv.second);
                freed += bytes[d];
                free_blocks[d].clear();
                bytes[d] = 0;
            }
        }
        for (auto &dp : drop) { DeviceScope ds(dp.first); (void)hipFree(dp.second); }
        return freed;
    }
};
extern BlockCache &g_block_cache;      // defined in api.hip; never destroyed: a handle may outlive static destruction at process exit

// diagnostic: DFM_ALLOC_GUARD=<KiB> puts that many KiB of 0xA5 before and after every block (cache off) and checks them at release:
// a kernel writing outside its buffers is reported on stderr with the block's size and the first damaged offset
inline size_t guard_bytes()
{
    static const size_t g = [] { const char *e = getenv("DFM_ALLOC_GUARD"); return e ? (size_t)atoi(e) * 1024 : (size_t)0; }();
    return g;
}
inline int alloc_poison()      // DFM_ALLOC_POISON=<byte>: -1 when not set
{
    static const int poison = [] { const char *e = getenv("DFM_ALLOC_POISON"); return e ? atoi(e) & 255 : -1; }();
    return poison;
}
// what the two diagnostics did in this process (dfm_alloc_diag): blocks handed out, bytes filled with the poison byte, guard bands
// checked at release and found damaged, and the first damaged block: its size and the damaged byte's offset from the block's start
// (negative in the head band, >= size in the tail band)
struct AllocDiag {
    std::atomic<int64_t> blocks{0}, poisoned{0}, bands{0}, damaged{0}, first_size{-1}, first_off{-1};
};
extern AllocDiag g_alloc_diag;      // defined in api.hip
struct DevPool {
    struct Block { void *p; size_t size; int dev; };
    std::vector<Block> ptrs;
    hipStream_t owner = nullptr;      // bind(): the one stream that ever touches this pool's blocks
    bool bound = false;
    void bind(hipStream_t s) { owner = s; bound = true; }
    ~DevPool() { release(); }
    // `drained`: the caller has synchronised the ONE stream that ever touched these blocks (a complex handle's own stream), so
    // nothing in flight reads them and the device-wide wait - which would also wait for every OTHER handle's queued work, e.g. a
    // whole dfm_sample call of the next complex of a set run - is not needed.
    void release(bool drained = false)
    {
        if (ptrs.empty()) return;
        if (const size_t G = guard_bytes()) {
            (void)hipDeviceSynchronize();
            std::vector<unsigned char> h(G);
            for (const Block &b : ptrs) {
                unsigned char *base = reinterpret_cast<unsigned char *>(b.p) - G;
                for (int side = 0; side < 2; ++side) {
                    (void)hipMemcpy(h.data(), side ? base + G + b.size : base, G, hipMemcpyDeviceToHost);
                    const size_t k = guard_first_damaged(h.data(), G);
                    g_alloc_diag.bands.fetch_add(1, std::memory_order_relaxed);
                    if (k < G) {
                        fprintf(stderr, "DFM_ALLOC_GUARD: block of %zu bytes: %s guard damaged at offset %zu (byte 0x%02x)\n", b.size,
                                side ? "TAIL" : "HEAD", k, h[k]);
                        if (g_alloc_diag.damaged.fetch_add(1, std::memory_order_relaxed) == 0) {
                            g_alloc_diag.first_size.store((int64_t)b.size, std::memory_order_relaxed);
                            g_alloc_diag.first_off.store(side ? (int64_t)(b.size + k) : (int64_t)k - (int64_t)G, std::memory_order_relaxed);
                        }
                    }
                }
                (void)hipFree(base);
            }
            ptrs.clear();
            return;
        }
        if (BlockCache::enabled()) {
            // what hipFree would have done: nothing in flight reads these blocks when the next owner gets them (a bound pool waits
            // for its own stream only)
            if (!drained) { if (bound) (void)hipStreamSynchronize(owner); else (void)hipDeviceSynchronize(); }
            for (const Block &b : ptrs)
                if (b.dev < 0 || b.dev >= MAX_DEVICES || !g_block_cache.give(b.dev, b.p, b.size)) (void)hipFree(b.p);
        } else {
            for (const Block &b : ptrs) (void)hipFree(b.p);
        }
        ptrs.clear();
    }
    // hand back the blocks allocated after `mark` (= ptrs.size() before a group of allocations that failed half way); the caller has
    // synchronised the owning stream
    void release_tail(size_t mark)
    {
        if (mark >= ptrs.size()) return;
        std::vector<Block> tail(ptrs.begin() + mark, ptrs.end()), head(ptrs.begin(), ptrs.begin() + mark);
        ptrs.swap(tail);
        release(true);
        ptrs.swap(head);
    }
    template <typename T> hipError_t alloc(T **out, size_t n)
    {
        size_t bytes = (n ? n : 1) * sizeof(T);
        int dev = -1;
        (void)hipGetDevice(&dev);
        void *p = nullptr;
        const int poison = alloc_poison();
        if (const size_t G = guard_bytes()) {
            unsigned char *base = nullptr;
            hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), bytes + 2 * G);
            if (e != hipSuccess) return e;
            (void)hipMemset(base, GUARD_BYTE, G); (void)hipMemset(base + G + bytes, GUARD_BYTE, G);
            if (poison >= 0) {      // the payload too: a guarded block is exact-size and fresh, its contents whatever the driver left
                (void)hipMemset(base + G, poison, bytes);
                g_alloc_diag.poisoned.fetch_add((int64_t)bytes, std::memory_order_relaxed);
            }
            (void)hipDeviceSynchronize();
            ptrs.push_back({base + G, bytes, dev});
            g_alloc_diag.blocks.fetch_add(1, std::memory_order_relaxed);
            *out = reinterpret_cast<T *>(base + G);
            return hipSuccess;
        }
        if (BlockCache::enabled() && dev >= 0 && dev < MAX_DEVICES) {
            bytes = (bytes + 65535) & ~(size_t)65535;      // 64 KiB granules: neighbouring sizes share blocks
            // the block's true size travels with it: look it up by taking from the cache under the lock
            {
                std::lock_guard<std::mutex> g(g_block_cache.m);
                auto &fb = g_block_cache.free_blocks[dev];
                auto it = fb.lower_bound(bytes);
                if (it != fb.end() && it->first <= 2 * bytes + (1u << 20)) {
                    p = it->second;
                    bytes = it->first;
                    g_block_cache.bytes[dev] -= it->first;
                    fb.erase(it);
                }
            }
        }
        if (!p) {
            hipError_t e = hipMalloc(&p, bytes);
            if (e != hipSuccess && BlockCache::enabled() && dev >= 0 && dev < MAX_DEVICES) {      // out of memory with blocks parked in the cache: drop them and retry
                std::vector<void *> drop;
                {
                    std::lock_guard<std::mutex> g(g_block_cache.m);
                    for (auto &kv : g_block_cache.free_blocks[dev]) drop.push_back(kv.second);
                    g_block_cache.free_blocks[dev].clear();
                    g_block_cache.bytes[dev] = 0;
                }
                for (void *q : drop) (void)hipFree(q);
                (void)hipGetLastError();
                e = hipMalloc(&p, bytes);
            }
            if (e != hipSuccess) return e;
        }
        ptrs.push_back({p, bytes, dev});
        g_alloc_diag.blocks.fetch_add(1, std::memory_order_relaxed);
        *out = reinterpret_cast<T *>(p);
        // diagnostic: DFM_ALLOC_POISON=<byte> fills every block handed out (fresh or from the cache) with that byte - 255 = NaN
        // patterns in fp32 / fp16 - so that a kernel reading memory nobody wrote shows up as a changed or non-finite result
        if (poison >= 0) {
            // The fill is waited for, on the pool's own stream or on the null stream.  What is written into the block next need not be
            // in that stream's order - upload() copies synchronously, upload_async() on whichever (non-blocking) stream the caller
            // names, and a memset of device memory may return before it has run - and a fill that lands afterwards replaces the data:
            // the one-byte-per-residue interface flags of dfm_native_create became "every residue" that way.
            const hipStream_t fs = bound ? owner : nullptr;
            hipError_t e = hipMemsetAsync(p, poison, bytes, fs);
            if (e == hipSuccess) e = hipStreamSynchronize(fs);
            if (e != hipSuccess) return e;
            g_alloc_diag.poisoned.fetch_add((int64_t)bytes, std::memory_order_relaxed);
        }
        return hipSuccess;
    }
    template <typename T> hipError_t upload(T **out, const T *host, size_t n)
    {
        hipError_t e = alloc(out, n);
        if (e != hipSuccess) return e;
        return hipMemcpy(*out, host, n * sizeof(T), hipMemcpyHostToDevice);
    }
    // the same on a handle's own (non-blocking) stream: the caller synchronises it before `host` may change
    template <typename T> hipError_t upload_async(T **out, const T *host, size_t n, hipStream_t s)
    {
        hipError_t e = alloc(out, n);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(*out, host, n * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

}  // namespace dfm

struct dfm_model {
    dfm_hparams hp;
    int device = 0;
    dfm::DevPool pool;
    float *single_embed = nullptr;   // [256][lm]
    dfm::LayerDev layers[8];
    dfm::HeadsDev heads;
    float *en0_w = nullptr;          // [256][512]
    dfm::PairHeadDev pair[3];             // family 1: 0 to_force, 1 to_energy, 2 to_confidence
    dfm::PairHeadDev dist;                // family 1: to_dist (fp32 only; w3 = [256][64], transposed)
    float *dist_w3f = nullptr;       // family 1: to_dist.3 in the fragment order of k_pair_dist_sum (PairDistSumArgs::w3f)
    float *ir0_w = nullptr, *ir0_b = nullptr, *ir2_w = nullptr, *ir2_b = nullptr, *ir4_w = nullptr, *ir4_b = nullptr;   // to_ires
    float tab_max[8][2] = {};        // per layer: largest |entry| of the two merged lookup tables as stored (log2e-scaled; before the fp16 clamp)    // local refinement: IGSO(3) cdf tables by sigma index (k_igso3_cdf, 8 KB each in `pool`), built on first use and never changed
    std::mutex ig_m;
    std::map<int, double *> ig_tab;
};
