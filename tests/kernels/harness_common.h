// harness_common.h - the runtime every kernel-test shim (tests/kernels/*_harness.hip) shares.  Host code only.
//
// The guard-band protocol.  A call is a record of named host buffers.  Each buffer in use gets a device block of its own with GUARD
// bytes of SENTINEL (0xff: a NaN as fp32 and as fp16, -1 as an integer) before and after its interior, and the interior starts as the
// sentinel too: an element a kernel should have written and did not is as visible as a byte it wrote outside its block.  The shim fills
// the shipped argument structs with the interior pointers, calls the SHIPPED launcher on a stream of its own, and every output block
// comes back to the host WITH its guard bands (tests/kernel_harness.py checks them).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace harness {

constexpr size_t GUARD = 4096;      // bytes of sentinel on each side of a block
constexpr unsigned char SENTINEL = 0xff;

// One host buffer.  host == nullptr: the slot is unused (nullptr to the launcher).
//   out 0  input: `bytes` bytes at host are uploaded.
//   out 1  output: host holds GUARD + bytes + GUARD bytes and receives the whole device block, guards included.
//   out 2  in / out: as 1, and the interior host[GUARD .. GUARD + bytes) is uploaded first (zero where a contract says "zero it first",
//          a base where it says "added to", a marker where only some threads write).
struct HarnessBuf {
    void *host;
    long long bytes;
    int out;
};

// The device blocks of one call: construct, fill the launcher's arguments from ptr(), begin(), launch, finish().
template <int N> struct Blocks {
    const HarnessBuf *buf;
    void *dev[N] = {};
    hipStream_t s = nullptr;
    hipError_t err = hipSuccess;      // of the construction

    explicit Blocks(const HarnessBuf *b) : buf(b)
    {
        for (int i = 0; i < N; ++i)
            if (b[i].bytes < 0 || b[i].out < 0 || b[i].out > 2) { err = hipErrorInvalidValue; return; }
        for (int i = 0; i < N && err == hipSuccess; ++i) {
            if (!b[i].host) continue;
            const size_t bytes = (size_t)b[i].bytes, total = GUARD + bytes + GUARD;
            if ((err = hipMalloc(&dev[i], total)) != hipSuccess) break;
            if ((err = hipMemset(dev[i], SENTINEL, total)) != hipSuccess) break;
            if (b[i].out != 1 && bytes > 0)
                err = hipMemcpy((char *)dev[i] + GUARD, (const char *)b[i].host + (b[i].out ? GUARD : 0), bytes, hipMemcpyHostToDevice);
        }
    }
    Blocks(const Blocks &) = delete;
    Blocks &operator=(const Blocks &) = delete;
    ~Blocks()
    {
        if (s) (void)hipStreamDestroy(s);
        for (int i = 0; i < N; ++i)
            if (dev[i]) (void)hipFree(dev[i]);
    }

    // interior of block i, or nullptr for an unused slot
    void *ptr(int i) const { return dev[i] ? (char *)dev[i] + GUARD : nullptr; }

    // The stream to launch on.  The fills and uploads went through the null stream, which a non-blocking stream does not wait for:
    // without the synchronisation a kernel could write a block that is still being filled.
    hipError_t begin(hipStream_t *stream)
    {
        hipError_t e = err;
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        *stream = s;
        return e;
    }

    // Waits for the stream and returns every output block with its guards - after a success, and after a launcher's refusal
    // (hipErrorInvalidValue) too, so that a test can see the prefill untouched.  Returns the launcher's error if any, else the copy's.
    hipError_t finish(hipError_t e)
    {
        if (s) {
            const hipError_t e2 = hipStreamSynchronize(s);
            if (e == hipSuccess) e = e2;
            (void)hipStreamDestroy(s);
            s = nullptr;
        }
        hipError_t ec = hipSuccess;
        if (e == hipSuccess || e == hipErrorInvalidValue)
            for (int i = 0; i < N && ec == hipSuccess; ++i)
                if (dev[i] && buf[i].out)
                    ec = hipMemcpy(buf[i].host, dev[i], GUARD + (size_t)buf[i].bytes + GUARD, hipMemcpyDeviceToHost);
        return e != hipSuccess ? e : ec;
    }
};

}  // namespace harness

// the three exports every shim has next to its own: kh_run(const Call *, int op) is written out in the shim
#define HARNESS_EXPORTS(Call)                                                  \
    long long kh_guard_bytes() { return (long long)harness::GUARD; }         \
    long long kh_call_bytes() { return (long long)sizeof(Call); }
