// dfm_guardscan.h - the scan of one guard band of the diagnostic allocator (dfm_host.h: DFM_ALLOC_GUARD), in plain C++: the library runs
// it over the host copy of every band at release, tests/guard_scan_main.cpp calls it without a GPU.
#pragma once

#include <stddef.h>

namespace dfm {

constexpr unsigned char GUARD_BYTE = 0xA5;      // what a band is filled with when its block is handed out

// offset of the first byte of band[0 .. n) that is no longer GUARD_BYTE; n when the band is intact (a band of no bytes is)
inline size_t guard_first_damaged(const unsigned char *band, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        if (band[k] != GUARD_BYTE) return k;
    return n;
}

}  // namespace dfm
