// guard_scan_main.cpp - the band scan of the diagnostic allocator (dfmdock_amd/csrc/dfm_guardscan.h) without a GPU, for
// tests/test_alloc_recipe_cpu.py, which builds this file with the address and undefined-behaviour sanitizers.
// usage: guard_scan N [OFFSET:BYTE ...]   a band of exactly N heap bytes filled with the guard byte, then damaged as listed; prints the
// offset of the first damaged byte (N: intact).  The band is its own allocation, so a scan that reads past it is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dfm_guardscan.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s N [OFFSET:BYTE ...]\n", argv[0]); return 2; }
    const size_t n = (size_t)strtoull(argv[1], nullptr, 10);
    unsigned char *band = n ? static_cast<unsigned char *>(malloc(n)) : nullptr;      // N = 0: no byte may be read at all
    if (n && !band) return 3;
    if (n) memset(band, dfm::GUARD_BYTE, n);
    for (int a = 2; a < argc; ++a) {
        unsigned long long off = 0; unsigned int byte = 0;
        if (sscanf(argv[a], "%llu:%u", &off, &byte) != 2 || off >= n || byte > 255) { fprintf(stderr, "bad damage %s\n", argv[a]); free(band); return 2; }
        band[off] = (unsigned char)byte;
    }
    printf("%zu\n", dfm::guard_first_damaged(band, n));
    free(band);
    return 0;
}
