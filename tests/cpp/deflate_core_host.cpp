// Host build of the device gzip compressor's logic (rp_deflate_core.h), TEST
// INFRASTRUCTURE ONLY: tests/test_deflate_core.py compares it byte for byte
// with zlib itself, so that what k_deflate runs one lane per payload is
// pinned on the CPU, where thousands of inputs take seconds.  The product
// never loads this library.
#include <stdint.h>
#include <stdlib.h>

// how often gen_bitlen's overflow repair ran, per max_length (15: literal and
// distance trees, 7: the bit-length tree): the corpus proves it reaches both
static uint64_t g_overflows[16];
#define DF_NOTE_OVERFLOW(max_length) g_overflows[max_length]++
#include "../../redpanda_amd/csrc/rp_deflate_core.h"

extern "C" uint64_t df_host_overflows(int max_length) { return g_overflows[max_length & 15]; }

extern "C" uint64_t df_host_work_bytes() { return rp::df::kWorkBytes; }
extern "C" uint64_t df_host_bound(uint64_t n) { return rp::df::bound(n); }

// out: df_host_bound(n) bytes; returns the stream's length, 0 without memory
extern "C" uint64_t df_host_gzip(const uint8_t* src, uint64_t n, uint64_t frag, uint8_t* out) {
    // a dirty work area: the core may rely on nothing but what it clears
    rp::df::Work* w = (rp::df::Work*)malloc(sizeof(rp::df::Work));
    if (!w) return 0;
    for (uint64_t i = 0; i < sizeof(rp::df::Work); i++) ((uint8_t*)w)[i] = (uint8_t)(0xA5 + i * 7);
    const uint64_t r = rp::df::gzip(src, n, frag, out, w);
    free(w);
    return r;
}
