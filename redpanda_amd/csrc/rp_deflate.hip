// rp_deflate.hip — compression::compressor::compress on the device for gzip:
// gzip_compressor::compress (compression/internal/gzip_compressor.cc:126-161)
// over zlib 1.2.11's deflate at level 6, byte for byte.  The algorithm is
// rp_deflate_core.h, the same text the CPU tests pin against the library
// (tests/test_deflate_core.py); this file only gives it lanes and memory.
//
// Execution model.  deflate is one serial chain per stream (every match
// decision feeds the hash chains the next one reads, every block's trees come
// from its symbol counts), so a payload is run by ONE LANE, start to end.
// The lanes are spread one per wave: the other lanes of a full wave would run
// 63 unrelated control flows in lock step, and the work area (df::kWorkBytes,
// about 183 KiB per stream) is what bounds the number of resident streams,
// not the lanes; one stream per wave gives each of up to kDeflateStreams
// streams a SIMD's issue slots.  The wave's 64 lanes together zero the
// stream's `head` table (a clear pass, 16 bytes per lane and step) before
// lane 0 starts; everything else is lane 0.  Payloads come from a list behind
// an atomic cursor: a wave that finishes a small payload takes the next.
// Output bits go straight into the payload's slot of deflateBound bytes.
// Plain loads and stores only.  Byte work only: no MFMA.
//
// k_deflate takes rpgpu_compress_batch's staged payloads; k_deflate_blocks
// takes the gzip blocks of rpgpu_recompress's block array (one block per
// batch, from the payload where it lies in the log, one fragment).
#define DF_FN __device__ inline
#define DF_CONST static __constant__
#include "rp_device.h"

namespace rp {

static_assert(df::kWorkBytes % 16 == 0 && kDeflateCursor % 16 == 0, "work areas stay 16-byte aligned");

namespace {

DEV df::Work* work_of(uint8_t* work) { return (df::Work*)(work + kDeflateCursor + (uint64_t)blockIdx.x * df::kWorkBytes); }

// the next list index (wave-uniform)
DEV uint32_t take(uint8_t* work) {
    uint32_t i = 0;
    if (lane() == 0) i = atomicAdd((uint32_t*)work, 1u);
    return uni32(i);
}

// head: zeros for every stream
DEV void clear_head(df::Work* w) {
    uint4* h = (uint4*)w->head;
    for (uint32_t k = lane(); k < sizeof(w->head) / 16; k += 64) h[k] = make_uint4(0, 0, 0, 0);
    __threadfence_block();
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_deflate(const uint8_t* __restrict__ in, const DeflateItem* __restrict__ items,
                                                uint32_t count, uint8_t* __restrict__ out, uint64_t* __restrict__ out_len,
                                                uint8_t* __restrict__ work) {
    df::Work* w = work_of(work);
    for (;;) {
        const uint32_t i = take(work);
        if (i >= count) return;
        clear_head(w);
        if (lane() == 0) {
            const DeflateItem it = items[i];
            out_len[i] = df::gzip(in + it.src, it.n, it.frag, out + it.out, w, true);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_deflate_blocks(const uint8_t* __restrict__ in, const CompBlock* __restrict__ blocks,
                                                       uint32_t nb, uint8_t* __restrict__ scratch,
                                                       const uint64_t* __restrict__ slot_off, uint32_t* __restrict__ sizes,
                                                       uint8_t* __restrict__ work) {
    df::Work* w = work_of(work);
    for (;;) {
        const uint32_t b = take(work);
        if (b >= nb) return;
        if (uni32(blocks[b].codec) != RPGPU_CODEC_GZIP) continue;
        clear_head(w);
        if (lane() == 0)
            sizes[b] = (uint32_t)df::gzip(in + blocks[b].src, blocks[b].n, 0, scratch + slot_off[b], w, true);
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_deflate(const uint8_t* in, const DeflateItem* items, uint32_t count, uint8_t* out, uint64_t* out_len,
                          uint8_t* work, uint32_t streams, hipStream_t s) {
    if (!count) return hipSuccess;
    hipError_t e = hipMemsetAsync(work, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_deflate, dim3(streams), dim3(64), 0, s, in, items, count, out, out_len, work);
    return hipGetLastError();
}

hipError_t launch_deflate_blocks(const uint8_t* in, const CompBlock* blocks, uint32_t nb, uint8_t* scratch,
                                 const uint64_t* slot_off, uint32_t* sizes, uint8_t* work, uint32_t streams, hipStream_t s) {
    if (!nb) return hipSuccess;
    hipError_t e = hipMemsetAsync(work, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_deflate_blocks, dim3(streams), dim3(64), 0, s, in, blocks, nb, scratch, slot_off, sizes, work);
    return hipGetLastError();
}

}  // namespace rp
