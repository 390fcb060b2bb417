// rp_recompress.hip — recompression of compacted batches on the device
// (rpgpu_recompress).
//
// Reference: copy_data_segment_reducer::do_compaction
// (storage/compaction_reducers.cc:223-258) hands every batch filter() returns
// to storage::internal::compress_batch (storage/parser_utils.cc:82-120):
// compressor::compress over the records, attrs |= codec,
// reset_size_checksum_metadata, and the appender's header_crc;
// compress_batch_consumer (:62-80) is the same under a size threshold.  Here,
// for the batches of a completed rpgpu_compact, with no host synchronisation:
//
//   k_recompress_sizes   one thread per input batch: the effective codec and
//                what becomes of the batch; for an LZ4 / snappy one its 64 KiB
//                blocks (per snappy fragment) and their scratch bytes
//   (scans)      the batch's first block, its scratch
//   k_recompress_fill    one thread per batch to compress: its CompBlocks and
//                their scratch slots (the host builds these for
//                rpgpu_compress_batch; here it knows capacities only, so the
//                block array is zeroed and the block kernels run over its bound)
//   k_compress_blocks    (rp_compress.hip) one wave per block, from the payload
//                where it lies in the input log
//   k_deflate_blocks     (rp_deflate.hip) with rpgpu_set_device_gzip: a gzip
//                batch is ONE block of the same array (codec gzip, its scratch
//                slot the deflateBound), compressed as one fragment by one
//                lane; its frame is that block's bytes
//   k_recompress_layout_sizes  one thread per batch: its output bytes (the
//                frame's length from the block sizes), its pack pieces
//   (scans)      output position, output ordinal / first piece
//   k_recompress_layout  one thread per segment: offsets, summaries; the
//                totals and the overflow verdict
//   k_recompress_pack    one wave per piece: a compressed batch is one piece
//                (the header copy with attrs |= codec, then the frame by
//                wave_write_frame); a copied batch moves in pieces of
//                kAppendPiece bytes (wave_copy_lines), header included
//   k_stamp      (rp_validate.hip) RPGPU_STAMP_CRC over the compressed batches
//   k_recompress_meta    one thread per output batch: its entry and the
//                rpgpu_batch_result a RPGPU_JOB_CRC job over the output reports
//                (oracle/rp_oracle.c rpo_scan_segment_layout: every field
//                follows from the final header and its stored crcs, which
//                rpgpu_compact and k_stamp made true)
#include "rp_device.h"

namespace rp {

namespace {

DEV uint64_t n_in(const RecompressArgs& a) {
    const uint64_t n = a.job.d_ctotals->batches_out;
    return n < a.nb ? n : a.nb;
}
// nothing can be produced: the source call overflowed, or its entries are not what the capacities promise
DEV bool unusable(const RecompressArgs& a) { return a.job.d_ctotals->overflow != 0 || a.counters[kRcBadInput] != 0; }
DEV uint32_t count_of(uint64_t packed) { return (uint32_t)packed; }
DEV uint32_t pieces_of(uint64_t packed) { return (uint32_t)(packed >> 32); }
DEV bool not_written(const RecompressArgs& a) {
    return unusable(a) || a.bpos[a.nb] + 16 > a.job.out_capacity || count_of(a.bcnt[a.nb]) > a.job.out_batch_capacity;
}

// bytes a block of n input bytes may compress to, rounded to the 16-byte slot
// grid: lz4 is given n - 1 bytes (a block that needs more is stored raw),
// snappy takes snappy::MaxCompressedLength(n)
HD uint64_t slot_bytes(uint32_t codec, uint64_t n) {
    return ((codec == RPGPU_CODEC_SNAPPY ? 32 + n + n / 6 : n) + 15) & ~15ull;
}
// a gzip batch's slot: deflateBound on the 16-byte slot grid
HD uint64_t gzip_slot(uint64_t n) { return (df::bound(n) + 15) & ~15ull; }
struct Geom {
    uint64_t blocks, scratch;
};
// the 64 KiB blocks of one fragment (an LZ4 payload is one)
HD Geom frag_geom(uint32_t codec, uint64_t len) {
    const uint64_t full = len >> 16, rem = len & 65535;
    Geom g;
    g.blocks = full + (rem ? 1 : 0);
    g.scratch = full * slot_bytes(codec, 65536) + (rem ? slot_bytes(codec, rem) : 0);
    return g;
}
// the fragment size of a payload of plen bytes: snappy_java_compressor takes
// the iobuf's fragments one by one, lz4 buffers across them
HD uint64_t frag_size(uint32_t codec, uint64_t plen, uint64_t snappy_frag) {
    uint64_t fr = (codec == RPGPU_CODEC_SNAPPY && snappy_frag) ? snappy_frag : plen;
    if (fr > plen) fr = plen;
    return fr ? fr : 1;
}
HD Geom batch_geom(uint32_t codec, uint64_t plen, uint64_t fr) {
    const Geom f = frag_geom(codec, fr), r = frag_geom(codec, plen % fr);
    Geom g;
    g.blocks = (plen / fr) * f.blocks + r.blocks;
    g.scratch = (plen / fr) * f.scratch + r.scratch;
    return g;
}
// rpgpu_compress_bound
HD uint64_t compress_bound(uint32_t codec, uint64_t n, uint64_t fr) {
    if (codec == RPGPU_CODEC_LZ4) return 15 + ((n + 65535) / 65536) * (4 + 65536) + 4;
    return 16 + (n ? (n + fr - 1) / fr : 0) * (4 + 32 + fr + fr / 6);
}

DEV uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
DEV uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }
DEV uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// the first input batch at or behind input position x
DEV uint64_t first_batch_at(const RecompressArgs& a, uint64_t nin, uint64_t x) {
    uint64_t lo = 0, hi = nin;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.job.d_in_batches[mid].out_pos < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(256) void k_recompress_sizes(RecompressArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nb) return;
    uint32_t mode = 0;
    Geom g;
    g.blocks = g.scratch = 0;
    if (b < n_in(a) && a.job.d_ctotals->overflow == 0) {
        const rpgpu_compact_batch& e = a.job.d_in_batches[b];
        const uint64_t plen = e.payload_len, pos = e.out_pos;
        if (pos > a.job.in_capacity || RPGPU_HEADER_SIZE + plen + 16 > a.job.in_capacity - pos) {
            atomicOr(&a.counters[kRcBadInput], 1u);
        } else {
            uint32_t codec = a.job.codec == RPGPU_RECOMPRESS_SOURCE_CODEC ? e.codec : a.job.codec;
            if (codec > 0xFF) codec = 0xFF;
            uint32_t flags = 0;
            if (RPGPU_HEADER_SIZE + plen < a.job.min_batch_bytes) {
                codec = RPGPU_CODEC_NONE;
            } else if (codec == RPGPU_CODEC_LZ4 || codec == RPGPU_CODEC_SNAPPY) {
                const uint64_t fr = frag_size(codec, plen, a.job.snappy_frag);
                if (RPGPU_HEADER_SIZE + compress_bound(codec, plen, fr) > 0x7FFFFFFFull ||
                    (codec == RPGPU_CODEC_SNAPPY && 32 + fr + fr / 6 > 0x7FFFFFFFull)) {
                    flags = RPGPU_RECOMPRESS_F_TOO_LARGE;
                } else {
                    flags = RPGPU_RECOMPRESS_F_COMPRESSED;
                    mode |= kRcCompress;
                    g = batch_geom(codec, plen, fr);
                }
            } else if (codec == RPGPU_CODEC_GZIP && a.device_gzip) {
                // rpgpu_set_device_gzip: one block (one stream of k_deflate_blocks, one fragment), its
                // scratch slot the deflateBound
                if (!df::takes(plen)) {
                    flags = RPGPU_RECOMPRESS_F_TOO_LARGE;
                } else {
                    flags = RPGPU_RECOMPRESS_F_COMPRESSED;
                    mode |= kRcCompress;
                    g.blocks = 1;
                    g.scratch = gzip_slot(plen);
                }
            } else if (codec == RPGPU_CODEC_GZIP || codec == RPGPU_CODEC_ZSTD) {
                flags = RPGPU_RECOMPRESS_F_HOST;
            } else if (codec != RPGPU_CODEC_NONE) {
                flags = RPGPU_RECOMPRESS_F_BAD_CODEC;
            }
            mode |= codec | (flags << 16);
        }
    }
    a.mode[b] = mode;
    a.bblk[b] = g.blocks;
    a.bscr[b] = g.scratch;
}

// after the scans: bblk[b] / bscr[b] = the batch's first block and its scratch offset; [nb] the totals
__global__ __launch_bounds__(256) void k_recompress_fill(RecompressArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nb) return;
    if (a.bblk[a.nb] > a.block_cap || a.bscr[a.nb] > a.scratch_cap) {
        // cannot happen for batches that lie apart inside in_capacity
        if (b == 0) atomicOr(&a.counters[kRcBadInput], 1u);
        return;
    }
    const uint32_t mode = a.mode[b];
    if (!(mode & kRcCompress)) return;
    const uint32_t codec = mode & 0xFF;
    const rpgpu_compact_batch& e = a.job.d_in_batches[b];
    const uint64_t plen = e.payload_len, src = e.out_pos + RPGPU_HEADER_SIZE;
    uint64_t k = a.bblk[b], so = a.bscr[b];
    if (codec == RPGPU_CODEC_GZIP) {
        CompBlock c;
        c.src = src;
        c.n = (uint32_t)plen;
        c.codec = codec;
        c.frag_len = (uint32_t)plen;
        c.frag_blocks = 1;
        a.blocks[k] = c;
        a.slot_off[k] = so;
        return;
    }
    const uint64_t fr = frag_size(codec, plen, a.job.snappy_frag);
    for (uint64_t f = 0; f < plen; f += fr) {
        const uint64_t flen = plen - f < fr ? plen - f : fr;
        const uint32_t nbk = (uint32_t)((flen + 65535) >> 16);
        for (uint32_t j = 0; j < nbk; j++, k++) {
            const uint64_t at = (uint64_t)j << 16;
            CompBlock c;
            c.src = src + f + at;
            c.n = (uint32_t)(flen - at < 65536 ? flen - at : 65536);
            c.codec = codec;
            c.frag_len = j == 0 ? (uint32_t)flen : 0;
            c.frag_blocks = j == 0 ? nbk : 0;
            a.blocks[k] = c;
            a.slot_off[k] = so;
            so += slot_bytes(codec, c.n);
        }
    }
}

__global__ __launch_bounds__(256) void k_recompress_layout_sizes(RecompressArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t size = 0, cnt = 0, in_bytes = 0;
    uint32_t compressed = 0, host = 0;
    if (b < n_in(a) && !unusable(a)) {
        const uint32_t mode = a.mode[b];
        const uint64_t plen = a.job.d_in_batches[b].payload_len;
        uint64_t clen = plen, pieces;
        if (mode & kRcCompress) {
            const uint64_t first = a.bblk[b];
            clen = frame_bytes(plen, (uint32_t)first, (uint32_t)(a.bblk[b + 1] - first), mode & 0xFF, a.blocks, a.sizes);
            pieces = 1;
            compressed = 1;
        } else {
            pieces = (RPGPU_HEADER_SIZE + plen + kAppendPiece - 1) / kAppendPiece;
            host = ((mode >> 16) & RPGPU_RECOMPRESS_F_HOST) ? 1 : 0;
        }
        a.clen[b] = (uint32_t)clen;
        size = RPGPU_HEADER_SIZE + clen;
        cnt = 1ull | (pieces << 32);
        in_bytes = RPGPU_HEADER_SIZE + plen;
    }
    if (b < a.nb) {
        a.bpos[b] = size;
        a.bcnt[b] = cnt;
    }
    // the totals' sums: one atomic per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        in_bytes += (uint64_t)__shfl_xor((unsigned long long)in_bytes, o, 64);
        compressed += __shfl_xor(compressed, o, 64);
        host += __shfl_xor(host, o, 64);
    }
    if (lane() == 0 && in_bytes) {
        rpgpu_recompress_totals* T = a.job.d_rtotals;
        atomicAdd((unsigned long long*)&T->bytes_in, (unsigned long long)in_bytes);
        if (compressed) atomicAdd((unsigned long long*)&T->batches_compressed, (unsigned long long)compressed);
        if (host) atomicAdd((unsigned long long*)&T->batches_host, (unsigned long long)host);
    }
}

// after the scans: bpos[b] / bcnt[b] = output position, output ordinal and first piece; [nb] the totals
__global__ __launch_bounds__(256) void k_recompress_layout(RecompressArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = unusable(a);
    const uint64_t nin = bad ? 0 : n_in(a);
    if (s == 0) {
        rpgpu_recompress_totals* T = a.job.d_rtotals;
        const uint64_t bytes = bad ? 0 : a.bpos[a.nb], nout = bad ? 0 : count_of(a.bcnt[a.nb]);
        T->batches_out = nout;
        T->bytes_out = bytes;
        T->out_capacity_needed = bytes + 16;
        T->out_batch_capacity_needed = nout;
        T->overflow = (bytes + 16 > a.job.out_capacity ? 1u : 0u) | (nout > a.job.out_batch_capacity ? 2u : 0u) |
                      (bad ? 4u : 0u);
        a.job.d_out_seg_offsets[a.job.n_segments] = bytes;
    }
    if (s >= a.job.n_segments) return;
    const uint64_t fb = first_batch_at(a, nin, a.job.d_in_seg_offsets[s]);
    uint64_t fe = first_batch_at(a, nin, a.job.d_in_seg_offsets[s + 1]);
    if (fe < fb) fe = fb;
    const uint64_t o0 = bad ? 0 : a.bpos[fb], bytes = bad ? 0 : a.bpos[fe] - o0;
    const uint64_t c0 = bad ? 0 : count_of(a.bcnt[fb]), n = bad ? 0 : count_of(a.bcnt[fe]) - c0;
    a.job.d_out_seg_offsets[s] = o0;
    // what a disk-layout job reports for a clean segment of n batches (the
    // chain ran to the end of the stream; the checkpoint is the last batch,
    // whose offsets the recompression leaves as they were)
    int64_t last_offset = 0;
    if (n) {
        const uint8_t* h = a.job.d_in + a.job.d_in_batches[fe - 1].out_pos;
        last_offset = (int64_t)(rd64(h + 8) + (uint64_t)(int64_t)(int32_t)rd32(h + 23));
    }
    rpgpu_segment_summary m;
    m.first_batch = c0;
    m.n_batches = n;
    m.terminal_pos = bytes;
    m.bytes_consumed = bytes;
    m.terminal_errc = RPGPU_ERRC_END_OF_STREAM;
    m.terminal_eof = 1;
    m.has_checkpoint = n ? 1 : 0;
    m.first_bad = (uint32_t)n;
    m.ckpt_last_offset = last_offset;
    m.ckpt_truncate_pos = n ? bytes : 0;
    m.n_records = 0;
    m.reserved[0] = m.reserved[1] = 0;
    a.job.d_out_summaries[s] = m;
}

__global__ __launch_bounds__(256) void k_recompress_pack(RecompressArgs a) {
    if (not_written(a)) return;
    const uint32_t l = lane();
    const uint32_t npieces = pieces_of(a.bcnt[a.nb]);
    const uint32_t waves = gridDim.x * 4;
    for (uint32_t w = uni32(blockIdx.x * 4 + (threadIdx.x >> 6)); w < npieces; w += waves) {
        // the batch owning piece w: pieces(lo) <= w < pieces(hi)
        uint64_t lo = 0, hi = a.nb;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (pieces_of(a.bcnt[mid]) <= w) lo = mid;
            else hi = mid;
        }
        const uint64_t b = lo;
        const uint32_t k = w - pieces_of(a.bcnt[b]);
        const uint32_t mode = uni32(a.mode[b]);
        const rpgpu_compact_batch& e = a.job.d_in_batches[b];
        const uint32_t plen = uni32(e.payload_len);
        const uint64_t op = uni64(a.bpos[b]);
        const uint8_t* __restrict__ src = a.job.d_in + uni64(e.out_pos);
        uint8_t* __restrict__ dst = a.job.d_out + op;
        if (mode & kRcCompress) {
            // compress_batch: attrs |= codec; size, crc and header_crc follow in k_stamp
            if (l < RPGPU_HEADER_SIZE) dst[l] = (uint8_t)(src[l] | (l == 21 ? (mode & 7u) : 0u));
            const uint64_t first = uni64(a.bblk[b]);
            wave_write_frame(dst + RPGPU_HEADER_SIZE, a.job.d_in, plen, (uint32_t)first,
                             (uint32_t)(uni64(a.bblk[b + 1]) - first), mode & 0xFF, a.blocks, a.scratch, a.slot_off,
                             a.sizes);
            if (l == 0) {
                const uint32_t i = atomicAdd(&a.counters[kRcStampCount], 1u);
                a.spos[i] = op;
                a.splen[i] = a.clen[b];
            }
        } else {
            const uint64_t total = (uint64_t)RPGPU_HEADER_SIZE + plen, p0 = (uint64_t)k * kAppendPiece;
            const uint32_t n = (uint32_t)(total - p0 < kAppendPiece ? total - p0 : kAppendPiece);
            wave_copy_lines(dst + p0, src + p0, n, l);
        }
    }
}

__global__ __launch_bounds__(256) void k_recompress_meta(RecompressArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nb || not_written(a) || b >= n_in(a)) return;
    const uint64_t op = a.bpos[b];
    const uint32_t oi = count_of(a.bcnt[b]), mode = a.mode[b];
    const rpgpu_compact_batch& src = a.job.d_in_batches[b];
    // the input segment holding the batch: the last one starting at or before it
    uint32_t lo = 0, hi = a.job.n_segments;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.job.d_in_seg_offsets[mid] <= src.out_pos) lo = mid;
        else hi = mid;
    }
    rpgpu_recompress_batch g;
    g.out_pos = op;
    g.in_batch = (uint32_t)b;
    g.payload_len = a.clen[b];
    g.in_payload_len = src.payload_len;
    g.codec = mode & 0xFF;
    g.flags = mode >> 16;
    g.reserved = 0;
    a.job.d_out_entries[oi] = g;
    const uint8_t* h = a.job.d_out + op;
    const uint32_t attrs = rd16(h + 21), codec = attrs & 7;
    rpgpu_batch_result e;
    e.file_pos = op - a.job.d_out_seg_offsets[lo];
    e.base_offset = (int64_t)rd64(h + 8);
    e.first_timestamp = (int64_t)rd64(h + 27);
    e.max_timestamp = (int64_t)rd64(h + 35);
    e.producer_id = (int64_t)rd64(h + 43);
    e.size_bytes = (int32_t)rd32(h + 4);
    e.record_count = (int32_t)rd32(h + 57);
    e.last_offset_delta = (int32_t)rd32(h + 23);
    e.base_sequence = (int32_t)rd32(h + 53);
    e.header_crc = e.header_crc_computed = rd32(h);
    e.crc = e.crc_computed = rd32(h + 17);
    e.flags = RPGPU_F_HEADER_OK | RPGPU_F_COMPLETE | RPGPU_F_CRC_OK | (codec ? RPGPU_F_COMPRESSED : 0u) |
              (codec >= 5 ? RPGPU_F_CODEC_INVALID : 0u) | (codec == RPGPU_CODEC_ZSTD ? RPGPU_F_CODEC_UNSUPPORTED : 0u);
    e.segment = lo;
    e.index_base = 0;
    e.decoded_off = 0;
    e.records_parsed = 0;
    e.decoded_len = codec ? 0u : g.payload_len;
    e.decoded_crc = 0;
    e.decoded_header_crc = 0;
    e.attrs = (int16_t)attrs;
    e.producer_epoch = (int16_t)rd16(h + 51);
    e.type = (int8_t)h[16];
    e.parse_err = 0;
    e.reserved0 = 0;
    e.reserved1 = 0;
    a.job.d_out_batches[oi] = e;
}

static uint32_t thread_grid(uint64_t items) { return (uint32_t)(items ? (items + 255) / 256 : 1); }

uint64_t recompress_block_cap(uint64_t in_capacity, uint64_t in_batch_capacity, uint64_t snappy_frag) {
    // a payload of n bytes in fragments of f has at most n / 65536 + n / f + 1
    // blocks (every fragment ends one), n / 65536 + 1 without fragments
    return in_capacity / 65536 + (snappy_frag ? in_capacity / snappy_frag : 0) + in_batch_capacity + 2;
}
uint64_t recompress_scratch_cap(uint64_t in_capacity, uint64_t block_cap) {
    // slot_bytes summed: at most 7/6 of the block's bytes and 47 more
    return in_capacity + in_capacity / 6 + 48 * block_cap + 256;
}

hipError_t launch_recompress_plan(const RecompressArgs& a, void* scan_tmp, size_t scan_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_recompress_sizes, dim3(thread_grid(a.nb)), dim3(256), 0, s, a);
    scan_exclusive_u64(a.bblk, a.nb, scan_tmp, scan_bytes, s);
    scan_exclusive_u64(a.bscr, a.nb, scan_tmp, scan_bytes, s);
    hipLaunchKernelGGL(k_recompress_fill, dim3(thread_grid(a.nb)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_recompress_layout(const RecompressArgs& a, void* scan_tmp, size_t scan_bytes, hipStream_t s) {
    if (a.nb) {
        hipLaunchKernelGGL(k_recompress_layout_sizes, dim3(thread_grid(a.nb)), dim3(256), 0, s, a);
        scan_exclusive_u64(a.bpos, a.nb, scan_tmp, scan_bytes, s);
        scan_exclusive_u64(a.bcnt, a.nb, scan_tmp, scan_bytes, s);
    }
    hipLaunchKernelGGL(k_recompress_layout, dim3(thread_grid((uint64_t)a.job.n_segments + 1)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_recompress_pack(const RecompressArgs& a, uint32_t cus, hipStream_t s) {
    // the piece count lives on the device: the bound the host knows is one
    // piece per batch plus one per kAppendPiece bytes of input
    const uint64_t pieces = a.nb + a.job.in_capacity / kAppendPiece;
    const uint64_t blocks = (pieces + 3) / 4, cap = (uint64_t)cus * 8;
    hipLaunchKernelGGL(k_recompress_pack, dim3((uint32_t)(blocks < 1 ? 1 : blocks < cap ? blocks : cap)), dim3(256), 0, s,
                       a);
    return hipGetLastError();
}
hipError_t launch_recompress_meta(const RecompressArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_recompress_meta, dim3(thread_grid(a.nb)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rp
