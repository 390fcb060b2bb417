// rp_deflate_core.h — gzip_compressor::compress (compression/internal/
// gzip_compressor.cc:51-64, :126-161) written once for host and device:
//   deflateInit2(Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15 + 16, 8,
//   Z_DEFAULT_STRATEGY), one deflate(Z_NO_FLUSH) per iobuf fragment into a
//   deflateBound-sized buffer, one deflate(Z_FINISH)
// over zlib 1.2.11, byte for byte.  No library calls: the device runs this
// text one lane per payload (rp_deflate.hip); tests/cpp/deflate_core_host.cpp
// builds it for the host, where tests/test_deflate_core.py pins it against
// the library itself.
//
// What is restated (level 6, memLevel 8, windowBits 15, default strategy):
//   * the gzip wrapper: the 10 header bytes 1f 8b 08 00 00 00 00 00 00 03,
//     CRC32 and ISIZE little-endian;
//   * deflate_slow: lazy matching over prev_length / prev_match /
//     match_available, string insertion up to max_insert inside an emitted
//     match, a block flushed at 16383 symbols, the pending literal and the
//     last block at Z_FINISH;
//   * longest_match: max_chain 128 (a quarter from good_length 8),
//     nice_length 128 clamped to the lookahead, max_lazy 16, MAX_DIST 32506,
//     NIL = 0 (window position 0 is never a candidate), TOO_FAR 4096;
//   * fill_window's schedule: at most window_size - lookahead - strstart
//     bytes of the current fragment, a slide by 32768 (slide_hash included)
//     once strstart >= w_size + MAX_DIST, a return for more input whenever
//     the lookahead is below 262 under Z_NO_FLUSH.  The payload is contiguous,
//     so it serves as the window itself: window[i] is src[base + i] and only
//     `base` moves.  Everything else (strstart, match_start, block_start, the
//     head / prev entries) is window-relative exactly as in zlib, because a
//     block whose start has slid out (block_start < 0) cannot be stored and a
//     chain entry that slid to 0 is NIL;
//   * trees.c: _tr_flush_block's choice among stored / fixed / dynamic,
//     build_tree (heap order, smaller()'s depth tie-break, the two forced
//     codes), gen_bitlen's overflow repair, gen_codes, scan_tree / send_tree
//     with the repeat codes, send_all_trees, compress_block.
// The hash is zlib's rolling ins_h computed from the three bytes it covers:
// ins_h is re-seeded from the window whenever fill_window has read input and
// the strings skipped past max_insert are never inserted, so both agree at
// every INSERT_STRING.
// zlib's pending buffer is not restated: the output slot holds deflateBound
// bytes (bound()), so every flush_pending drains completely and the bits go
// straight to the slot.
#pragma once
#include <stdint.h>

#ifndef DF_FN
#define DF_FN inline
#endif
#ifndef DF_CONST
#define DF_CONST static const
#endif
// test hook: gen_bitlen's overflow repair ran (max_length: 15 or 7)
#ifndef DF_NOTE_OVERFLOW
#define DF_NOTE_OVERFLOW(max_length)
#endif

namespace rp {
namespace df {

constexpr uint32_t kWSize = 32768, kWMask = kWSize - 1, kWindowSize = 2 * kWSize;
constexpr uint32_t kHashMask = 32767, kHashShift = 5;
constexpr uint32_t kLitBufsize = 16384;
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258, kMinLookahead = kMaxMatch + kMinMatch + 1;
constexpr uint32_t kMaxDist = kWSize - kMinLookahead, kTooFar = 4096;
constexpr uint32_t kGoodLength = 8, kMaxLazy = 16, kNiceLength = 128, kMaxChain = 128;
constexpr int kLiterals = 256, kLengthCodes = 29, kLCodes = kLiterals + 1 + kLengthCodes, kDCodes = 30, kBlCodes = 19;
constexpr int kHeapSize = 2 * kLCodes + 1, kMaxBits = 15, kMaxBlBits = 7, kEndBlock = 256;
constexpr int kRep3_6 = 16, kRepz3_10 = 17, kRepz11_138 = 18;

DF_CONST uint8_t kExtraL[kLengthCodes] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
DF_CONST uint8_t kExtraD[kDCodes] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
DF_CONST uint8_t kExtraBl[kBlCodes] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 7};
DF_CONST uint8_t kBlOrder[kBlCodes] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ct_data: Freq and Code share a field, Dad and Len share a field (gen_bitlen
// overwrites Dad with Len while it still reads the parents')
struct Ct {
    uint16_t fc;
    uint16_t dl;
};

// the work area of one stream
struct alignas(16) Work {
    uint16_t head[kWSize];  // zeros at the start of every stream (gzip() clears it)
    uint16_t prev[kWSize];
    uint16_t d_buf[kLitBufsize];  // the symbol buffer: distances (0: a literal) ...
    uint8_t l_buf[kLitBufsize];   // ... and literals / match lengths - 3
    Ct dyn_ltree[kHeapSize], dyn_dtree[2 * kDCodes + 1], bl_tree[2 * kBlCodes + 1];
    Ct static_ltree[kLCodes + 2], static_dtree[kDCodes];
    uint16_t heap[kHeapSize];
    uint8_t depth[kHeapSize];
    uint16_t bl_count[kMaxBits + 1];
    uint16_t base_length[kLengthCodes], base_dist[kDCodes];
    uint8_t length_code[kMaxMatch - kMinMatch + 1], dist_code[512];
    uint32_t crc_tab[256];
};
constexpr uint64_t kWorkBytes = sizeof(Work);

// deflateBound for these parameters (the gzip wrapper included)
constexpr uint64_t bound(uint64_t n) { return n + (n >> 12) + (n >> 14) + (n >> 25) + 25; }
// a payload is taken when a batch header (61 bytes) plus its bound fits int32
// (a batch's size_bytes)
constexpr bool takes(uint64_t n) { return n < (1ull << 31) && 61 + bound(n) <= 0x7FFFFFFFull; }

struct State {
    Work* w;
    const uint8_t* src;  // the payload; window[i] = src[base + i]
    uint8_t* out;
    uint64_t op;
    uint64_t bi_buf;
    uint32_t bi_valid;
    uint64_t base;  // payload offset of window[0]
    uint64_t read;  // payload bytes read into the window (total_in)
    uint32_t strstart, lookahead, match_length, prev_length, match_start, prev_match, match_available;
    int64_t block_start;
    uint32_t last_lit;
    uint64_t opt_len, static_len;
    int l_max_code, d_max_code;
    int heap_len, heap_max;
};

DF_FN void send_bits(State& s, uint32_t value, uint32_t length) {
    s.bi_buf |= (uint64_t)value << s.bi_valid;
    s.bi_valid += length;
    while (s.bi_valid >= 8) {
        s.out[s.op++] = (uint8_t)s.bi_buf;
        s.bi_buf >>= 8;
        s.bi_valid -= 8;
    }
}
DF_FN void send_code(State& s, uint32_t c, const Ct* tree) { send_bits(s, tree[c].fc, tree[c].dl); }
DF_FN void bi_windup(State& s) {
    if (s.bi_valid) s.out[s.op++] = (uint8_t)s.bi_buf;
    s.bi_buf = 0;
    s.bi_valid = 0;
}
DF_FN uint32_t bi_reverse(uint32_t code, int len) {
    uint32_t res = 0;
    do {
        res |= code & 1;
        code >>= 1;
        res <<= 1;
    } while (--len > 0);
    return res >> 1;
}

DF_FN void gen_codes(Ct* tree, int max_code, const uint16_t* bl_count) {
    uint16_t next_code[kMaxBits + 1];
    uint32_t code = 0;
    for (int bits = 1; bits <= kMaxBits; bits++) {
        code = (code + bl_count[bits - 1]) << 1;
        next_code[bits] = (uint16_t)code;
    }
    for (int n = 0; n <= max_code; n++) {
        const int len = tree[n].dl;
        if (len == 0) continue;
        tree[n].fc = (uint16_t)bi_reverse(next_code[len]++, len);
    }
}

// tr_static_init, and the CRC32 table
DF_FN void static_init(Work* w) {
    int n, code, length = 0, dist = 0;
    for (code = 0; code < kLengthCodes - 1; code++) {
        w->base_length[code] = (uint16_t)length;
        for (n = 0; n < (1 << kExtraL[code]); n++) w->length_code[length++] = (uint8_t)code;
    }
    w->base_length[code] = 0;
    w->length_code[length - 1] = (uint8_t)code;
    for (code = 0; code < 16; code++) {
        w->base_dist[code] = (uint16_t)dist;
        for (n = 0; n < (1 << kExtraD[code]); n++) w->dist_code[dist++] = (uint8_t)code;
    }
    dist >>= 7;
    for (; code < kDCodes; code++) {
        w->base_dist[code] = (uint16_t)(dist << 7);
        for (n = 0; n < (1 << (kExtraD[code] - 7)); n++) w->dist_code[256 + dist++] = (uint8_t)code;
    }
    for (n = 0; n <= kMaxBits; n++) w->bl_count[n] = 0;
    n = 0;
    while (n <= 143) w->static_ltree[n++].dl = 8, w->bl_count[8]++;
    while (n <= 255) w->static_ltree[n++].dl = 9, w->bl_count[9]++;
    while (n <= 279) w->static_ltree[n++].dl = 7, w->bl_count[7]++;
    while (n <= 287) w->static_ltree[n++].dl = 8, w->bl_count[8]++;
    gen_codes(w->static_ltree, kLCodes + 1, w->bl_count);
    for (n = 0; n < kDCodes; n++) {
        w->static_dtree[n].dl = 5;
        w->static_dtree[n].fc = (uint16_t)bi_reverse((uint32_t)n, 5);
    }
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
        w->crc_tab[i] = c;
    }
}

DF_FN void init_block(State& s) {
    Work* w = s.w;
    for (int n = 0; n < kLCodes; n++) w->dyn_ltree[n].fc = 0;
    for (int n = 0; n < kDCodes; n++) w->dyn_dtree[n].fc = 0;
    for (int n = 0; n < kBlCodes; n++) w->bl_tree[n].fc = 0;
    w->dyn_ltree[kEndBlock].fc = 1;
    s.opt_len = s.static_len = 0;
    s.last_lit = 0;
}

DF_FN bool smaller(const Ct* tree, int n, int m, const uint8_t* depth) {
    return tree[n].fc < tree[m].fc || (tree[n].fc == tree[m].fc && depth[n] <= depth[m]);
}

DF_FN void pqdownheap(State& s, const Ct* tree, int k) {
    Work* w = s.w;
    const int v = w->heap[k];
    int j = k << 1;
    while (j <= s.heap_len) {
        if (j < s.heap_len && smaller(tree, w->heap[j + 1], w->heap[j], w->depth)) j++;
        if (smaller(tree, v, w->heap[j], w->depth)) break;
        w->heap[k] = w->heap[j];
        k = j;
        j <<= 1;
    }
    w->heap[k] = (uint16_t)v;
}

DF_FN void gen_bitlen(State& s, Ct* tree, int max_code, const Ct* stree, const uint8_t* extra, int base, int max_length) {
    Work* w = s.w;
    int h, n, m, bits, xbits, overflow = 0;
    for (bits = 0; bits <= kMaxBits; bits++) w->bl_count[bits] = 0;
    tree[w->heap[s.heap_max]].dl = 0;  // the root
    for (h = s.heap_max + 1; h < kHeapSize; h++) {
        n = w->heap[h];
        bits = tree[tree[n].dl].dl + 1;
        if (bits > max_length) bits = max_length, overflow++;
        tree[n].dl = (uint16_t)bits;
        if (n > max_code) continue;  // not a leaf
        w->bl_count[bits]++;
        xbits = 0;
        if (n >= base) xbits = extra[n - base];
        const uint64_t f = tree[n].fc;
        s.opt_len += f * (uint32_t)(bits + xbits);
        if (stree) s.static_len += f * (uint32_t)(stree[n].dl + xbits);
    }
    if (overflow == 0) return;
    DF_NOTE_OVERFLOW(max_length);
    do {
        bits = max_length - 1;
        while (w->bl_count[bits] == 0) bits--;
        w->bl_count[bits]--;
        w->bl_count[bits + 1] += 2;
        w->bl_count[max_length]--;
        overflow -= 2;
    } while (overflow > 0);
    for (bits = max_length; bits != 0; bits--) {
        n = w->bl_count[bits];
        while (n != 0) {
            m = w->heap[--h];
            if (m > max_code) continue;
            if ((uint32_t)tree[m].dl != (uint32_t)bits) {
                s.opt_len += ((uint64_t)bits - tree[m].dl) * tree[m].fc;
                tree[m].dl = (uint16_t)bits;
            }
            n--;
        }
    }
}

// returns max_code
DF_FN int build_tree(State& s, Ct* tree, const Ct* stree, const uint8_t* extra, int base, int elems, int max_length) {
    Work* w = s.w;
    int n, m, max_code = -1, node;
    s.heap_len = 0;
    s.heap_max = kHeapSize;
    for (n = 0; n < elems; n++) {
        if (tree[n].fc != 0) {
            w->heap[++s.heap_len] = (uint16_t)(max_code = n);
            w->depth[n] = 0;
        } else {
            tree[n].dl = 0;
        }
    }
    while (s.heap_len < 2) {
        node = w->heap[++s.heap_len] = (uint16_t)(max_code < 2 ? ++max_code : 0);
        tree[node].fc = 1;
        w->depth[node] = 0;
        s.opt_len--;
        if (stree) s.static_len -= stree[node].dl;
    }
    for (n = s.heap_len / 2; n >= 1; n--) pqdownheap(s, tree, n);
    node = elems;
    do {
        n = w->heap[1];
        w->heap[1] = w->heap[s.heap_len--];
        pqdownheap(s, tree, 1);
        m = w->heap[1];
        w->heap[--s.heap_max] = (uint16_t)n;
        w->heap[--s.heap_max] = (uint16_t)m;
        tree[node].fc = (uint16_t)(tree[n].fc + tree[m].fc);
        w->depth[node] = (uint8_t)((w->depth[n] >= w->depth[m] ? w->depth[n] : w->depth[m]) + 1);
        tree[n].dl = tree[m].dl = (uint16_t)node;
        w->heap[1] = (uint16_t)node++;
        pqdownheap(s, tree, 1);
    } while (s.heap_len >= 2);
    w->heap[--s.heap_max] = w->heap[1];
    gen_bitlen(s, tree, max_code, stree, extra, base, max_length);
    gen_codes(tree, max_code, w->bl_count);
    return max_code;
}

DF_FN void scan_tree(State& s, Ct* tree, int max_code) {
    Ct* bl = s.w->bl_tree;
    int prevlen = -1, curlen, nextlen = tree[0].dl, count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) max_count = 138, min_count = 3;
    tree[max_code + 1].dl = 0xffff;  // guard
    for (int n = 0; n <= max_code; n++) {
        curlen = nextlen;
        nextlen = tree[n + 1].dl;
        if (++count < max_count && curlen == nextlen) {
            continue;
        } else if (count < min_count) {
            bl[curlen].fc = (uint16_t)(bl[curlen].fc + count);
        } else if (curlen != 0) {
            if (curlen != prevlen) bl[curlen].fc++;
            bl[kRep3_6].fc++;
        } else if (count <= 10) {
            bl[kRepz3_10].fc++;
        } else {
            bl[kRepz11_138].fc++;
        }
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) max_count = 138, min_count = 3;
        else if (curlen == nextlen) max_count = 6, min_count = 3;
        else max_count = 7, min_count = 4;
    }
}

DF_FN void send_tree(State& s, const Ct* tree, int max_code) {
    const Ct* bl = s.w->bl_tree;
    int prevlen = -1, curlen, nextlen = tree[0].dl, count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) max_count = 138, min_count = 3;
    for (int n = 0; n <= max_code; n++) {
        curlen = nextlen;
        nextlen = tree[n + 1].dl;
        if (++count < max_count && curlen == nextlen) {
            continue;
        } else if (count < min_count) {
            do { send_code(s, (uint32_t)curlen, bl); } while (--count != 0);
        } else if (curlen != 0) {
            if (curlen != prevlen) {
                send_code(s, (uint32_t)curlen, bl);
                count--;
            }
            send_code(s, kRep3_6, bl);
            send_bits(s, (uint32_t)(count - 3), 2);
        } else if (count <= 10) {
            send_code(s, kRepz3_10, bl);
            send_bits(s, (uint32_t)(count - 3), 3);
        } else {
            send_code(s, kRepz11_138, bl);
            send_bits(s, (uint32_t)(count - 11), 7);
        }
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) max_count = 138, min_count = 3;
        else if (curlen == nextlen) max_count = 6, min_count = 3;
        else max_count = 7, min_count = 4;
    }
}

DF_FN uint32_t d_code(const Work* w, uint32_t dist) { return dist < 256 ? w->dist_code[dist] : w->dist_code[256 + (dist >> 7)]; }

DF_FN void compress_block(State& s, const Ct* ltree, const Ct* dtree) {
    const Work* w = s.w;
    for (uint32_t lx = 0; lx < s.last_lit; lx++) {
        uint32_t dist = w->d_buf[lx], lc = w->l_buf[lx];
        if (dist == 0) {
            send_code(s, lc, ltree);
        } else {
            uint32_t code = w->length_code[lc];
            send_code(s, code + kLiterals + 1, ltree);
            uint32_t extra = kExtraL[code];
            if (extra != 0) send_bits(s, lc - w->base_length[code], extra);
            dist--;
            code = d_code(w, dist);
            send_code(s, code, dtree);
            extra = kExtraD[code];
            if (extra != 0) send_bits(s, dist - w->base_dist[code], extra);
        }
    }
    send_code(s, kEndBlock, ltree);
}

// FLUSH_BLOCK_ONLY: _tr_flush_block over [block_start, strstart), then
// block_start = strstart
DF_FN void flush_block(State& s, int last) {
    Work* w = s.w;
    const uint64_t stored_len = (uint64_t)((int64_t)s.strstart - s.block_start);
    s.l_max_code = build_tree(s, w->dyn_ltree, w->static_ltree, kExtraL, kLiterals + 1, kLCodes, kMaxBits);
    s.d_max_code = build_tree(s, w->dyn_dtree, w->static_dtree, kExtraD, 0, kDCodes, kMaxBits);
    // build_bl_tree
    scan_tree(s, w->dyn_ltree, s.l_max_code);
    scan_tree(s, w->dyn_dtree, s.d_max_code);
    build_tree(s, w->bl_tree, nullptr, kExtraBl, 0, kBlCodes, kMaxBlBits);
    int max_blindex;
    for (max_blindex = kBlCodes - 1; max_blindex >= 3; max_blindex--)
        if (w->bl_tree[kBlOrder[max_blindex]].dl != 0) break;
    s.opt_len += 3 * ((uint64_t)max_blindex + 1) + 5 + 5 + 4;
    uint64_t opt_lenb = (s.opt_len + 3 + 7) >> 3;
    const uint64_t static_lenb = (s.static_len + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    if (stored_len + 4 <= opt_lenb && s.block_start >= 0) {
        // _tr_stored_block
        send_bits(s, (0u << 1) + (uint32_t)last, 3);
        bi_windup(s);
        s.out[s.op++] = (uint8_t)stored_len;
        s.out[s.op++] = (uint8_t)(stored_len >> 8);
        s.out[s.op++] = (uint8_t)~stored_len;
        s.out[s.op++] = (uint8_t)(~stored_len >> 8);
        const uint8_t* b = s.src + s.base + (uint64_t)s.block_start;
        for (uint64_t i = 0; i < stored_len; i++) s.out[s.op++] = b[i];
    } else if (static_lenb == opt_lenb) {
        send_bits(s, (1u << 1) + (uint32_t)last, 3);
        compress_block(s, w->static_ltree, w->static_dtree);
    } else {
        send_bits(s, (2u << 1) + (uint32_t)last, 3);
        // send_all_trees
        send_bits(s, (uint32_t)(s.l_max_code + 1 - 257), 5);
        send_bits(s, (uint32_t)(s.d_max_code + 1 - 1), 5);
        send_bits(s, (uint32_t)(max_blindex + 1 - 4), 4);
        for (int rank = 0; rank < max_blindex + 1; rank++) send_bits(s, w->bl_tree[kBlOrder[rank]].dl, 3);
        send_tree(s, w->dyn_ltree, s.l_max_code);
        send_tree(s, w->dyn_dtree, s.d_max_code);
        compress_block(s, w->dyn_ltree, w->dyn_dtree);
    }
    init_block(s);
    if (last) bi_windup(s);
    s.block_start = s.strstart;
}

DF_FN bool tally_lit(State& s, uint32_t c) {
    Work* w = s.w;
    w->d_buf[s.last_lit] = 0;
    w->l_buf[s.last_lit++] = (uint8_t)c;
    w->dyn_ltree[c].fc++;
    return s.last_lit == kLitBufsize - 1;
}
DF_FN bool tally_dist(State& s, uint32_t dist, uint32_t len) {
    Work* w = s.w;
    w->d_buf[s.last_lit] = (uint16_t)dist;
    w->l_buf[s.last_lit++] = (uint8_t)len;
    dist--;
    w->dyn_ltree[w->length_code[len] + kLiterals + 1].fc++;
    w->dyn_dtree[d_code(w, dist)].fc++;
    return s.last_lit == kLitBufsize - 1;
}

// fill_window; in_end: the end of the current fragment (avail_in = in_end - read)
DF_FN void fill_window(State& s, uint64_t in_end) {
    Work* w = s.w;
    do {
        uint32_t more = kWindowSize - s.lookahead - s.strstart;
        if (s.strstart >= kWSize + kMaxDist) {
            s.base += kWSize;
            s.match_start -= kWSize;
            s.strstart -= kWSize;
            s.block_start -= (int64_t)kWSize;
            // slide_hash
            for (uint32_t i = 0; i < kWSize; i++) {
                const uint32_t m = w->head[i];
                w->head[i] = (uint16_t)(m >= kWSize ? m - kWSize : 0);
            }
            for (uint32_t i = 0; i < kWSize; i++) {
                const uint32_t m = w->prev[i];
                w->prev[i] = (uint16_t)(m >= kWSize ? m - kWSize : 0);
            }
            more += kWSize;
        }
        if (s.read == in_end) break;
        const uint64_t avail = in_end - s.read;
        const uint32_t n = avail < more ? (uint32_t)avail : more;
        s.read += n;
        s.lookahead += n;
    } while (s.lookahead < kMinLookahead && s.read != in_end);
}

// INSERT_STRING; the string's three bytes are inside the lookahead
DF_FN uint32_t insert_string(State& s, uint32_t str) {
    Work* w = s.w;
    const uint8_t* p = s.src + s.base + str;
    const uint32_t h = (((uint32_t)p[0] << (2 * kHashShift)) ^ ((uint32_t)p[1] << kHashShift) ^ p[2]) & kHashMask;
    const uint32_t head = w->head[h];
    w->prev[str & kWMask] = (uint16_t)head;
    w->head[h] = (uint16_t)str;
    return head;
}

// longest_match.  zlib compares up to MAX_MATCH bytes, past the lookahead
// too, and clamps afterwards; nice_match <= lookahead makes the result
// independent of what lies there, so the comparison here stops at the
// lookahead.  With prev_length >= lookahead the result is the lookahead
// whatever the chain holds (and the previous match is the one emitted).
DF_FN uint32_t longest_match(State& s, uint32_t cur_match) {
    const Work* w = s.w;
    if (s.prev_length >= s.lookahead) return s.lookahead;
    uint32_t chain_length = kMaxChain;
    const uint8_t* win = s.src + s.base;
    const uint8_t* scan = win + s.strstart;
    uint32_t best_len = s.prev_length;
    uint32_t nice_match = kNiceLength;
    const uint32_t limit = s.strstart > kMaxDist ? s.strstart - kMaxDist : 0;
    const uint32_t maxlen = s.lookahead < kMaxMatch ? s.lookahead : kMaxMatch;
    uint8_t scan_end1 = scan[best_len - 1], scan_end = scan[best_len];
    if (s.prev_length >= kGoodLength) chain_length >>= 2;
    if (nice_match > s.lookahead) nice_match = s.lookahead;
    do {
        const uint8_t* match = win + cur_match;
        if (match[best_len] != scan_end || match[best_len - 1] != scan_end1 || match[0] != scan[0] || match[1] != scan[1])
            continue;
        uint32_t len = 2;
        while (len < maxlen && scan[len] == match[len]) len++;
        if (len > best_len) {
            s.match_start = cur_match;
            best_len = len;
            if (len >= nice_match) break;
            scan_end1 = scan[best_len - 1];
            scan_end = scan[best_len];
        }
    } while ((cur_match = w->prev[cur_match & kWMask]) > limit && --chain_length != 0);
    return best_len <= s.lookahead ? best_len : s.lookahead;
}

// deflate_slow over the fragment ending at in_end; finish: Z_FINISH
DF_FN void deflate_slow(State& s, uint64_t in_end, bool finish) {
    for (;;) {
        if (s.lookahead < kMinLookahead) {
            fill_window(s, in_end);
            if (s.lookahead < kMinLookahead && !finish) return;  // need_more
            if (s.lookahead == 0) break;
        }
        uint32_t hash_head = 0;
        if (s.lookahead >= kMinMatch) hash_head = insert_string(s, s.strstart);
        s.prev_length = s.match_length;
        s.prev_match = s.match_start;
        s.match_length = kMinMatch - 1;
        if (hash_head != 0 && s.prev_length < kMaxLazy && s.strstart - hash_head <= kMaxDist) {
            s.match_length = longest_match(s, hash_head);
            if (s.match_length == kMinMatch && s.strstart - s.match_start > kTooFar) s.match_length = kMinMatch - 1;
        }
        if (s.prev_length >= kMinMatch && s.match_length <= s.prev_length) {
            const uint32_t max_insert = s.strstart + s.lookahead - kMinMatch;
            const bool bflush = tally_dist(s, s.strstart - 1 - s.prev_match, s.prev_length - kMinMatch);
            s.lookahead -= s.prev_length - 1;
            s.prev_length -= 2;
            do {
                if (++s.strstart <= max_insert) insert_string(s, s.strstart);
            } while (--s.prev_length != 0);
            s.match_available = 0;
            s.match_length = kMinMatch - 1;
            s.strstart++;
            if (bflush) flush_block(s, 0);
        } else if (s.match_available) {
            if (tally_lit(s, s.src[s.base + s.strstart - 1])) flush_block(s, 0);
            s.strstart++;
            s.lookahead--;
        } else {
            s.match_available = 1;
            s.strstart++;
            s.lookahead--;
        }
    }
    if (s.match_available) {
        tally_lit(s, s.src[s.base + s.strstart - 1]);
        s.match_available = 0;
    }
    flush_block(s, 1);
}

// The gzip stream of src[0, n) fed in fragments of `frag` bytes (0: one
// fragment), into out (bound(n) bytes); returns its length.  w: kWorkBytes,
// 16-byte aligned (alignof(Work)); head_clear: the caller has zeroed w->head already.
DF_FN uint64_t gzip(const uint8_t* src, uint64_t n, uint64_t frag, uint8_t* out, Work* w, bool head_clear = false) {
    State s;
    s.w = w;
    s.src = src;
    s.out = out;
    s.op = 0;
    s.bi_buf = 0;
    s.bi_valid = 0;
    s.base = 0;
    s.read = 0;
    s.strstart = s.lookahead = s.match_start = s.prev_match = s.match_available = 0;
    s.match_length = s.prev_length = kMinMatch - 1;
    s.block_start = 0;
    s.l_max_code = s.d_max_code = 0;
    s.heap_len = s.heap_max = 0;
    if (!head_clear) {
        // head: zeros; 8 bytes per store
        uint64_t* h8 = (uint64_t*)w->head;
        for (uint32_t i = 0; i < kWSize / 4; i++) h8[i] = 0;
    }
    static_init(w);
    init_block(s);
    const uint8_t hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    for (int i = 0; i < 10; i++) out[s.op++] = hdr[i];
    if (frag == 0) frag = n ? n : 1;
    for (uint64_t f = 0; f < n; f += frag) deflate_slow(s, n - f < frag ? n : f + frag, false);
    deflate_slow(s, n, true);
    uint32_t crc = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) crc = w->crc_tab[(crc ^ src[i]) & 0xff] ^ (crc >> 8);
    crc = ~crc;
    for (int i = 0; i < 4; i++) out[s.op++] = (uint8_t)(crc >> (8 * i));
    for (int i = 0; i < 4; i++) out[s.op++] = (uint8_t)((uint32_t)n >> (8 * i));
    return s.op;
}

}  // namespace df
}  // namespace rp
