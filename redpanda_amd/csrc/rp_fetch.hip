// rp_fetch.hip — the fetch path's log read on the device (rpgpu_fetch).
//
// Reference: a Kafka fetch makes a storage::log_reader over the partition's
// segments, driven by skipping_consumer (storage/log_reader.cc:26-119,
// :212-343) under a log_reader_config (storage/types.h:201-270), and folds the
// accepted batches through kafka_batch_serializer (kafka/protocol/
// batch_consumer.h:27-78) into the partition's wire record set
// (kafka/server/handlers/fetch.cc:128-173).  Here, for every partition of a
// completed disk-layout job (the read rule is spelled out in include/rpgpu.h):
//
//   k_fetch_select    one wave per partition: its segments in order, 64 chain
//                batches per turn.  Each lane evaluates the stateless tests of
//                one batch; the coupled state (start, expected, consumed) is
//                resolved across the wave: start is a prefix maximum of
//                last_offset + 1, consumed a prefix sum of the accepted sizes,
//                expected the previous lane's last_offset + 1; the turn's first
//                stopping lane ends the read.  Per returned batch: its bytes,
//                a count / its copy pieces, its record count, its partition
//   (host)       exclusive scans of the three arrays: output position, output
//                ordinal / first piece, records; a partition's share is the
//                difference to the value at its first batch
//   k_fetch_plan      one thread per partition: rpgpu_fetch_part, its output
//                span, the totals and the overflow verdict
//   k_fetch_copy      the hot path, one wave per piece of kAppendPiece payload
//                bytes: the piece's batch by bisection of the piece scan; the
//                first piece also writes the wire header (one lane per byte,
//                k_to_wire's transform) and the batch's rpgpu_fetch_batch.
//                The payload moves as in k_append_copy (wave_copy_lines): no
//                store leaves [out_pos, out_pos + size_bytes) of its batch and
//                no load leaves the batch's own bytes
#include "rp_device.h"

namespace rp {

namespace {

constexpr int64_t kI64Min = (int64_t)0x8000000000000000ull;
constexpr int64_t kI64Max = 0x7FFFFFFFFFFFFFFFll;

DEV uint64_t n_batches_of(const FetchArgs& a) {
    const uint64_t n = a.job.d_totals->n_batches;
    return n < a.nb ? n : a.nb;
}
DEV bool source_overflow(const FetchArgs& a) { return a.job.d_totals->overflow != 0; }
DEV uint32_t count_of(uint64_t packed) { return (uint32_t)packed; }
DEV uint32_t pieces_of(uint64_t packed) { return (uint32_t)(packed >> 32); }
DEV int64_t add_wrap(int64_t x, int64_t y) { return (int64_t)((uint64_t)x + (uint64_t)y); }

// the bytes a returned batch takes in the output: its size_bytes; a complete
// batch below 61 would need a segment of 4 GiB, it counts as a bare header
DEV uint32_t out_size(int32_t size_bytes) {
    return (uint32_t)size_bytes < RPGPU_HEADER_SIZE ? RPGPU_HEADER_SIZE : (uint32_t)size_bytes;
}

// the job's segments [s0, s1) of partition p and their batches [first, end)
struct PartRange {
    uint32_t s0, s1;
    uint64_t first, end;
};
DEV PartRange part_range(const FetchArgs& a, uint32_t p, uint64_t nbt) {
    const uint32_t nseg = a.job.n_segments;
    PartRange r;
    const uint32_t x = a.job.d_part_segments[p], y = a.job.d_part_segments[p + 1];
    r.s0 = x < nseg ? x : nseg;
    r.s1 = y < r.s0 ? r.s0 : y < nseg ? y : nseg;
    uint64_t f = r.s0 < nseg ? a.job.d_summaries[r.s0].first_batch : nbt;
    uint64_t e = r.s1 < nseg ? a.job.d_summaries[r.s1].first_batch : nbt;
    r.first = f < nbt ? f : nbt;
    e = e < nbt ? e : nbt;
    r.end = e < r.first ? r.first : e;
    return r;
}

DEV int64_t shfl64(int64_t v, uint32_t src) { return (int64_t)__shfl((long long)v, (int)src, 64); }
DEV int64_t shfl_up64(int64_t v, uint32_t d) { return (int64_t)__shfl_up((long long)v, d, 64); }

// sum of v over the lanes below this one
DEV uint64_t wave_exclusive_sum(uint64_t v, uint32_t l) {
    uint64_t x = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint64_t y = (uint64_t)shfl_up64((int64_t)x, o);
        if (l >= o) x += y;
    }
    return x - v;
}
// max of seed and of v over the lanes below this one
DEV int64_t wave_exclusive_max(int64_t v, int64_t seed, uint32_t l) {
    int64_t x = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const int64_t y = shfl_up64(x, o);
        if (l >= o && y > x) x = y;
    }
    const int64_t below = shfl_up64(x, 1);
    return (l == 0 || below < seed) ? seed : below;
}

// one partition's request and the state of its read (wave-uniform)
struct Read {
    int64_t start, expected, max_offset, first_ts;
    uint64_t consumed, max_bytes;
    int32_t type;
    bool strict, by_type, by_time;
    bool over, ended;
    uint32_t status;
};

// where the consumer enters a segment's chain [first, first + n): the chain
// ordinal of segment_index::find_nearest(start)'s batch (rpgpu.h, step 4)
DEV uint64_t entry_of(const FetchArgs& a, uint32_t seg, uint64_t first, uint64_t n, int64_t start) {
    if (!a.job.d_index_states) return 0;
    const rpgpu_index_state& st = a.job.d_index_states[seg];
    const uint64_t fe = st.first_entry;
    if (fe >= a.nb) return 0;
    const uint64_t ne = st.n_entries < a.nb - fe ? st.n_entries : a.nb - fe;
    if (start < st.base_offset || ne == 0) return 0;
    const uint32_t needle = (uint32_t)((uint64_t)start - (uint64_t)st.base_offset);
    const uint32_t* __restrict__ rel = a.job.d_rel_offset + fe;
    uint64_t lo = 0, len = ne;  // std::lower_bound
    while (len) {
        const uint64_t half = len >> 1;
        if (rel[lo + half] < needle) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    uint64_t i = lo == ne ? ne - 1 : lo;
    for (;;) {
        if (rel[i] <= needle) break;
        if (i == 0) return 0;  // no entry: position 0
        i--;
    }
    const uint64_t pos = a.job.d_position[fe + i];
    uint64_t b = 0, e = n;  // the first chain batch with file_pos >= pos
    while (b < e) {
        const uint64_t mid = b + (e - b) / 2;
        if (a.job.d_batches[first + mid].file_pos < pos) b = mid + 1;
        else e = mid;
    }
    return b;
}

}  // namespace

__global__ __launch_bounds__(256) void k_fetch_select(FetchArgs a) {
    const uint32_t l = lane();
    const uint32_t waves = gridDim.x * 4;
    const uint64_t nbt = n_batches_of(a);
    const bool sov = source_overflow(a);
    for (uint32_t p = uni32(blockIdx.x * 4 + (threadIdx.x >> 6)); p < a.job.n_partitions; p += waves) {
        const rpgpu_fetch_request q = a.job.d_requests[p];
        Read r;
        r.start = q.start_offset;
        r.expected = kI64Min;
        r.max_offset = q.max_offset;
        r.first_ts = q.first_timestamp;
        r.consumed = 0;
        r.max_bytes = q.max_bytes;
        r.type = q.type_filter;
        r.strict = (q.flags & RPGPU_FETCH_STRICT_MAX_BYTES) != 0;
        r.by_type = (q.flags & RPGPU_FETCH_TYPE_FILTER) != 0;
        r.by_time = (q.flags & RPGPU_FETCH_FIRST_TIMESTAMP) != 0;
        r.over = false;
        r.ended = sov;
        r.status = sov ? (uint32_t)RPGPU_FETCH_SOURCE_OVERFLOW : (uint32_t)RPGPU_FETCH_OK;
        int64_t out_base = kI64Min, out_last = kI64Min, out_ts = -1;
        int64_t bad_expected = 0, bad_actual = 0;  // RPGPU_FETCH_OFFSETS: the two offsets the reference's message names
        bool any = false;
        PartRange pr;
        pr.s0 = pr.s1 = 0;
        pr.first = pr.end = 0;
        if (!sov) pr = part_range(a, p, nbt);
        for (uint32_t seg = pr.s0; seg < pr.s1 && !r.ended; seg++) {
            const rpgpu_segment_summary& sm = a.job.d_summaries[seg];
            const uint64_t first = uni64(sm.first_batch < nbt ? sm.first_batch : nbt);
            uint64_t n = uni64(sm.n_batches < nbt - first ? sm.n_batches : nbt - first);
            if (n && !(a.job.d_batches[first + n - 1].flags & RPGPU_F_COMPLETE)) n--;
            if (n == 0) continue;
            const rpgpu_batch_result& E = a.job.d_batches[first + n - 1];
            const int64_t dirty = add_wrap(E.base_offset, (int64_t)E.last_offset_delta);
            if (r.start > dirty) continue;
            r.expected = kI64Min;
            for (uint64_t i0 = uni64(entry_of(a, seg, first, n, r.start)); i0 < n && !r.ended; i0 += 64) {
                const uint64_t b = first + i0 + l;
                const bool valid = i0 + l < n;
                int64_t base = 0, fts = 0, last = kI64Min;
                uint64_t size = 0;
                int32_t type = 0, size_bytes = 0, rc = 0;
                if (valid) {
                    const rpgpu_batch_result& R = a.job.d_batches[b];
                    base = R.base_offset;
                    fts = R.first_timestamp;
                    size_bytes = R.size_bytes;
                    rc = R.record_count;
                    type = R.type;
                    size = (uint64_t)(int64_t)size_bytes;
                    last = add_wrap(base, (int64_t)R.last_offset_delta);
                }
                const int64_t nxt = add_wrap(last, 1);
                const uint32_t cnt = (uint32_t)(n - i0 < 64 ? n - i0 : 64);
                const bool filtered = (r.by_type && type != r.type) || (r.by_time && r.first_ts > fts);
                uint64_t accmask = 0;
                if (__ballot(valid && last == kI64Max)) {
                    // last_offset + 1 wraps in this turn, start is no prefix
                    // maximum: the rules one batch at a time, every lane alike
                    for (uint32_t j = 0; j < cnt && !r.ended; j++) {
                        const int64_t jb = shfl64(base, j), jl = shfl64(last, j), jn = shfl64(nxt, j);
                        const uint64_t js = (uint64_t)shfl64((int64_t)size, j);
                        const bool jf = __shfl((int)filtered, (int)j, 64) != 0;
                        if (jb < r.expected) {
                            r.status = RPGPU_FETCH_OFFSETS;
                            bad_expected = r.expected;
                            bad_actual = jb;
                            r.ended = true;
                        } else if (jb > r.max_offset) {
                            r.ended = true;
                        } else if ((r.strict || r.consumed != 0) && r.consumed + js > r.max_bytes) {
                            r.over = true;
                            r.ended = true;
                        } else if (jl < r.start) {
                            r.expected = jn;
                        } else if (jf) {
                            r.start = r.expected = jn;
                        } else {
                            accmask |= 1ull << j;
                            r.start = r.expected = jn;
                            r.consumed += js;
                            if (jl >= r.max_offset || r.consumed > r.max_bytes) r.ended = true;
                        }
                    }
                } else {
                    const int64_t below_nxt = shfl_up64(nxt, 1);
                    const int64_t exp_l = l == 0 ? r.expected : below_nxt;
                    const int64_t start_l = wave_exclusive_max(valid ? nxt : kI64Min, r.start, l);
                    const bool below = last < start_l;
                    const bool acc = valid && !below && !filtered;
                    const uint64_t cons_l = r.consumed + wave_exclusive_sum(acc ? size : 0, l);
                    const bool v1 = base < exp_l, v2 = base > r.max_offset;
                    const bool v3 = (r.strict || cons_l != 0) && cons_l + size > r.max_bytes;
                    const bool pre = valid && (v1 || v2 || v3);
                    const bool post = acc && !pre && (last >= r.max_offset || cons_l + size > r.max_bytes);
                    const uint64_t stops = __ballot(pre || post);
                    const uint32_t at = stops ? (uint32_t)__builtin_ctzll(stops) : cnt - 1;
                    const uint64_t upto = at == 63 ? ~0ull : (1ull << (at + 1)) - 1;
                    accmask = __ballot(acc && !pre) & upto;
                    // the state behind lane `at`: the stopping lane, or the turn's last
                    const bool at_pre = __shfl((int)pre, (int)at, 64) != 0;
                    const int64_t s_after = (pre || below) ? start_l : nxt;
                    const uint64_t c_after = cons_l + ((acc && !pre) ? size : 0);
                    r.start = shfl64(s_after, at);
                    r.consumed = (uint64_t)shfl64((int64_t)c_after, at);
                    r.expected = shfl64(nxt, at);
                    if (stops) {
                        r.ended = true;
                        if (at_pre) {
                            const bool at_v1 = __shfl((int)v1, (int)at, 64) != 0, at_v2 = __shfl((int)v2, (int)at, 64) != 0;
                            if (at_v1) {
                                r.status = RPGPU_FETCH_OFFSETS;
                                bad_expected = shfl64(exp_l, at);
                                bad_actual = shfl64(base, at);
                            } else if (!at_v2) {
                                r.over = true;
                            }
                        }
                    }
                }
                if (accmask) {
                    const uint32_t lo = (uint32_t)__builtin_ctzll(accmask), hi = 63u - (uint32_t)__builtin_clzll(accmask);
                    if (!any) {
                        out_base = shfl64(base, lo);
                        out_ts = shfl64(fts, lo);
                        any = true;
                    }
                    out_last = shfl64(last, hi);
                    if ((accmask >> l) & 1) {
                        const uint32_t sz = out_size(size_bytes);
                        const uint64_t plen = sz - RPGPU_HEADER_SIZE;
                        const uint64_t pieces = plen ? (plen + kAppendPiece - 1) / kAppendPiece : 1;
                        a.bpos[b] = sz;
                        a.bcnt[b] = 1ull | (pieces << 32);
                        a.brec[b] = (uint32_t)rc;
                        a.bpart[b] = p;
                    }
                }
            }
        }
        if (r.status == RPGPU_FETCH_OFFSETS) {
            // the reference throws: nothing of the partition is returned
            __threadfence();
            for (uint64_t b = pr.first + l; b < pr.end; b += 64) a.bpos[b] = a.bcnt[b] = a.brec[b] = 0;
            out_base = bad_expected;
            out_last = bad_actual;
            out_ts = -1;
        }
        if (l == 0) {
            FetchSel s;
            s.status = r.status;
            s.over_budget = r.over ? 1u : 0u;
            s.base_offset = out_base;
            s.last_offset = out_last;
            s.next_offset = r.start;
            s.first_timestamp = out_ts;
            a.sel[p] = s;
        }
    }
}

// after the scans: bpos[b] / bcnt[b] / brec[b] = output position, output
// ordinal and first piece, records before batch b; [nb] the totals
__global__ __launch_bounds__(256) void k_fetch_plan(FetchArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    rpgpu_fetch_totals* T = a.job.d_ftotals;
    if (p == 0) {
        const uint64_t bytes = a.bpos[a.nb], nout = count_of(a.bcnt[a.nb]);
        T->batches_out = nout;
        T->bytes_out = bytes;
        T->out_capacity_needed = bytes + 16;
        T->out_batch_capacity_needed = nout;
        T->overflow = (bytes + 16 > a.job.out_capacity ? 1u : 0u) | (nout > a.job.out_batch_capacity ? 2u : 0u);
        a.job.d_out_part_offsets[a.job.n_partitions] = bytes;
    }
    if (p >= a.job.n_partitions) return;
    PartRange r;
    r.s0 = r.s1 = 0;
    r.first = r.end = 0;
    if (!source_overflow(a)) r = part_range(a, p, n_batches_of(a));
    const FetchSel s = a.sel[p];
    const uint64_t o0 = a.bpos[r.first], c0 = count_of(a.bcnt[r.first]);
    rpgpu_fetch_part g;
    g.status = s.status;
    g.over_budget = s.over_budget;
    g.n_batches = count_of(a.bcnt[r.end]) - c0;
    g.first_out = (uint32_t)c0;
    g.record_count = (uint32_t)(a.brec[r.end] - a.brec[r.first]);
    g.bytes_out = a.bpos[r.end] - o0;
    g.base_offset = s.base_offset;
    g.last_offset = s.last_offset;
    g.next_offset = s.next_offset;
    g.first_timestamp = s.first_timestamp;
    a.job.d_parts[p] = g;
    a.job.d_out_part_offsets[p] = o0;
    if (s.status == RPGPU_FETCH_OK) atomicAdd((unsigned long long*)&T->parts_ok, 1ull);
}

__global__ __launch_bounds__(256) void k_fetch_copy(FetchArgs a) {
    const uint32_t l = lane();
    const uint64_t total = a.bcnt[a.nb];
    if (a.bpos[a.nb] + 16 > a.job.out_capacity || count_of(total) > a.job.out_batch_capacity) return;
    const uint32_t npieces = pieces_of(total);
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
        const rpgpu_batch_result& R = a.job.d_batches[b];
        const uint32_t seg = uni32(R.segment), size = uni32(out_size(R.size_bytes));
        const uint32_t plen = size - RPGPU_HEADER_SIZE;
        const uint64_t op = uni64(a.bpos[b]);
        const uint8_t* __restrict__ src = a.job.d_data + uni64(a.job.d_seg_offsets[seg]) + uni64(R.file_pos);
        uint8_t* __restrict__ dst = a.job.d_out + op;
        if (k == 0) {
            // wire byte l from disk byte `from`, reversed within each field
            // (k_to_wire, rp_validate.hip): base_offset 0..7, batch_length
            // 8..11 = size_bytes - 12, partition leader epoch 0, magic 2, crc
            // 17..20, attrs .. record_count (the BE40 prefix) 21..60
            const uint32_t db = l < RPGPU_HEADER_SIZE ? (uint32_t)src[l] : 0u;
            const uint32_t blen = size - 12u;
            int from = -1;
            uint32_t wb = 0;
            if (l < 8) from = 15 - (int)l;
            else if (l < 12) wb = (blen >> (8 * (11 - l))) & 0xFFu;
            else if (l < 16) wb = 0;
            else if (l == 16) wb = 2;
            else if (l < 21) from = 37 - (int)l;
            else if (l < RPGPU_HEADER_SIZE) from = 21 + be_index(l);
            const uint32_t v = (uint32_t)__shfl((int)db, from < 0 ? 0 : from, 64);
            if (from >= 0) wb = v;
            if (l < RPGPU_HEADER_SIZE) dst[l] = (uint8_t)wb;
            if (l == 0) {
                rpgpu_fetch_batch e;
                e.out_pos = op;
                e.src_batch = (uint32_t)b;
                e.partition = a.bpart[b];
                a.job.d_out_batches[count_of(a.bcnt[b])] = e;
            }
        }
        const uint32_t p0 = k * kAppendPiece;
        const uint32_t n = plen - p0 < kAppendPiece ? plen - p0 : kAppendPiece;
        wave_copy_lines(dst + RPGPU_HEADER_SIZE + p0, src + RPGPU_HEADER_SIZE + p0, n, l);
    }
}

hipError_t launch_fetch_select(const FetchArgs& a, hipStream_t s) {
    const uint32_t np = a.job.n_partitions;
    hipLaunchKernelGGL(k_fetch_select, dim3(np ? (np + 3) / 4 : 1), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_fetch_plan(const FetchArgs& a, hipStream_t s) {
    const uint32_t np = a.job.n_partitions;
    hipLaunchKernelGGL(k_fetch_plan, dim3(np ? (np + 255) / 256 : 1), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_fetch_copy(const FetchArgs& a, uint32_t cus, hipStream_t s) {
    // the piece count lives on the device: the bound the host knows is one
    // piece per batch plus one per kAppendPiece bytes of output capacity
    const uint64_t pieces = a.nb + a.job.out_capacity / kAppendPiece;
    const uint64_t blocks = (pieces + 3) / 4, cap = (uint64_t)cus * 8;
    hipLaunchKernelGGL(k_fetch_copy, dim3((uint32_t)(blocks < 1 ? 1 : blocks < cap ? blocks : cap)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rp
