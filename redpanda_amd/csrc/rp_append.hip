// rp_append.hip — the produce path's append on the device (rpgpu_append_wire).
//
// Reference: a produce request's record set is adapted batch by batch
// (kafka_batch_adapter::adapt, kafka/protocol/kafka_batch_adapter.cc:126-188:
// the disk header of :32-91 in front of the wire payload), the partition is
// accepted or rejected (kafka/server/handlers/produce.cc:364-412), a topic
// with append time gets set_max_timestamp (produce.cc:223-232,
// model/record.h:598-608), and disk_log_appender::operator()
// (storage/disk_log_appender.cc:72-74, :113-119) assigns base_offset and
// header_crc.  Here, for every record set of a completed wire-layout job:
//
//   k_append_verdict  one thread per source batch: its verdict from the job's
//                flags; the first failing chain ordinal of each set (atomicMin)
//   k_append_sizes    one thread per source batch: is it appended (its set is
//                accepted; the produce rule takes the first batch only)?  Its
//                bytes, a count / its copy pieces, its offset step
//   (host)       exclusive scans of the three arrays: output position, output
//                ordinal / first piece, offset relative to the job's start;
//                a set's share is the difference to its first batch's value
//   k_append_plan     one thread per set: rpgpu_append_set, the output segment's
//                summary and span, the totals and the overflow verdict
//   k_append_copy     the hot path, one wave per piece of kAppendPiece payload
//                bytes: the piece's batch by bisection of the piece scan; the
//                first piece also writes the header (one lane per byte, the
//                transform of wave_header_wire, header_crc from the final
//                bytes).  The payload moves 16 bytes per lane: stores aligned
//                to the destination, loads at whatever alignment the source
//                has, the head and tail up to the 16-byte lines byte-wise, so
//                no store leaves [out_pos, out_pos + size_bytes) of its batch
//                and no load leaves the batch's own wire bytes
//   k_stamp      (rp_validate.hip) RPGPU_STAMP_CRC over the append-time
//                batches: crc over the new BE40 prefix and the payload, then
//                header_crc
//   k_append_meta     one thread per appended batch: its rpgpu_batch_result, the
//                source entry with the fields a disk-layout job over the
//                output reports differently rewritten
#include "rp_device.h"

namespace rp {

namespace {

DEV uint64_t n_batches_of(const AppendArgs& a) {
    const uint64_t n = a.job.d_totals->n_batches;
    return n < a.nb ? n : a.nb;
}
DEV bool source_overflow(const AppendArgs& a) { return a.job.d_totals->overflow != 0; }
DEV bool all_batches(const AppendArgs& a) { return (a.job.flags & RPGPU_APPEND_ALL_BATCHES) != 0; }
DEV uint32_t count_of(uint64_t packed) { return (uint32_t)packed; }
DEV uint32_t pieces_of(uint64_t packed) { return (uint32_t)(packed >> 32); }

// the order batch_reader::consume_batch (include/rpgpu_redpanda.h) follows
DEV uint32_t batch_verdict(uint32_t f) {
    if (!(f & RPGPU_F_COMPLETE)) return RPGPU_APPEND_MALFORMED;
    if (!(f & RPGPU_F_WIRE_V2)) return RPGPU_APPEND_CORRUPT_MESSAGE;
    if (!(f & RPGPU_F_CRC_OK)) return RPGPU_APPEND_CORRUPT_MESSAGE;
    if (f & RPGPU_F_CODEC_INVALID) return RPGPU_APPEND_MALFORMED;
    if (!(f & RPGPU_F_COMPRESSED) && !(f & RPGPU_F_PARSE_OK)) return RPGPU_APPEND_INVALID_RECORD;
    return RPGPU_APPEND_OK;
}

// the source batches [first, first + n) of set s, inside the job's total
struct SetRange {
    uint64_t first, n;
};
DEV SetRange set_range(const AppendArgs& a, uint32_t s, uint64_t nbt) {
    const rpgpu_segment_summary& sm = a.job.d_summaries[s];
    SetRange r;
    r.first = sm.first_batch < nbt ? sm.first_batch : nbt;
    r.n = sm.n_batches < nbt - r.first ? sm.n_batches : nbt - r.first;
    return r;
}

// the set's status and the chain ordinal that decided it
DEV uint32_t set_status(const AppendArgs& a, uint32_t s, const SetRange& r, uint32_t& first_bad) {
    const uint32_t bad = a.seg_bad[s];
    if (!all_batches(a)) {
        first_bad = 0;
        if (r.n == 0) return RPGPU_APPEND_MALFORMED;
        if (bad == 0) return a.verdict[r.first];
        first_bad = (uint32_t)r.n;
        return RPGPU_APPEND_OK;
    }
    if (bad < r.n) {
        first_bad = bad;
        return a.verdict[r.first + bad];
    }
    first_bad = (uint32_t)r.n;
    return a.job.d_summaries[s].terminal_errc == RPGPU_ERRC_END_OF_STREAM ? RPGPU_APPEND_OK : RPGPU_APPEND_MALFORMED;
}

// set_max_timestamp applies to set s
DEV bool append_time_of(const AppendArgs& a, uint32_t s, int64_t& t) {
    if (!a.job.d_append_time) return false;
    t = a.job.d_append_time[s];
    return t != RPGPU_APPEND_CREATE_TIME;
}

}  // namespace

__global__ __launch_bounds__(256) void k_append_verdict(AppendArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nb) return;
    uint32_t v = RPGPU_APPEND_OK;
    if (b < n_batches_of(a) && !source_overflow(a)) {
        const rpgpu_batch_result& R = a.job.d_batches[b];
        v = batch_verdict(R.flags);
        const uint32_t seg = R.segment;
        if (v != RPGPU_APPEND_OK && seg < a.job.n_segments) {
            const uint64_t ord = b - a.job.d_summaries[seg].first_batch;
            if (ord == 0 || (all_batches(a) && ord < 0xFFFFFFFFull)) atomicMin(&a.seg_bad[seg], (uint32_t)ord);
        }
    }
    a.verdict[b] = v;
}

__global__ __launch_bounds__(256) void k_append_sizes(AppendArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nb) return;
    uint64_t size = 0, cnt = 0, step = 0;
    const uint64_t nbt = n_batches_of(a);
    if (b < nbt && !source_overflow(a)) {
        const rpgpu_batch_result& R = a.job.d_batches[b];
        const uint32_t seg = R.segment;
        if (seg < a.job.n_segments) {
            const SetRange r = set_range(a, seg, nbt);
            const uint64_t ord = b - r.first;
            uint32_t fb;
            if (ord < r.n && (ord == 0 || all_batches(a)) && set_status(a, seg, r, fb) == RPGPU_APPEND_OK) {
                size = (uint32_t)R.size_bytes;
                const uint64_t plen = size - RPGPU_HEADER_SIZE;
                const uint64_t pieces = plen ? (plen + kAppendPiece - 1) / kAppendPiece : 1;
                cnt = 1ull | (pieces << 32);
                // disk_log_appender.cc:113-119: the appender moves on to last_offset + 1
                step = (uint64_t)((int64_t)R.last_offset_delta + 1);
            }
        }
    }
    a.bpos[b] = size;
    a.bcnt[b] = cnt;
    a.bstep[b] = step;
}

// after the scans: bpos[b] / bcnt[b] / bstep[b] = output position, output
// ordinal and first piece, offset from the job's first batch; [nb] the totals
__global__ __launch_bounds__(256) void k_append_plan(AppendArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    rpgpu_append_totals* T = a.job.d_atotals;
    if (s == 0) {
        const uint64_t bytes = a.bpos[a.nb], nout = count_of(a.bcnt[a.nb]);
        T->batches_out = nout;
        T->bytes_out = bytes;
        T->out_capacity_needed = bytes + 16;
        T->out_batch_capacity_needed = nout;
        T->overflow = (bytes + 16 > a.job.out_capacity ? 1u : 0u) | (nout > a.job.out_batch_capacity ? 2u : 0u);
        a.job.d_out_seg_offsets[a.job.n_segments] = bytes;
    }
    if (s >= a.job.n_segments) return;
    const bool sov = source_overflow(a);
    SetRange r;
    r.first = r.n = 0;
    if (!sov) r = set_range(a, s, n_batches_of(a));
    uint32_t first_bad = 0;
    const uint32_t status = sov ? (uint32_t)RPGPU_APPEND_SOURCE_OVERFLOW : set_status(a, s, r, first_bad);
    const uint64_t o0 = a.bpos[r.first], bytes = a.bpos[r.first + r.n] - o0;
    const uint64_t c0 = count_of(a.bcnt[r.first]), n = count_of(a.bcnt[r.first + r.n]) - c0;
    const uint64_t steps = a.bstep[r.first + r.n] - a.bstep[r.first];
    const int64_t next = a.job.d_next_offset[s];
    rpgpu_append_set g;
    g.status = status;
    g.first_bad = first_bad;
    g.n_batches = n;
    g.base_offset = next;
    g.last_offset = (int64_t)((uint64_t)next + steps - 1);
    g.bytes_out = bytes;
    a.job.d_sets[s] = g;
    a.job.d_out_seg_offsets[s] = o0;
    // what a disk-layout job reports for a clean segment of n batches
    // (continuous_batch_parser ran to the end of the stream; the
    // checksumming_consumer checkpoint is the last batch)
    rpgpu_segment_summary m;
    m.first_batch = c0;
    m.n_batches = n;
    m.terminal_pos = bytes;
    m.bytes_consumed = bytes;
    m.terminal_errc = RPGPU_ERRC_END_OF_STREAM;
    m.terminal_eof = 1;
    m.has_checkpoint = n ? 1 : 0;
    m.first_bad = (uint32_t)n;
    m.ckpt_last_offset = n ? g.last_offset : 0;
    m.ckpt_truncate_pos = n ? bytes : 0;
    m.n_records = 0;
    m.reserved[0] = m.reserved[1] = 0;
    a.job.d_out_summaries[s] = m;
    if (status == RPGPU_APPEND_OK) atomicAdd((unsigned long long*)&T->sets_ok, 1ull);
}

__global__ __launch_bounds__(256) void k_append_copy(AppendArgs a) {
    const uint32_t l = lane();
    const uint64_t total = a.bcnt[a.nb];
    if (a.bpos[a.nb] + 16 > a.job.out_capacity || count_of(total) > a.job.out_batch_capacity) return;
    const uint32_t npieces = pieces_of(total);
    const Tables* __restrict__ T = a.tables;
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
        const uint32_t seg = uni32(R.segment), size = uni32((uint32_t)R.size_bytes);
        const uint32_t plen = size - RPGPU_HEADER_SIZE;
        const uint64_t op = uni64(a.bpos[b]);
        const uint8_t* __restrict__ src = a.job.d_data + uni64(a.job.d_seg_offsets[seg]) + uni64(R.file_pos);
        uint8_t* __restrict__ dst = a.job.d_out + op;
        if (k == 0) {
            const uint64_t first = a.job.d_summaries[seg].first_batch;
            const uint64_t bo = uni64((uint64_t)a.job.d_next_offset[seg] + (a.bstep[b] - a.bstep[first]));
            int64_t t = 0;
            const bool stamped = append_time_of(a, seg, t);
            // disk byte l from wire byte `from` (wave_header_wire, rp_device.h):
            // size_bytes 4..7, base_offset 8..15, type 16, crc and the fields
            // from attrs on byte-reversed in place
            const uint32_t wb = l < RPGPU_HEADER_SIZE ? (uint32_t)src[l] : 0u;
            int from = 0;
            if (l >= 17 && l < 21) from = 37 - (int)l;
            else if (l >= 21 && l < RPGPU_HEADER_SIZE) from = 21 + be_index(l);
            uint32_t d = (uint32_t)__shfl((int)wb, from, 64);
            if (l >= 4 && l < 8) d = (size >> (8 * (l - 4))) & 0xFFu;
            if (l >= 8 && l < 16) d = (uint32_t)(bo >> (8 * (l - 8))) & 0xFFu;
            if (l == 16) d = 1u;  // model::record_batch_type::raft_data
            if (stamped) {        // set_max_timestamp (model/record.h:598-608); crc follows in k_stamp
                if (l == 21) d |= 8u;
                if (l >= 35 && l < 43) d = (uint32_t)((uint64_t)t >> (8 * (l - 35))) & 0xFFu;
            }
            const uint32_t contrib = (l >= 4 && l < RPGPU_HEADER_SIZE) ? T->hdr[60 - l][d] : 0u;
            const uint32_t hc = ~(T->c57 ^ wave_xor(contrib));
            if (l < 4) d = (hc >> (8 * l)) & 0xFFu;
            if (l < RPGPU_HEADER_SIZE) dst[l] = (uint8_t)d;
            if (stamped && l == 0) {
                const uint32_t i = atomicAdd(&a.counters[kAcStampCount], 1u);
                a.spos[i] = op;
                a.splen[i] = plen;
            }
        }
        const uint32_t p0 = k * kAppendPiece;
        const uint32_t n = plen - p0 < kAppendPiece ? plen - p0 : kAppendPiece;
        wave_copy_lines(dst + RPGPU_HEADER_SIZE + p0, src + RPGPU_HEADER_SIZE + p0, n, l);
    }
}

__global__ __launch_bounds__(256) void k_append_meta(AppendArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nb) return;
    const uint64_t total = a.bcnt[a.nb];
    if (a.bpos[a.nb] + 16 > a.job.out_capacity || count_of(total) > a.job.out_batch_capacity) return;
    const uint64_t op = a.bpos[b];
    if (a.bpos[b + 1] == op) return;  // not appended
    rpgpu_batch_result e = a.job.d_batches[b];
    const uint32_t seg = e.segment;
    const uint64_t first = a.job.d_summaries[seg].first_batch;
    const uint8_t* h = a.job.d_out + op;
    const uint32_t hc = (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16) | ((uint32_t)h[3] << 24);
    e.file_pos = op - a.bpos[first];
    e.base_offset = (int64_t)((uint64_t)a.job.d_next_offset[seg] + (a.bstep[b] - a.bstep[first]));
    e.header_crc = hc;
    e.header_crc_computed = hc;
    e.flags &= ~RPGPU_F_WIRE_V2;
    e.decoded_crc = 0;
    e.decoded_header_crc = 0;
    int64_t t = 0;
    if (append_time_of(a, seg, t)) {
        const uint32_t crc = (uint32_t)h[17] | ((uint32_t)h[18] << 8) | ((uint32_t)h[19] << 16) | ((uint32_t)h[20] << 24);
        e.attrs = (int16_t)((uint16_t)e.attrs | 8u);
        e.max_timestamp = t;
        e.crc = crc;
        e.crc_computed = crc;
    }
    e.reserved0 = 0;
    e.reserved1 = 0;
    a.job.d_out_batches[count_of(a.bcnt[b])] = e;
}

static uint32_t thread_grid(uint64_t items) { return (uint32_t)(items ? (items + 255) / 256 : 1); }

hipError_t launch_append_sizes(const AppendArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_append_verdict, dim3(thread_grid(a.nb)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_append_sizes, dim3(thread_grid(a.nb)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_append_plan(const AppendArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_append_plan, dim3(thread_grid(a.job.n_segments)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_append_copy(const AppendArgs& a, uint32_t cus, hipStream_t s) {
    // the piece count lives on the device: the bound the host knows is one
    // piece per batch plus one per kAppendPiece bytes of output capacity
    const uint64_t pieces = a.nb + a.job.out_capacity / kAppendPiece;
    const uint64_t blocks = (pieces + 3) / 4, cap = (uint64_t)cus * 8;
    hipLaunchKernelGGL(k_append_copy, dim3((uint32_t)(blocks < 1 ? 1 : blocks < cap ? blocks : cap)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_append_meta(const AppendArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_append_meta, dim3(thread_grid(a.nb)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rp
