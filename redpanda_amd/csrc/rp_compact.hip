// rp_compact.hip — key compaction of segments on the device (rpgpu_compact).
//
// Reference: self_compact_segment (storage/segment_utils.cc:306-365) runs
// three reducers over a segment and its compaction index:
//   compaction_key_reducer         (compaction_reducers.cc:34-83): per key the
//                                  entry with the highest offset survives;
//   compacted_offset_list_reducer  (:108-114): the surviving offsets;
//   copy_data_segment_reducer      (:116-222): every batch filtered by that
//                                  list, partly kept batches re-encoded with
//                                  model::append_record_to_buffer
//                                  (model/record_utils.cc:183-225).
// Here the inputs are the outputs of a CRC | PARSE | DECODE job: the record
// index names every key, the decoded arena holds compressed payloads.
//
// Launches (one stream, in order):
//   k_cinit      per segment: job-level eligibility, accumulators zeroed
//   k_celig      one wave per batch: verdict flags, strictly increasing record
//                offsets (each record against the previous index slot)
//   k_cinsert    one wave per batch of an eligible segment, one record per
//                lane: open-addressing key table, word = tag << 32 | slot + 1;
//                empty words are claimed by CAS, a tag match is settled by
//                comparing the key bytes, equal keys fetch_max the word.
//                Every table access is an agent-scope 8-byte atomic (a plain
//                load could return another XCD's stale line).  Keys above
//                kLaneKey bytes are hashed and compared by the whole wave.
//   k_ckeep      table words -> keep bitmap (a launch of its own, so the
//                table is complete and visible)
//   k_csize      one wave per batch: kept count, output payload bytes (the
//                re-encoded sizes of the kept records when partly kept)
//   (two exclusive scans: output position and output ordinal per batch)
//   k_cplan      per segment: result entry, output offsets; totals, overflow
//   k_cwrite     one wave per output batch: header fields, then the payload:
//                verbatim, or the kept records, runs of adjacent canonically
//                encoded ones as one 16-B-per-lane copy, the others re-encoded
//                by their lane
//   k_stamp      (rp_validate.hip) RPGPU_STAMP_CRC: size, crc, header_crc
#include "rp_device.h"

namespace rp {

namespace {

constexpr uint32_t kLaneKey = 256;  // longer keys take the wave path
constexpr uint32_t kElig = RPGPU_F_HEADER_OK | RPGPU_F_COMPLETE | RPGPU_F_CRC_OK | RPGPU_F_PARSED | RPGPU_F_PARSE_OK |
                           RPGPU_F_INDEX_WRITTEN;

#define AGENT_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

DEV uint64_t n_batches_of(const CompactArgs& a) {
    const uint64_t n = a.job.d_totals->n_batches;
    return n < a.nb ? n : a.nb;
}
DEV uint64_t n_records_of(const CompactArgs& a) {
    const uint64_t n = a.job.d_totals->n_records;
    return n < a.nr ? n : a.nr;
}

// the (decoded) payload of a batch of an eligible segment
DEV const uint8_t* payload_of(const CompactArgs& a, const rpgpu_batch_result& B) {
    if (B.flags & RPGPU_F_COMPRESSED) return a.job.d_decoded + B.decoded_off;
    return a.job.d_data + a.job.d_seg_offsets[B.segment] + B.file_pos + RPGPU_HEADER_SIZE;
}

// the compaction key of a record: its first min(key_len, 65515) key bytes
// (never past the record's end: iobuf_copy stops at the end of the payload)
DEV uint32_t key_len_of(const rpgpu_record_index& r) {
    if (r.key_len <= 0 || r.end_pos <= r.key_pos) return 0;
    uint32_t n = (uint32_t)r.key_len;
    if (n > r.end_pos - r.key_pos) n = r.end_pos - r.key_pos;
    return n < RPGPU_COMPACT_MAX_KEY ? n : RPGPU_COMPACT_MAX_KEY;
}

DEV uint32_t ld32u(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

DEV uint64_t mix64(uint64_t h, uint64_t w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
DEV uint64_t fin64(uint64_t h, uint32_t seg, uint32_t len) {
    h = mix64(h, ((uint64_t)seg << 32) | len);
    h *= 0xC2B2AE3D27D4EB4Full;
    return h ^ (h >> 32);
}

// one lane hashes a short key
DEV uint64_t hash_lane(const uint8_t* k, uint32_t n, uint32_t seg) {
    uint64_t h = 0x2545F4914F6CDD1Dull;
    uint32_t i = 0;
    for (; i + 4 <= n; i += 4) h = mix64(h, ld32u(k + i));
    uint32_t t = 0;
    for (uint32_t s = 0; i < n; i++, s += 8) t |= (uint32_t)k[i] << s;
    return fin64(mix64(h, t), seg, n);
}
DEV bool equal_lane(const uint8_t* a, const uint8_t* b, uint32_t n) {
    uint32_t i = 0;
    for (; i + 4 <= n; i += 4)
        if (ld32u(a + i) != ld32u(b + i)) return false;
    for (; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

// the wave hashes a long key: lane l takes the dwords l, l + 64, ...; the
// lanes' states are folded with their lane number.  A key's length decides
// which of the two hashes it gets, so equal keys always get the same one.
DEV uint64_t hash_wave(const uint8_t* k, uint32_t n, uint32_t seg) {
    const uint32_t l = lane();
    uint64_t h = 0x2545F4914F6CDD1Dull + l;
    const uint32_t words = n >> 2;
    for (uint32_t w = l; w < words; w += 64) h = mix64(h, ld32u(k + 4 * w));
    if (l == 0) {
        uint32_t t = 0;
        for (uint32_t i = words * 4, s = 0; i < n; i++, s += 8) t |= (uint32_t)k[i] << s;
        h = mix64(h, t);
    }
    h *= 0xC2B2AE3D27D4EB4Full;
    const uint32_t lo = wave_xor((uint32_t)h), hi = wave_xor((uint32_t)(h >> 32));
    return fin64(((uint64_t)hi << 32) | lo, seg, n);
}
DEV bool equal_wave(const uint8_t* a, const uint8_t* b, uint32_t n) {
    const uint32_t l = lane();
    bool ne = false;
    const uint32_t words = n >> 2;
    for (uint32_t w = l; w < words; w += 64) ne |= ld32u(a + 4 * w) != ld32u(b + 4 * w);
    const uint32_t i = words * 4 + l;
    if (i < n) ne |= a[i] != b[i];
    return __ballot(ne) == 0;
}

// Insert record `slot` (key k, n bytes, segment seg).  WAVE: every lane of
// the wave runs the same insert (same values, same addresses); the atomics
// are idempotent under that: a CAS that loses to the wave's own word reads
// that word back, and fetch_max of one value is one value.
template <bool WAVE>
DEV void key_insert(const CompactArgs& a, uint32_t slot, const uint8_t* k, uint32_t n, uint32_t seg) {
    const uint64_t h = WAVE ? hash_wave(k, n, seg) : hash_lane(k, n, seg);
    const uint32_t tag = (uint32_t)(h >> 32) & a.tag_mask;
    const uint64_t word = ((uint64_t)tag << 32) | (uint64_t)(slot + 1u);
    // a shortened tag (diagnostic build) also starts the probe, so that keys
    // sharing a tag do meet in the table
    uint64_t idx = (a.tag_mask == ~0u ? h : (uint64_t)tag) & a.table_mask;
    // the table has at least twice as many words as records: an empty word is always reached
    for (uint64_t probes = 0; probes <= a.table_mask; probes++, idx = (idx + 1) & a.table_mask) {
        uint64_t cur = AGENT_LOAD(&a.table[idx]);
        if (cur == 0) {
            uint64_t expect = 0;
            if (__hip_atomic_compare_exchange_strong(&a.table[idx], &expect, word, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                return;
            cur = expect;
        }
        if ((uint32_t)(cur >> 32) != tag) continue;
        const uint32_t other = (uint32_t)cur - 1u;
        if (other == slot) return;  // WAVE: another lane of this wave claimed the word
        // the word's record may be replaced while we look, but only by a record of the same key
        const rpgpu_record_index& ro = a.job.d_records[other];
        const rpgpu_batch_result& bo = a.job.d_batches[ro.batch];
        bool same = bo.segment == seg && key_len_of(ro) == n;
        if (same) {
            const uint8_t* ko = payload_of(a, bo) + ro.key_pos;
            same = WAVE ? equal_wave(k, ko, n) : equal_lane(k, ko, n);
        }
        if (same) {
            __hip_atomic_fetch_max(&a.table[idx], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (!WAVE || lane() == 0) atomicAdd(&a.counters[kCcKeyMismatches], 1u);
    }
}

// ---------------------------------------------------------------------------
// model::append_record_to_buffer over a parsed record, from its stored bytes.
// ---------------------------------------------------------------------------
// vint::deserialize (utils/vint.h:82-98): at most 10 bytes, stops at the end
// of the input with what it has
DEV int64_t rd_vint(const uint8_t* p, uint32_t avail, uint32_t& br) {
    uint64_t result = 0;
    uint32_t shift = 0;
    br = 0;
    for (uint32_t i = 0; shift <= 63 && i < avail; i++) {
        const uint64_t byte = p[i];
        br++;
        if (byte & 128) {
            result |= (byte & 127) << shift;
        } else {
            result |= byte << shift;
            break;
        }
        shift += 7;
    }
    return (int64_t)((result >> 1) ^ (~(result & 1) + 1));
}

struct Reenc {
    const uint8_t* pay;
    uint32_t plen;  // payload bytes
    uint32_t pos;   // read cursor
    uint32_t n;     // bytes produced
    bool canon;     // the produced bytes equal the stored ones so far
    uint8_t* out;
};

// one varint: read, narrowed the way model::record stores it (is32), written
// canonically (vint::to_bytes).  Returns the value as read.
template <bool W>
DEV int64_t re_vint(Reenc& e, bool is32, int64_t& stored) {
    uint32_t br;
    const int64_t v = rd_vint(e.pay + e.pos, e.plen - e.pos, br);
    stored = is32 ? (int64_t)(int32_t)v : v;
    const uint64_t zz = ((uint64_t)stored << 1) ^ (uint64_t)(stored >> 63);
    uint32_t cl = 1;
    for (uint64_t t = zz >> 7; t; t >>= 7) cl++;
    bool same = br == cl;
    for (uint32_t i = 0; i < cl; i++) {
        const uint8_t b = (uint8_t)(((zz >> (7 * i)) & 0x7F) | (i + 1 < cl ? 0x80 : 0));
        if (same && e.pay[e.pos + i] != b) same = false;
        if (W) e.out[e.n + i] = b;
    }
    e.canon &= same;
    e.n += cl;
    e.pos += br;
    return v;
}

// the bytes a length field owns: the parser takes them when the value read
// is positive (iobuf_copy: int-truncated, at most what is left), the writer
// writes what the parser took
template <bool W>
DEV void re_bytes(Reenc& e, int64_t v, int64_t stored) {
    if (v <= 0 || stored <= 0) return;
    uint32_t take = (uint32_t)stored;
    if (take > e.plen - e.pos) {
        take = e.plen - e.pos;
        e.canon = false;  // the stored record ends early; later fields are written though never stored
    }
    if (W)
        for (uint32_t i = 0; i < take; i++) e.out[e.n + i] = e.pay[e.pos + i];
    e.n += take;
    e.pos += take;
}

// Returns the re-encoded size; canon: it is the byte range [rec_pos, end_pos).
template <bool W>
DEV uint32_t reencode(const uint8_t* pay, uint32_t plen, const rpgpu_record_index& r, uint8_t* out, bool& canon) {
    Reenc e{pay, plen, r.rec_pos, 0, true, out};
    int64_t st, v;
    re_vint<W>(e, true, st);  // record::size_bytes, kept as parsed
    if (e.pos < plen) {       // attributes (always there in a parsed record)
        if (W) out[e.n] = pay[e.pos];
        e.n++;
        e.pos++;
    }
    re_vint<W>(e, false, st);  // timestamp_delta
    re_vint<W>(e, true, st);   // offset_delta
    v = re_vint<W>(e, true, st);
    re_bytes<W>(e, v, st);     // key
    v = re_vint<W>(e, true, st);
    re_bytes<W>(e, v, st);     // value
    const int64_t hcount = re_vint<W>(e, false, st);
    for (int64_t h = 0; h < hcount; h++) {
        if (e.pos >= plen) {
            // parse_record_headers goes on reading {0, 0} at the end of the
            // payload and keeps every such header: two zero varints each
            const uint32_t rest = (uint32_t)(hcount - h) * 2u;
            if (W)
                for (uint32_t i = 0; i < rest; i++) out[e.n + i] = 0;
            e.n += rest;
            e.canon = false;
            break;
        }
        v = re_vint<W>(e, true, st);
        re_bytes<W>(e, v, st);
        v = re_vint<W>(e, true, st);
        re_bytes<W>(e, v, st);
    }
    canon = e.canon && e.pos == r.end_pos && e.n == r.end_pos - r.rec_pos;
    return e.n;
}

// n bytes, 16 per lane per step (unaligned dwordx4 accesses are native), the
// last n % 16 one byte per lane
DEV void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    const uint32_t l = lane();
    const uint32_t body = n & ~15u;
    for (uint32_t o = l * 16; o < body; o += 1024) {
        const uint4 v = ld16u(src + o);
        __builtin_memcpy(dst + o, &v, 16);
    }
    if (l < n - body) dst[body + l] = src[body + l];
}

DEV uint64_t rl64c(uint64_t v, int l) {
    return (uint64_t)rl((uint32_t)v, l) | ((uint64_t)rl((uint32_t)(v >> 32), l) << 32);
}

DEV bool batch_clean(const CompactArgs& a, const rpgpu_batch_result& B, uint64_t nrt) {
    if ((B.flags & kElig) != kElig || (B.flags & RPGPU_F_DECODE_OVERFLOW)) return false;
    if ((B.flags & RPGPU_F_COMPRESSED) && (!(B.flags & RPGPU_F_CODEC_OK) || !a.job.d_decoded)) return false;
    if (B.record_count < 0 || B.records_parsed != (uint32_t)B.record_count) return false;
    return B.index_base <= nrt && (uint64_t)B.record_count <= nrt - B.index_base;
}

}  // namespace

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cinit(CompactArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.job.n_segments) return;
    const rpgpu_segment_summary& sm = a.job.d_summaries[s];
    const uint64_t nbt = n_batches_of(a);
    const bool ok = a.job.d_totals->overflow == 0 && sm.first_bad == sm.n_batches && sm.first_batch <= nbt &&
                    sm.n_batches <= nbt - sm.first_batch;
    a.seg_state[s] = ok ? 0u : 1u;
    a.seg_acc[3 * (uint64_t)s] = a.seg_acc[3 * (uint64_t)s + 1] = a.seg_acc[3 * (uint64_t)s + 2] = 0;
}

// grid-stride, one wave per batch
__global__ __launch_bounds__(256) void k_celig(CompactArgs a) {
    const uint32_t l = lane();
    const uint64_t nbt = n_batches_of(a), nrt = n_records_of(a);
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nbt; b += waves) {
        const rpgpu_batch_result& B = a.job.d_batches[b];
        const uint32_t s = B.segment;
        if (s >= a.job.n_segments) continue;
        if (!batch_clean(a, B, nrt)) {
            if (l == 0) atomicOr(&a.seg_state[s], 1u);
            continue;
        }
        const rpgpu_segment_summary& sm = a.job.d_summaries[s];
        if (sm.first_batch >= nbt || b < sm.first_batch) {
            if (l == 0) atomicOr(&a.seg_state[s], 1u);
            continue;
        }
        const rpgpu_batch_result& B0 = a.job.d_batches[sm.first_batch];
        const uint64_t base0 = (uint64_t)B0.base_offset, slot0 = B0.index_base;
        uint32_t bad = 0;
        for (uint32_t j = l; j < (uint32_t)B.record_count; j += 64) {
            const uint64_t slot = B.index_base + j;
            const rpgpu_record_index& r = a.job.d_records[slot];
            if (r.batch != (uint32_t)b || r.end_pos > B.decoded_len || r.rec_pos > r.end_pos || r.key_pos > r.end_pos) {
                bad |= 1;
                continue;
            }
            const uint64_t o = (uint64_t)B.base_offset + (uint64_t)(int64_t)r.offset_delta;
            if (o - base0 >= (1ull << 32)) bad |= 2;
            if (slot > slot0 && slot0 < nrt) {
                // the previous record in natural order: the previous index slot
                const rpgpu_record_index& p = a.job.d_records[slot - 1];
                if (p.batch < sm.first_batch || p.batch > b) {
                    bad |= 1;  // the segment's slots are not dense: one of its batches is not clean
                } else {
                    const uint64_t po = (uint64_t)a.job.d_batches[p.batch].base_offset + (uint64_t)(int64_t)p.offset_delta;
                    if (!((int64_t)o > (int64_t)po)) bad |= 2;
                }
            }
        }
        bad = wave_or(bad);
        if (bad && l == 0) atomicOr(&a.seg_state[s], bad);
    }
}

__global__ __launch_bounds__(256) void k_cinsert(CompactArgs a) {
    const uint32_t l = lane();
    const uint64_t nbt = n_batches_of(a);
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nbt; b += waves) {
        const rpgpu_batch_result& B = a.job.d_batches[b];
        const uint32_t s = B.segment;
        if (s >= a.job.n_segments || a.seg_state[s]) continue;
        const uint8_t* pay = payload_of(a, B);
        const uint32_t rc = (uint32_t)B.record_count;
        for (uint32_t j0 = 0; j0 < rc; j0 += 64) {
            const uint32_t j = j0 + l;
            const bool act = j < rc;
            const uint32_t slot = (uint32_t)(B.index_base + (act ? j : 0));
            uint32_t klen = 0, kpos = 0;
            if (act) {
                const rpgpu_record_index& r = a.job.d_records[slot];
                klen = key_len_of(r);
                kpos = r.key_pos;
            }
            const bool big = act && klen > kLaneKey;
            if (act && !big) key_insert<false>(a, slot, pay + kpos, klen, s);
            uint64_t m = __ballot(big);
            while (m) {
                const int f = __builtin_ctzll(m);
                m &= m - 1;
                key_insert<true>(a, rl(slot, f), pay + rl(kpos, f), rl(klen, f), s);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_ckeep(CompactArgs a) {
    const uint64_t nrt = n_records_of(a);
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= a.table_mask; i += step) {
        const uint64_t w = a.table[i];
        if (!w) continue;
        const uint64_t slot = (uint32_t)w - 1u;
        if (slot < nrt) atomicOr((unsigned long long*)&a.job.d_keep[slot >> 6], 1ull << (slot & 63));
    }
}

__global__ __launch_bounds__(256) void k_csize(CompactArgs a) {
    const uint32_t l = lane();
    const uint64_t nbt = n_batches_of(a);
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    // entries past the job's batches: nothing to write (the scans run over nb entries)
    for (uint64_t b = nbt + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.nb;
         b += (uint64_t)gridDim.x * blockDim.x) {
        a.bpos[b] = a.bcnt[b] = 0;
        a.bkept[b] = a.bplen[b] = 0;
    }
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nbt; b += waves) {
        const rpgpu_batch_result& B = a.job.d_batches[b];
        const uint32_t s = B.segment;
        uint32_t k = 0, plen = 0;
        const bool live = s < a.job.n_segments && a.seg_state[s] == 0;
        if (live) {
            const uint32_t rc = (uint32_t)B.record_count;
            for (uint32_t j0 = 0; j0 < rc; j0 += 64) {
                const uint64_t slot = B.index_base + j0 + l;
                const bool kept = j0 + l < rc && ((a.job.d_keep[slot >> 6] >> (slot & 63)) & 1);
                k += (uint32_t)__builtin_popcountll(__ballot(kept));
            }
            if (k == rc) {
                plen = B.decoded_len;
            } else if (k) {
                const uint8_t* pay = payload_of(a, B);
                uint32_t mine = 0;
                for (uint32_t j = l; j < rc; j += 64) {
                    const uint64_t slot = B.index_base + j;
                    if (!((a.job.d_keep[slot >> 6] >> (slot & 63)) & 1)) continue;
                    bool canon;
                    mine += reencode<false>(pay, B.decoded_len, a.job.d_records[slot], nullptr, canon);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
                plen = mine;
            }
            if (l == 0) {
                atomicAdd((unsigned long long*)&a.seg_acc[3 * (uint64_t)s], (unsigned long long)rc);
                atomicAdd((unsigned long long*)&a.seg_acc[3 * (uint64_t)s + 1], (unsigned long long)k);
                if (k && k != rc) atomicAdd((unsigned long long*)&a.seg_acc[3 * (uint64_t)s + 2], 1ull);
            }
        }
        if (l == 0) {
            a.bpos[b] = k ? (uint64_t)RPGPU_HEADER_SIZE + plen : 0;
            a.bcnt[b] = k ? 1 : 0;
            a.bkept[b] = k;
            a.bplen[b] = plen;
        }
    }
}

// after the scans: bpos[b] / bcnt[b] = output position / ordinal of batch b,
// [nb] the totals
__global__ __launch_bounds__(256) void k_cplan(CompactArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nbt = n_batches_of(a);
    rpgpu_compact_totals* T = a.job.d_ctotals;
    if (s == 0) {
        const uint64_t bytes = a.bpos[a.nb], nout = a.bcnt[a.nb];
        T->batches_out = nout;
        T->bytes_out = bytes;
        T->out_capacity_needed = bytes + 16;
        T->out_batch_capacity_needed = nout;
        const uint32_t ov = (bytes + 16 > a.job.out_capacity ? 1u : 0u) | (nout > a.job.out_batch_capacity ? 2u : 0u);
        T->overflow = ov;
        T->key_compare_mismatches = a.counters[kCcKeyMismatches];
        a.counters[kCcStampCount] = ov ? 0u : (uint32_t)nout;
        a.job.d_out_seg_offsets[a.job.n_segments] = bytes;
    }
    if (s >= a.job.n_segments) return;
    const rpgpu_segment_summary& sm = a.job.d_summaries[s];
    const uint32_t st = a.seg_state[s];
    const uint64_t fb = sm.first_batch < nbt ? sm.first_batch : nbt;
    const uint64_t lb = sm.n_batches < nbt - fb ? fb + sm.n_batches : nbt;
    a.job.d_out_seg_offsets[s] = a.bpos[fb];
    rpgpu_compact_segment g;
    g.status = (st & 1) ? RPGPU_COMPACT_NOT_CLEAN : (st & 2) ? RPGPU_COMPACT_OFFSETS : RPGPU_COMPACT_OK;
    g.reserved = 0;
    g.records_in = g.records_kept = g.batches_in = g.batches_out = g.batches_rewritten = g.bytes_out = 0;
    if (st == 0) {
        g.records_in = a.seg_acc[3 * (uint64_t)s];
        g.records_kept = a.seg_acc[3 * (uint64_t)s + 1];
        g.batches_rewritten = a.seg_acc[3 * (uint64_t)s + 2];
        g.batches_in = lb - fb;
        g.batches_out = a.bcnt[lb] - a.bcnt[fb];
        g.bytes_out = a.bpos[lb] - a.bpos[fb];
        atomicAdd((unsigned long long*)&T->records_in, (unsigned long long)g.records_in);
        atomicAdd((unsigned long long*)&T->records_kept, (unsigned long long)g.records_kept);
        atomicAdd((unsigned long long*)&T->batches_in, (unsigned long long)g.batches_in);
        atomicAdd((unsigned long long*)&T->batches_rewritten, (unsigned long long)g.batches_rewritten);
    }
    a.job.d_seg[s] = g;
}

// byte l (0..60) of the disk header (storage/segment_appender_utils.cc:28-54);
// header_crc, size_bytes and crc are stamped afterwards
DEV uint32_t header_byte(uint32_t l, const rpgpu_batch_result& B, uint32_t attrs, int64_t first_ts, int64_t max_ts,
                         uint32_t count) {
    uint64_t v = 0;
    uint32_t at = 0;
    if (l < 8) return 0;
    if (l < 16) { v = (uint64_t)B.base_offset; at = 8; }
    else if (l < 17) { v = (uint8_t)B.type; at = 16; }
    else if (l < 21) return 0;
    else if (l < 23) { v = attrs; at = 21; }
    else if (l < 27) { v = (uint32_t)B.last_offset_delta; at = 23; }
    else if (l < 35) { v = (uint64_t)first_ts; at = 27; }
    else if (l < 43) { v = (uint64_t)max_ts; at = 35; }
    else if (l < 51) { v = (uint64_t)B.producer_id; at = 43; }
    else if (l < 53) { v = (uint16_t)B.producer_epoch; at = 51; }
    else if (l < 57) { v = (uint32_t)B.base_sequence; at = 53; }
    else { v = count; at = 57; }
    return (uint32_t)(v >> (8 * (l - at))) & 0xFFu;
}

__global__ __launch_bounds__(256) void k_cwrite(CompactArgs a) {
    const uint32_t l = lane();
    if (a.job.d_ctotals->overflow) return;
    const uint64_t nbt = n_batches_of(a);
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nbt; b += waves) {
        const uint32_t k = a.bkept[b];
        if (!k) continue;
        const uint64_t oi = a.bcnt[b], op = a.bpos[b];
        const uint32_t plen = a.bplen[b];
        if (oi >= a.job.out_batch_capacity || op + RPGPU_HEADER_SIZE + plen + 16 > a.job.out_capacity) continue;
        const rpgpu_batch_result& B = a.job.d_batches[b];
        const uint8_t* pay = payload_of(a, B);
        uint8_t* dst = a.job.d_out + op + RPGPU_HEADER_SIZE;
        const uint32_t rc = (uint32_t)B.record_count;
        int64_t first_ts = B.first_timestamp, max_ts = B.max_timestamp;
        if (k == rc) {
            wave_copy(dst, pay, plen);
        } else {
            uint32_t carry = 0;
            bool have_first = false;
            int64_t ftd = 0, ltd = 0;
            for (uint32_t j0 = 0; j0 < rc; j0 += 64) {
                const uint64_t slot = B.index_base + j0 + l;
                const bool kept = j0 + l < rc && ((a.job.d_keep[slot >> 6] >> (slot & 63)) & 1);
                const uint64_t km = __ballot(kept);
                if (!km) continue;
                uint32_t sz = 0, rpos = 0, epos = 0;
                bool canon = false;
                int64_t td = 0;
                if (kept) {
                    const rpgpu_record_index& r = a.job.d_records[slot];
                    sz = reencode<false>(pay, B.decoded_len, r, nullptr, canon);
                    rpos = r.rec_pos;
                    epos = r.end_pos;
                    td = r.ts_delta;
                }
                if (!have_first) {
                    ftd = (int64_t)rl64c((uint64_t)td, __builtin_ctzll(km));
                    have_first = true;
                }
                ltd = (int64_t)rl64c((uint64_t)td, 63 - __builtin_clzll(km));
                // exclusive scan of the sizes
                uint32_t inc = sz;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(inc, d, 64);
                    if (l >= (uint32_t)d) inc += o;
                }
                const uint32_t off = carry + inc - sz;
                carry += rl(inc, 63);
                if (kept && !canon) {
                    bool c2;
                    reencode<true>(pay, B.decoded_len, a.job.d_records[slot], dst + off, c2);
                }
                // runs of adjacent canonical records: one copy each
                uint64_t cm = __ballot(kept && canon);
                while (cm) {
                    const int f = __builtin_ctzll(cm);
                    const uint64_t rest = ~(cm >> f);
                    const int e = rest ? __builtin_ctzll(rest) : 64 - f;  // lanes f .. f + e - 1
                    const uint32_t from = rl(rpos, f), to = rl(epos, f + e - 1);
                    wave_copy(dst + rl(off, f), pay + from, to - from);
                    cm &= (f + e >= 64) ? 0ull : (~0ull << (f + e));
                }
            }
            // copy_data_segment_reducer::filter (compaction_reducers.cc:207-217)
            first_ts = (int64_t)((uint64_t)B.first_timestamp + (uint64_t)ftd);
            if (!((uint16_t)B.attrs & 8u)) max_ts = (int64_t)((uint64_t)first_ts + (uint64_t)ltd);
        }
        const uint32_t attrs = (uint16_t)B.attrs & ~7u;
        if (l < RPGPU_HEADER_SIZE) a.job.d_out[op + l] = (uint8_t)header_byte(l, B, attrs, first_ts, max_ts, k);
        if (l == 0) {
            rpgpu_compact_batch e;
            e.out_pos = op;
            e.src_batch = (uint32_t)b;
            e.payload_len = plen;
            e.codec = (uint16_t)B.attrs & 7u;
            e.kept = k;
            e.flags = k == rc ? 0u : RPGPU_COMPACT_F_REWRITTEN;
            e.reserved = 0;
            a.job.d_out_batches[oi] = e;
            a.spos[oi] = op;
            a.splen[oi] = plen;
        }
    }
}

static uint32_t wave_grid(uint64_t items, uint32_t cus) {
    const uint64_t blocks = (items + 3) / 4, cap = (uint64_t)cus * 8;
    return (uint32_t)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

hipError_t launch_compact_insert(const CompactArgs& a, uint32_t cus, hipStream_t s) {
    hipLaunchKernelGGL(k_cinit, dim3((a.job.n_segments + 255) / 256 + 1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_celig, dim3(wave_grid(a.nb, cus)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cinsert, dim3(wave_grid(a.nb, cus)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_compact_keep(const CompactArgs& a, uint32_t cus, hipStream_t s) {
    const uint64_t blocks = (a.table_mask + 256) / 256, cap = (uint64_t)cus * 8;
    hipLaunchKernelGGL(k_ckeep, dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_compact_size(const CompactArgs& a, uint32_t cus, hipStream_t s) {
    hipLaunchKernelGGL(k_csize, dim3(wave_grid(a.nb, cus)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_compact_plan(const CompactArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_cplan, dim3((a.job.n_segments + 255) / 256 + 1), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_compact_write(const CompactArgs& a, uint32_t cus, hipStream_t s) {
    hipLaunchKernelGGL(k_cwrite, dim3(wave_grid(a.nb, cus)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rp
