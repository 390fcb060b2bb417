// rp_internal.h — shared between the device kernels (rp_kernels.hip) and the
// host runtime (rp_runtime.hip).  Not part of the public C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rpgpu.h"
#include "rp_deflate_core.h"  // rp::df: the work-area size, deflateBound, takes()

namespace rp {

constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kCrcPoly = 0x82F63B78u;

// Shift tables: advance a raw CRC state over 16 << m zero bytes (m = 0..5):
// the cross-lane merge tree of the validate kernel.
constexpr uint32_t kShiftLevels = 6;
// Braid stride of the validate kernel: lane l's 16 bytes of window row i sit
// at 1024 i + 16 l, so a braid word is followed by 1020 bytes of other braids.
constexpr uint32_t kBraidSkip = 1020;

// Validate kernel (rp_validate.hip): one wave per batch, 16 waves per
// workgroup (4 per SIMD), one workgroup per CU.  A payload is processed in
// 16 KiB windows of 16 rows of 1 KiB: lane l holds bytes [1024 i + 16 l, +16)
// of every row i (one coalesced dwordx4 load per row).
constexpr uint32_t kVWaves = 16;
constexpr uint32_t kWinBytes = 16384;
// LDS image of the validate kernel (bytes):
//  [0, 128 KiB)    braid tables T1023..T1020 (byte followed by 1023..1020
//                  zero bytes),
//                  32 copies so lane L always hits bank L % 32: two 64 KiB
//                  row-sets, entry e row = 256 B, table A at [0,128) and
//                  table B at [128,256), copy c at 4c
//  [128, 132 KiB)  slice tables T3..T0 (single copy): word/byte steps
//  [132, 156 KiB)  shift tables: 6 levels, shift by 16 << m bytes
constexpr uint32_t kLdsBraidOff = 0;
constexpr uint32_t kLdsSlice4Off = 131072;
constexpr uint32_t kLdsShiftOff = kLdsSlice4Off + 4096;
constexpr uint32_t kLdsValidateBytes = kLdsShiftOff + kShiftLevels * 4096;
static_assert(kLdsValidateBytes <= 160u * 1024u, "validate LDS image exceeds 160 KiB");

// Constant tables, built on the host once per context.
struct Tables {
    uint32_t slice[4][256];          // T_k[b]: byte b followed by k zero bytes (raw CRC)
    uint32_t hdr[57][256];           // T_d for d = 0..56 (parallel header CRC)
    uint32_t braid[4][256];          // T_{1023-t}[b]: byte b followed by 1023 - t zero bytes
    uint32_t shift[kShiftLevels][4][256]; // state byte j (value b << 8j) over 16 << m zero bytes
    uint32_t c57;                    // state 0xFFFFFFFF advanced over 57 zero bytes
    uint32_t c40;                    // state 0xFFFFFFFF advanced over 40 zero bytes
    uint32_t pad[2];
    // streaming CRC of decoded output (k_lz_exec): lane l's 16-byte state
    // moved to its 1 KiB row end, x^(8 * 16 (63 - l)); and the inverse
    // shifts x^(-8 z) (z = 0..1023) that take a zero-padded last row back to
    // the true end
    uint32_t lane_rowend[64];
    uint32_t inv_shift[1024];
};

// Discovery record per chunk (speculative walk), 32 bytes.
struct ChunkRec {
    uint64_t entry;   // first header position found in the chunk (kNone if none)
    uint64_t exit;    // first chain position >= chunk end, or terminal position
    uint32_t count;   // batches (with valid header) whose header starts in the chunk
    int32_t term;     // -1: ran through; else parser errc | (eof << 8)
    uint64_t tpos;    // terminal position when term >= 0
};

// Per-segment resolve output.
struct SegTerm {
    uint64_t pos;
    int32_t errc;
    int32_t eof;
};

// One piece of a planned compressed payload: an LZ4F block, a snappy-java
// chunk, or a whole raw snappy stream.  Independent pieces decode into their
// planned arena position; the blocks of a linked LZ4F frame are decoded in
// order by one wave, which rewrites `dst` with the position each landed at.
struct BlockItem {
    uint64_t src;    // absolute offset of the block data in the job's data
    uint64_t dst;    // absolute offset in the decoded arena (planned; actual for linked blocks)
    uint32_t csize;  // block data bytes
    uint32_t kind;   // kBlk* bits
    int32_t out;     // decoded bytes, -1 on failure (written by k_lz_exec)
    uint32_t cap;    // bytes reserved at dst (LZ4: the block maximum = the decoder's output bound)
    uint32_t crc;    // linear CRC32C (zero state, no final xor) of the decoded bytes, from k_lz_exec's
                     // flush; a linked frame's whole output on its first block
    uint32_t fast;   // kLzf*: walked by k_lzf_walk (executed from its records by k_lz_exec)
};
// BlockItem.fast: 0 k_lz_walk walks it; kLzfListed the planner gave it to
// k_lzf_walk (frecs reserved: PieceState.first_slab); kLzfReady walked into
// frecs by k_lzf_walk + k_lzf_tail (k_lz_exec executes those records);
// kLzfReject rejected there (out = -1 written)
// kLzfRaw: an independent raw block k_raw_copy copies (out / crc written there)
constexpr uint32_t kLzfNone = 0, kLzfReady = 1, kLzfReject = 2, kLzfListed = 3, kLzfRaw = 4;
// kBlkWhole: a raw (non-xerial) snappy payload, snappy_standard_compressor
// semantics (length 0 is an empty result whatever follows)
constexpr uint32_t kBlkRaw = 1, kBlkChecksum = 2, kBlkSnappy = 4, kBlkLinked = 8, kBlkWhole = 16;

// One parsed sequence of an LZ4 block / snappy tag: literal bytes
// [lip, lip + ll) of the piece's stream, then ml bytes copied from `off`
// back (ml = 0: literal only).  Written by the parse phase of k_lz_exec,
// executed by its wave phase.
struct SeqRec {
    uint32_t lip, ll, ml, off;
};
// k_lz_walk stores each piece's records in slabs of kSlabRecs taken from
// one pool (bump counter); slab_next chains a piece's slabs
constexpr uint32_t kSlabRecs = 512;
constexpr uint32_t kRecsPerLane = 256;                // k_lz_exec's own walk (pool exhausted): records per pass
// k_lz_exec waves (one LDS ring each) per CU: one workgroup of that many
// waves per CU, as compiled into rp_codec.hip (its ring size decides it)
uint32_t lz_exec_wgs_per_cu();

// A piece's walk result (k_lz_walk -> k_lz_exec)
struct PieceState {
    int32_t ip, op, need, st;   // the walk's PState (st: 1 done, -1 rejected, 0 suspended: pool exhausted)
    uint32_t ulen, safe;
    uint32_t nrec;              // records stored
    uint32_t first_slab;        // 0xFFFFFFFF: none
};

// FramePlan::mode
enum FrameMode : uint32_t {
    kFrameWhole = 0,   // decoded whole by k_decode_blocks (seq_list: what the planner did not split)
    kFrameLz4f = 1,    // LZ4F blocks
    kFrameSnappy = 2,  // snappy-java chunks, or a raw snappy stream as one piece
    kFrameNoRoom = 3,  // no arena room: DECODE_OVERFLOW
};
// FramePlan::xxh
enum FrameXxh : uint32_t {
    kXxhNotTaken = 0,  // k_content_xxh left the frame to k_decode_finish
    kXxhMatch = 1,
    kXxhMismatch = 2,  // k_content_apply takes the frame's verdict back
};
// Per decode item: how its payload is being decoded
struct FramePlan {
    uint32_t mode;   // FrameMode
    uint32_t first;  // first BlockItem
    uint32_t nb;     // number of BlockItems
    uint32_t ccs;    // LZ4F: content checksum present
    uint64_t content_size;  // LZ4F: content size (0 = absent)
    uint32_t ccs_val;       // LZ4F: stored content checksum
    uint32_t csf;           // LZ4F: content size present
    uint32_t xxh;           // k_content_xxh's verdict (FrameXxh)
    uint32_t pad;
};

// DeviceJob::inf_state: where the first pass left a gzip / zstd member
enum InfState : uint32_t {
    kInfDecoded = 0,    // decoded and checked, the bytes wait in scratch (inf_off): k_inflate_copy moves them
    kInfRejected = 1,   // the stream is rejected
    kInfAgain = 2,      // the output outgrew its scratch slot (or the pool ran out): k_members decodes it
                        // again, into the arena
    kZsFast = 3,        // zstd, parsed into records (zstd_fast_item; inf_off -> a ZsFastDesc): k_zexec executes them
    kZsPending = 4,     // zstd, turned down by k_zplan or k_zparse: k_zfallback runs the wave decoder on it
    kZsPlanned = 5,     // zstd, sized and planned by k_zplan for k_zparse
    kZsExact = 6,       // zstd, the decode reached into the overwritten part of the previous ring segment
                        // (zs::RingDirtyHook): k_zexact decodes it over the exact DCtx-buffer environment
    kZsExactAgain = 7,  // ... and again into its arena slot (k_zexact's pass 1) when it outgrew the scratch slot
};

// a kZsFast member's records (rp_inflate.hip zstd_fast_item), at inf_off in
// the scratch pool; k_zexec (rp_codec.hip) executes them into the arena slot
constexpr uint32_t kZsFastHdr = 128;  // descriptor bytes before the literal buffer
struct ZsFastDesc {
    uint64_t nlit, nrec, lit_off, rec_off;  // literal bytes, records; offsets from the descriptor
    uint64_t lcap, rcap;                    // literal buffer / record array capacities (k_zplan's header walk)
    uint64_t items, nitems;                 // the member's Huffman literal blocks (ZsLitItem), offset from the descriptor
    uint64_t sitems, nsitems;               // its sequence sections (ZsSeqItem)
    uint64_t pad[6];
};
static_assert(sizeof(ZsFastDesc) == kZsFastHdr, "descriptor size");
// One block's sequence section, planned by k_zplan (its three FSE tables
// snapshot, the stream) and decoded ahead by k_zlits into 16-byte raw
// sequences (rp_zstd_core.h RawSeq: lengths and the offset code), which the
// lane parser then only applies
struct ZsSeqItem {
    uint64_t src, n;   // member payload (offset in d_data), bytes
    uint64_t seqs;     // scratch offset of its raw sequences
    uint64_t tab;      // scratch offset of the ll / of / ml table snapshot
    uint64_t sp, sn;   // stream start (member offset), bytes
    uint32_t nseq, llog, olog, mlog;
    uint32_t status;   // 0 not decoded, 1 decoded and the stream ended exactly, 2 decoded, it did not
    uint32_t pad;
};
constexpr uint64_t kZsSeqTab = 10240;  // ll[512] + of[256] + ml[512] SeqSyms
// One block's Huffman literal section, planned by k_zplan (table snapshot,
// stream bounds, where its literals go) and decoded ahead by k_zlits, one
// wave per block, while k_zparse later only takes the bytes
struct ZsLitItem {
    uint64_t src;      // member payload (offset in d_data)
    uint64_t n;        // member bytes
    uint64_t lits;     // scratch offset of the block's literals
    uint64_t tab;      // scratch offset of the Huffman table snapshot (1 << hlog entries)
    uint64_t s0[4];    // stream starts (member offsets)
    uint32_t sn[4];    // stream bytes
    uint32_t cnt[4];   // symbols per stream
    uint32_t lsz, seg, ns, hlog, x2;
    uint32_t status;   // 0 not decoded, 1 decoded and every stream ended exactly, 2 decoded, a stream did not
};

// one chunk of a large gzip member decoded on its own wave (rp_inflate.hip,
// k_gzsplan / k_gzsfind / k_gzsdecode / k_gzsresolve)
struct GzsItem {
    uint32_t member;     // inf_list index (~0: unused)
    uint32_t k, nk;      // chunk ordinal, chunks of the member
    int32_t status;      // k_gzsdecode's verdict (0: not decoded)
    uint64_t begin, end; // deflate bytes searched for the chunk's first block header
    uint64_t start;      // bit offset of that block (~0: none found)
    uint64_t stop;       // bit offset the decode ended at
    uint64_t out;        // pool offset (symbols) of the decoded symbols
    uint64_t len;        // symbols decoded
    uint64_t guess;      // the member's output guess (sizes the region)
    uint32_t cap, pad;   // region symbols
};
constexpr uint64_t kGzsMin = 16384;    // stored gzip payloads this large take the split decode
constexpr uint64_t kGzsChunk = 16384;  // deflate bytes per chunk
constexpr uint32_t kGzsMaxK = 256;     // chunks per member at most

// job counters (DeviceJob::counters), zeroed per submit
constexpr size_t kCounterBytes = 256;
// The words of DeviceJob::counters, in slot order: ...Count a list's length
// (its writer appends), ...Cursor a claim cursor (fetch-add by the kernel
// that works the list off), ...64 the low word of a 64-bit pair (the next
// word is its high half: 25, 37, 43).  A new slot takes a free number, in
// its place below, and leaves the free list.
// Free: 51..63.
enum JobCounter : uint32_t {
    kCtrRewalks = 0,               // k_resolve: chunks walked again; k_finalize_totals -> totals.n_rewalks
    kCtrOverflowBits = 1,          // the record walks (k_validate, k_validate_decoded, k_walk): bit 1 = index
                                   // capacity; k_finalize_totals -> totals.overflow
    kCtrDecodeCount = 2,           // decode_list: k_emit; k_decode, k_crc_compose, k_decode_finish, k_content_xxh,
                                   // k_content_apply, k_dchain, k_validate_decoded
    kCtrSplitCount = 3,            // split_list: k_validate; k_crc_split, k_crc_combine, k_finalize_totals (DIAG)
    kCtrBlockCount = 4,            // blocks reserved (may pass block_capacity): k_decode's planners; k_lz_walk,
                                   // k_lz_exec
    kCtrSeqCursor = 5,             // k_decode_blocks over seq_list
    kCtrSeqCount = 6,              // seq_list: k_decode; k_decode_blocks
    kCtrLinkCount = 7,             // link_list: plan_lz4f; k_lz_exec
    kCtrExecCursor = 8,            // k_lz_exec over its units (linked frames, long pieces, chunks of 64 blocks)
    kCtrSlabCursor = 9,            // the record slab pool's bump cursor: k_lz_walk (walk_long, the lane walk)
    kCtrLaneCursor = 10,           // k_lz_walk's lane loop over lane_list
    kCtrLongCount = 11,            // long_list: k_decode's planners; k_lz_exec
    kCtrComposeCursor = 12,        // k_crc_compose over the decode list
    kCtrDecodedCursor = 13,        // k_validate_decoded over the decode, member and host lists
    kCtrFinishCursor = 14,         // k_decode_finish's phase 1 (frames without a content checksum) over the decode list
    kCtrSplitCursor = 15,          // k_crc_split over split_list
    kCtrInfCount = 16,             // inf_list: k_emit; every member kernel of rp_inflate.hip, k_zexec, k_dchain,
                                   // k_validate_decoded
    kCtrMembersFirstCursor = 17,   // k_members_first passes 0 / 1, phase 0 (members >= 128 KiB) over inf_list
    kCtrMembersCursor = 18,        // k_members over inf_list
    kCtrHostCount = 19,            // host_list: k_emit; host_codec_step (copied to the host), k_host_desc, k_dchain,
                                   // k_validate_decoded
    kCtrMembersFirstCursor2 = 20,  // k_members_first passes 0 / 1, phase 1 (the rest)
    kCtrZexecCursor = 21,          // k_zexec over inf_list
    kCtrZparseCursor = 22,         // k_zparse phase 0 (members >= 128 KiB) over inf_list
    kCtrZparseCursor2 = 23,        // k_zparse phase 1 (the rest)
    // Words 24..25 have two users.  kCtrInfScratchUsed64 is the bump allocator
    // of the gzip / zstd first-pass pool (DeviceJob::inf_scratch_used points
    // at it): every first-pass kernel of rp_inflate.hip adds to it.
    // kCtrRawBytes64 is the bytes k_raw_copy copied, k_crc_compose's gate
    // (it returns unless 2 x raw bytes >= data_len).  The allocator is not
    // disturbed: its kernels all run in the members stage, which wholly
    // precedes the decode stage on the job's stream, and nothing allocates
    // after that.  The gate is loosened: in a job with gzip / zstd members
    // and LZ4F raw blocks (benchmark stanza C6) the raw bytes start from what
    // the members reserved from the pool, so k_crc_compose may run where raw
    // blocks are a minority.  Results are the same (k_validate streams what
    // is not composed); the speed is unmeasured.
    kCtrInfScratchUsed64 = 24,
    kCtrRawBytes64 = 24,
    kCtrZfallbackCursor = 26,      // k_zfallback over inf_list
    kCtrZexactCount = 27,          // members marked kZsExact: zstd_first_item; k_zexact (0: nothing to do)
    kCtrZsItemCount = 28,          // zs_items (may pass zs_items_cap): k_zplan; k_zlits
    kCtrZlitsCursor = 29,          // k_zlits over zs_items
    kCtrZplanCursor = 30,          // k_zplan over inf_list
    kCtrZexactWork = 31,           // k_zexact's buffers, pool offset / 16 + 1 (0: none): its pass 0; its pass 1
    kCtrGzsItemCount = 32,         // gzs_items (may pass gzs_items_cap): k_gzsplan; k_gzsfind, k_gzsdecode
    kCtrGzsFindCursor = 33,        // k_gzsfind over gzs_items
    kCtrGzsDecodeCursor = 34,      // k_gzsdecode over gzs_items
    kCtrGzsResolveCursor = 35,     // k_gzsresolve over inf_list
    kCtrGzsPoolUsed64 = 36,        // gzs_pool symbols used (bump allocator): k_gzsdecode
    kCtrWlongCount = 38,           // wlong_list: k_decode's planners; k_lz_walk
    kCtrWlongCursor = 39,          // k_lz_walk's wave walk over wlong_list
    kCtrRawCount = 40,             // raw_list: plan_lz4f; k_raw_copy, k_crc_compose (0: nothing to compose)
    kCtrLaneCount = 41,            // lane_list (may pass block_capacity): k_decode's planners; k_lz_walk
    kCtrFrecsUsed64 = 42,          // frecs records reserved (bump allocator): plan_lz4f (note_fast)
    // one cursor, two kernels: k_decode_finish's phase 0 (the checksummed
    // frames first) and k_content_xxh, both over the decode list.  `defer`
    // makes k_decode_finish skip its phase 0 exactly when k_content_xxh runs.
    kCtrXxhCursor = 44,
    kCtrLzfCount = 45,             // lzf_list: plan_lz4f (note_fast); k_lzf_walk
    kCtrLzfCursor = 46,            // k_lzf_walk over lzf_list
    kCtrLzfTailCount = 47,         // lzf_tail: k_lzf_walk; k_lzf_tail
    kCtrMembersFirstP2Cursor = 48,   // k_members_first pass 2, phase 0
    kCtrMembersFirstP2Cursor2 = 49,  // k_members_first pass 2, phase 1
    kCtrComposeStored = 50,        // RPGPU_DIAG builds only: crcs k_crc_compose stored; k_finalize_totals ->
                                   // totals.reserved[0]
    kCtrCount = 51
};
static_assert(kCtrInfScratchUsed64 % 2 == 0 && kCtrRawBytes64 % 2 == 0 && kCtrGzsPoolUsed64 % 2 == 0 &&
                  kCtrFrecsUsed64 % 2 == 0,
              "a 64-bit pair starts at an even word");
static_assert(kCtrCount * sizeof(uint32_t) <= kCounterBytes, "the counter block holds every slot");

// Stored payloads with at most kLaneWalkMax records are walked one lane per
// batch by k_walk; k_validate walks the rest (and decoded payloads) with the
// wave-parallel walk.  (k_emit and the validate kernels must agree on it.)
constexpr int32_t kLaneWalkMax = 256;
__host__ __device__ __forceinline__ bool lane_walked(uint32_t flags, uint32_t codec, int32_t rc) {
    return (flags & RPGPU_F_COMPLETE) && codec == 0 && rc <= kLaneWalkMax;
}

// k_emit -> k_walk, 16 bytes per batch (contiguous across the lanes of a wave,
// where the batch results are 128 bytes apart): the absolute payload start,
// its length and the record count, or kNotLaneWalked where lane_walked() is
// false (incomplete, compressed, more than kLaneWalkMax records).
struct WalkDesc {
    uint64_t start;
    uint32_t n;
    int32_t rc;
};
static_assert(sizeof(WalkDesc) == 16, "one dwordx4 per lane");
constexpr int32_t kNotLaneWalked = 0x7FFFFFFF;
static_assert(kLaneWalkMax < kNotLaneWalked, "the mark is no record count k_walk takes");

// k_walk -> k_finalize_bitmap, 8 bytes per batch: the walk's verdict bits
// (RPGPU_F_PARSED ..), records_parsed (<= kLaneWalkMax) and parse_err; 0 =
// k_walk left the batch alone (its verdict is whoever else's).
constexpr uint64_t kVerdictWalked = 1ull << 63;
__host__ __device__ __forceinline__ uint64_t walk_verdict_pack(uint32_t flags, uint32_t parsed, uint32_t perr) {
    return kVerdictWalked | ((uint64_t)(perr & 0x7Fu) << 56) | ((uint64_t)(parsed & 0xFFFFFFu) << 32) | flags;
}
static_assert(kLaneWalkMax <= 0xFFFFFF, "records_parsed field of the verdict");

struct DeviceJob {
    const uint8_t* data;
    uint64_t data_len;            // bytes of d_data (= h_seg_offsets[n_segments])
    const uint64_t* seg_off;      // n_segments + 1
    const uint64_t* chunk_base;   // n_segments + 1 : first global chunk index of each segment
    uint32_t n_segments;
    uint32_t flags;
    uint32_t layout;              // rpgpu_layout
    uint32_t chunk_bytes;
    uint32_t total_chunks;
    ChunkRec* chunks;
    uint64_t* chunk_count;        // total_chunks (+1) : resolved counts -> exclusive scan in place
    uint64_t* chunk_entry;        // total_chunks : resolved entry position
    SegTerm* seg_term;
    rpgpu_batch_result* batches;
    uint64_t batch_capacity;
    uint64_t* slots;              // batch_capacity (+1): planned index slots -> scan
    uint64_t* dcap;               // batch_capacity (+1): planned decode bytes -> scan
    rpgpu_record_index* records;
    uint64_t record_capacity;
    uint8_t* decoded;
    uint64_t decoded_capacity;
    rpgpu_segment_summary* summaries;
    rpgpu_job_totals* totals;
    uint64_t* bitmap;
    const Tables* tables;
    uint32_t* counters;           // kCounterBytes: the words JobCounter names
    uint32_t* decode_list;        // batch_capacity: ordinals of batches to uncompress (kCtrDecodeCount)
    uint32_t* seq_list;           // batch_capacity: decode items decoded whole by one lane (kCtrSeqCount, kCtrSeqCursor)
    uint32_t* link_list;          // batch_capacity: decode items whose linked LZ4F blocks one wave decodes in order
                                  // (kCtrLinkCount)
    uint32_t* long_list;          // block_capacity: pieces k_lz_exec runs alone (kCtrLongCount)
    uint32_t* wlong_list;         // block_capacity: the long pieces k_lz_walk may walk one wave each (not
                                  // k_lzf_walk's; kCtrWlongCount, kCtrWlongCursor)
    uint32_t* split_list;         // split_capacity: stored payloads >= kSplitMin whose CRC runs in kSplitParts
                                  // chunks on separate waves (kCtrSplitCount)
    uint32_t* split_part;         // split_capacity * kSplitParts: the chunks' linear CRCs
    uint32_t split_capacity;
    uint64_t split_min;           // payloads this large are split: max(kSplitMin, 2 x the job's bytes per k_validate wave)
    SeqRec* seqs;                 // k_lz_exec's own walks: kRecsPerLane per resident wave
    uint32_t exec_waves;          // k_lz_exec waves (lz_exec_wgs_per_cu() per workgroup; sizes `seqs`)
    PieceState* pstate;           // block_capacity: walk results
    SeqRec* pool;                 // record slabs
    uint32_t crc_compose;         // k_crc_compose assembles LZ4F stored crcs from k_raw_copy's block CRCs
    uint32_t* dchain;             // k_dchain's record-chain ends of decoded payloads, at their index slots (the
                                  // record pool, free again once decode is done); nullptr = k_validate_decoded chains
    uint32_t* slab_next;          // pool_slabs: next slab of the same piece
    uint32_t pool_slabs;
    uint2* frecs;                 // LZ4 sequence records of k_lzf_walk (executed by k_lz_exec), 8 B each
    uint64_t frec_cap;            // records frecs holds
    uint32_t* lzf_list;           // block_capacity: blocks k_lzf_walk takes (planner-listed; kCtrLzfCount, kCtrLzfCursor)
    uint32_t* lane_list;          // block_capacity: the blocks k_lz_walk's lane loop considers (kCtrLaneCount,
                                  // kCtrLaneCursor)
    uint32_t* raw_list;           // block_capacity: independent raw blocks k_raw_copy copies (kCtrRawCount)
    uint32_t* lzf_tail;           // block_capacity: blocks whose tails k_lzf_tail runs (kCtrLzfTailCount)
    BlockItem* blocks;            // block work list (kCtrBlockCount items reserved; k_lz_exec takes them in
                                  // chunks of 64 off kCtrExecCursor)
    uint32_t block_capacity;
    FramePlan* plans;             // one per decode item
    uint32_t* seg_first_bad;      // n_segments: first chain ordinal failing complete && crc_ok (atomicMin)
    const uint64_t* seeds;        // optional chain seeds (index-seeded discovery), per segment ascending
    const uint64_t* seed_off;     // n_segments + 1
    uint32_t* inf_list;           // batch_capacity: ordinals of gzip / zstd batches (k_members_first / k_members;
                                  // kCtrInfCount)
    uint32_t* inf_state;          // batch_capacity: each member's InfState
    uint64_t* inf_off;            // batch_capacity: scratch offset of each member's first-pass output
    uint64_t* inf_total;          // batch_capacity: decoded bytes of each member
    uint8_t* inf_scratch;         // first-pass output pool (context scratch)
    uint64_t inf_scratch_bytes;
    uint64_t* inf_scratch_used;   // bump allocator of the pool (zeroed per job)
    uint32_t zs_fast;             // zstd members may take the parse / execute split (kZsFast)
    uint32_t zs_split;            // k_zparse (side stream) owns the zstd members' first pass
    uint64_t* zs_items;           // zs_items_cap: scratch offsets of the planned literal blocks (k_zplan -> k_zlits)
    uint32_t zs_items_cap;
    uint32_t* host_list;          // batch_capacity: ordinals of host-decoded (zstd) batches (RPGPU_JOB_HOST_CODECS)
    uint32_t* gzs_mem;            // 2 x batch_capacity, per member: first item, chunks | 1 << 31 once resolved
                                  // (null: no split decode, k_members_first takes every gzip member)
    GzsItem* gzs_items;           // gzs_items_cap
    uint32_t gzs_items_cap;
    uint16_t* gzs_pool;           // decoded symbols of the chunks (bytes, or 256 + a window position)
    uint64_t gzs_pool_syms;
    WalkDesc* walk_desc;          // batch_capacity: k_emit -> k_walk, what a lane needs to walk its batch
    uint64_t* walk_verdict;       // batch_capacity: k_walk -> k_finalize_bitmap (walk_verdict_pack; PARSE jobs)
};

// one host-decoded batch (RPGPU_JOB_HOST_CODECS): its payload, the host's
// verdict and where its bytes sit in the staging buffers
struct HostItem {
    uint64_t src;        // payload offset in d_data
    uint64_t stage;      // offset in the payload / decoded staging
    uint64_t out_len;    // decoded bytes
    uint64_t cap;        // arena reservation (0 when rejected)
    uint32_t n;          // payload bytes
    uint32_t ord;        // batch ordinal
    int32_t record_count;
    int32_t status;      // 0 decoded, -1 the reference throws
};
hipError_t launch_host_desc(const DeviceJob& j, HostItem* items, uint32_t n, hipStream_t s);
hipError_t launch_host_gather(const DeviceJob& j, const HostItem* items, uint32_t n, uint8_t* stage, hipStream_t s);
hipError_t launch_host_patch(const DeviceJob& j, const HostItem* items, uint32_t n, hipStream_t s);
hipError_t launch_host_scatter(const DeviceJob& j, const HostItem* items, uint32_t n, const uint8_t* stage,
                               hipStream_t s);

// kernel launchers (rp_kernels.hip)
hipError_t launch_chunk_base(const DeviceJob& j, hipStream_t s);
hipError_t launch_discover(const DeviceJob& j, hipStream_t s);
hipError_t launch_resolve(const DeviceJob& j, hipStream_t s);
hipError_t launch_emit(const DeviceJob& j, hipStream_t s);
hipError_t launch_validate(const DeviceJob& j, hipStream_t s, uint32_t grid, bool compose = true);  // rp_validate.hip
hipError_t launch_crc_compose(const DeviceJob& j, hipStream_t s, uint32_t grid);
bool dchain_wanted(const DeviceJob& j);                                         // rp_validate.hip
hipError_t launch_dchain(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_validate_decoded(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_walk(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_decode(const DeviceJob& j, hipStream_t s, uint32_t grid);    // rp_codec.hip
hipError_t launch_decode_blocks(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_lz_walk(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_lz_exec(const DeviceJob& j, hipStream_t s);
hipError_t launch_raw_copy(const DeviceJob& j, hipStream_t s, uint32_t cus);
hipError_t launch_lzf_walk(const DeviceJob& j, hipStream_t s, uint32_t cus);
hipError_t launch_decode_finish(const DeviceJob& j, hipStream_t s, uint32_t grid, bool defer = false);
hipError_t launch_content_xxh(const DeviceJob& j, hipStream_t s, uint32_t grid);  // k_decode_finish(defer)'s checksums
hipError_t launch_content_apply(const DeviceJob& j, hipStream_t s, uint32_t grid);  // their mismatches, after the join
// gzip members (rp_inflate.hip): first pass (into scratch) before the slot
// scans, then the copy into the arena and the second pass where needed
hipError_t launch_inflate_plan(const DeviceJob& j, hipStream_t s, uint32_t grid, int pass = 0);
hipError_t launch_inflate(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_zparse(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_zplan(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_gzsplan(const DeviceJob& j, hipStream_t s);
hipError_t launch_gzsplit(const DeviceJob& j, hipStream_t s, uint32_t grid, int part);  // part 1: find, 2: decode + resolve
hipError_t launch_zfallback(const DeviceJob& j, hipStream_t s, uint32_t grid);
hipError_t launch_zexact(const DeviceJob& j, hipStream_t s, int pass);  // rp_inflate.hip
hipError_t launch_zstamps(hipStream_t s, int print);  // RPGPU_ZSTAMPS builds: reset / print the decoder stamps
hipError_t launch_zexec(const DeviceJob& j, hipStream_t s);  // rp_codec.hip
// one payload, one wave (rpgpu_uncompress); res[0] = rc (0 / -1 / -2), res[1] = out_len
hipError_t launch_uncompress_one(int codec, const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap,
                                 int64_t* res, hipStream_t s);
// rpgpu_uncompress_batch: one payload per lane
struct UncItem {
    uint64_t src, n;    // input bytes [src, src + n) of the staged inputs
    uint64_t dst, cap;  // output slot [dst, dst + cap) (cap includes 16 bytes of wild-copy room)
    int32_t codec, pad;
};
// compressor::compress (rp_compress.hip): 64 KiB blocks into scratch slots
// of kCompSlot bytes (>= snappy::MaxCompressedLength(65536)), then one frame
// per payload
constexpr uint32_t kCompSlot = 76800;
// large stored payloads (disk layout): CRC in kSplitParts chunks, one wave
// each, merged by GF(2) shifts (k_crc_split / k_crc_combine).  Only payloads
// above twice a wave's share of the job are split (DeviceJob::split_min): a
// job of many batches is balanced by k_validate's stride already, and
// splitting C2 / C5's batches at 256 KiB measured slower (validate 8.8 ->
// 9.9 ms), a separate pass where the stride overlapped them.
constexpr uint64_t kSplitMin = 256u << 10;
constexpr uint32_t kSplitParts = 16;
struct CompBlock {
    uint64_t src;                    // input offset of the block (any alignment; 8 readable bytes past the block)
    uint32_t n, codec;               // block bytes (<= 65536), RPGPU_CODEC_LZ4 / _SNAPPY
    uint32_t frag_len, frag_blocks;  // snappy: on a fragment's first block, the fragment's bytes and blocks
};
struct CompPayload {
    uint64_t n, out;                 // input bytes; output offset
    uint32_t first, nblocks, codec, pad;
};
hipError_t launch_compress(const uint8_t* in, const CompBlock* blocks, uint32_t nb, const CompPayload* pay, uint32_t np,
                           uint8_t* scratch, uint32_t* sizes, uint8_t* out, uint64_t* out_len, hipStream_t s);
// the block kernels alone, over a block array that may hold fewer than nb
// blocks (the rest zeroed: codec 0, their waves leave); block b compresses into
// scratch + slot_off[b] (slot_off null: b * kCompSlot)
hipError_t launch_compress_blocks(const uint8_t* in, const CompBlock* blocks, uint32_t nb, uint8_t* scratch,
                                  const uint64_t* slot_off, uint32_t* sizes, bool lz4, bool snappy, hipStream_t s);
// gzip_compressor::compress on the device (rp_deflate.hip): one stream per
// wave (lane 0 runs rp_deflate_core.h), at most kDeflateStreams resident, each
// over a work area of df::kWorkBytes; payloads are taken from the list
// through a cursor.  Output slots hold df::bound(n); df::takes(n) says which
// payloads the device accepts.  The work buffer is kDeflateCursor bytes (the
// cursor, a fixed slot) followed by the streams' areas.
constexpr uint32_t kDeflateStreams = 1024;
constexpr uint64_t kDeflateCursor = 256;
inline uint64_t deflate_work_bytes(uint32_t streams) { return kDeflateCursor + (uint64_t)streams * df::kWorkBytes; }
struct DeflateItem {
    uint64_t src, n;     // input bytes [src, src + n)
    uint64_t frag, out;  // fragment size (0: one fragment); output slot offset
};
hipError_t launch_deflate(const uint8_t* in, const DeflateItem* items, uint32_t count, uint8_t* out, uint64_t* out_len,
                          uint8_t* work, uint32_t streams, hipStream_t s);
// the gzip blocks of a recompress block array (codec RPGPU_CODEC_GZIP, one
// block per batch, one fragment): block b into scratch + slot_off[b], its
// length into sizes[b]
struct CompBlock;
hipError_t launch_deflate_blocks(const uint8_t* in, const CompBlock* blocks, uint32_t nb, uint8_t* scratch,
                                 const uint64_t* slot_off, uint32_t* sizes, uint8_t* work, uint32_t streams, hipStream_t s);
hipError_t launch_uncompress_many(const UncItem* items, uint32_t count, const uint8_t* in, uint64_t in_total,
                                  uint8_t* out, int64_t* res, hipStream_t s);
hipError_t launch_finalize(const DeviceJob& j, hipStream_t s);
// rpgpu_serialize_wire (rp_validate.hip): batches [first, first + n) of a job's
// results; src/dst: n + 1 u64 each (dst ends as the exclusive scan, dst[n] = total)
hipError_t launch_to_wire(const uint8_t* disk, uint8_t* wire, const rpgpu_batch_result* batches, const uint64_t* seg_off,
                          uint64_t first, uint32_t n, uint64_t* src, uint64_t* dst, void* scan_tmp, size_t scan_bytes,
                          uint32_t grid, hipStream_t s);
// rpgpu_stamp (rp_validate.hip): base offset of batch i = next + offs[i]
// (RPGPU_STAMP_OFFSETS: offs = exclusive scan of the steps), cursor zeroed
hipError_t launch_stamp_steps(const uint8_t* data, const uint64_t* pos, uint32_t n, uint64_t* steps, hipStream_t s);
// d_n (optional, device): the batch count is min(*d_n, n)
hipError_t launch_stamp(uint8_t* data, const uint64_t* pos, const uint32_t* plen, const uint64_t* offs, int64_t next,
                        uint32_t n, uint32_t flags, const Tables* T, uint32_t* cursor, uint32_t grid, hipStream_t s,
                        const uint32_t* d_n = nullptr);
hipError_t scan_exclusive_u64(uint64_t* data, uint64_t n, void* temp, size_t temp_bytes, hipStream_t s);
// n = min(*d_n, n_cap), read on the device
hipError_t scan_exclusive_u64_devn(uint64_t* data, const uint64_t* d_n, uint64_t n_cap, void* temp, hipStream_t s);
size_t scan_temp_bytes(uint64_t n);

// rp_index.hip: segment index rebuild (rpgpu_segment_index), one wave per segment
hipError_t launch_segment_index(const rpgpu_batch_result* batches, uint64_t cap, const rpgpu_segment_summary* sums,
                                uint32_t n_segments, uint64_t step, rpgpu_index_state* states, uint32_t* rel_offset,
                                uint32_t* rel_time, uint64_t* position, hipStream_t s);
size_t segment_index_ws_bytes(uint32_t n_segments, uint64_t cap);
hipError_t launch_segment_index_pieces(const rpgpu_batch_result* batches, uint64_t cap,
                                       const rpgpu_segment_summary* sums, uint32_t n_segments, uint64_t step,
                                       rpgpu_index_state* states, uint32_t* rel_offset, uint32_t* rel_time,
                                       uint64_t* position, void* ws, hipStream_t s);


// rp_compact.hip: key compaction (rpgpu_compact).  Workspace arrays are
// context scratch; nb / nr bound the source job's batch / record totals.
struct CompactArgs {
    rpgpu_compact_job job;
    uint64_t nb, nr;          // job.batch_capacity / job.record_capacity
    uint64_t* table;          // key table: tag << 32 | (record slot + 1), 0 = empty
    uint64_t table_mask;      // words - 1 (a power of two)
    uint32_t tag_mask;        // ~0u (RPGPU_CKEY_TAG_BITS in the diagnostic build: fewer tag bits)
    uint32_t* seg_state;      // n_segments: bit 0 not clean, bit 1 offsets
    uint64_t* seg_acc;        // n_segments * 3: records in, records kept, batches rewritten
    uint64_t* bpos;           // nb + 1: output bytes per source batch -> exclusive scan
    uint64_t* bcnt;           // nb + 1: 1 per source batch with kept records -> exclusive scan
    uint32_t* bkept;          // nb: kept records per source batch
    uint32_t* bplen;          // nb: output payload bytes per source batch
    uint64_t* spos;           // nb: rpgpu_stamp positions of the output batches
    uint32_t* splen;          // nb: their payload lengths
    uint32_t* counters;       // the words CompactCounter names
};
enum CompactCounter : uint32_t {
    kCcKeyMismatches = 0,  // key compare mismatches: k_cinsert; k_cplan -> the totals
    kCcStampCount = 1,     // batches to stamp: k_cplan; k_stamp (its d_n)
    kCcStampCursor = 2,    // k_stamp's claim cursor
    kCcCount = 3
};
hipError_t launch_compact_insert(const CompactArgs& a, uint32_t cus, hipStream_t s);  // eligibility + key insert
hipError_t launch_compact_keep(const CompactArgs& a, uint32_t cus, hipStream_t s);
hipError_t launch_compact_size(const CompactArgs& a, uint32_t cus, hipStream_t s);
hipError_t launch_compact_plan(const CompactArgs& a, hipStream_t s);  // after the scans: segments, totals, overflow
hipError_t launch_compact_write(const CompactArgs& a, uint32_t cus, hipStream_t s);

// rp_append.hip: produce-path append (rpgpu_append_wire).  Workspace arrays
// are context scratch; nb bounds the source job's batch total.
// Payloads are copied in pieces of kAppendPiece bytes, one wave each (a
// starting guess, not a measured value).
constexpr uint32_t kAppendPiece = 65536;
struct AppendArgs {
    rpgpu_append_job job;
    uint64_t nb;              // job.batch_capacity
    uint32_t* seg_bad;        // n_segments: first failing chain ordinal of each set (atomicMin; ~0u = none)
    uint32_t* verdict;        // nb: rpgpu_append_status of each source batch
    uint64_t* bpos;           // nb + 1: output bytes per source batch (0: not appended) -> exclusive scan
    uint64_t* bcnt;           // nb + 1: low half 1 per appended batch, high half its copy pieces -> exclusive scan
    uint64_t* bstep;          // nb + 1: offset step (last_offset_delta + 1) per appended batch -> exclusive scan
    uint64_t* spos;           // nb: rpgpu_stamp positions of the append-time batches
    uint32_t* splen;          // nb: their payload lengths
    uint32_t* counters;       // the words AppendCounter names
    const Tables* tables;
};
enum AppendCounter : uint32_t {
    kAcStampCount = 0,   // append-time batches to stamp: k_append_copy lists them; k_stamp (its d_n)
    kAcStampCursor = 1,  // k_stamp's claim cursor
    kAcCount = 2
};
hipError_t launch_append_sizes(const AppendArgs& a, hipStream_t s);   // verdicts, then sizes / counts / steps
hipError_t launch_append_plan(const AppendArgs& a, hipStream_t s);    // after the scans: sets, summaries, totals
hipError_t launch_append_copy(const AppendArgs& a, uint32_t cus, hipStream_t s);
hipError_t launch_append_meta(const AppendArgs& a, hipStream_t s);    // after the stamp: d_out_batches

// rp_fetch.hip: fetch-path log read (rpgpu_fetch).  Workspace arrays are
// context scratch; nb bounds the source job's batch total.  Payloads are
// copied in pieces of kAppendPiece bytes, one wave each, as the append does.
// What k_fetch_select leaves per partition for k_fetch_plan.
struct FetchSel {
    uint32_t status, over_budget;
    int64_t base_offset, last_offset, next_offset, first_timestamp;
};
struct FetchArgs {
    rpgpu_fetch_job job;
    uint64_t nb;              // job.batch_capacity
    uint64_t* bpos;           // nb + 1: output bytes per source batch (0: not returned) -> exclusive scan
    uint64_t* bcnt;           // nb + 1: low half 1 per returned batch, high half its copy pieces -> exclusive scan
    uint64_t* brec;           // nb + 1: record_count (as uint32) per returned batch -> exclusive scan
    uint32_t* bpart;          // nb: the partition of each returned batch
    FetchSel* sel;            // n_partitions
};
hipError_t launch_fetch_select(const FetchArgs& a, hipStream_t s);  // bpos / bcnt / brec zeroed before
hipError_t launch_fetch_plan(const FetchArgs& a, hipStream_t s);    // after the scans: parts, offsets, totals
hipError_t launch_fetch_copy(const FetchArgs& a, uint32_t cus, hipStream_t s);  // payloads, headers, d_out_batches

// rp_recompress.hip: recompression of compacted batches (rpgpu_recompress).
// Workspace arrays are context scratch; nb bounds the input batch count, the
// block array and the block scratch are sized from the input capacities
// (recompress_block_cap / recompress_scratch_cap).
// RecompressArgs::mode[b]: the effective codec in the low byte, then
constexpr uint32_t kRcCompress = 1u << 8;  // compressed here (its blocks are planned)
struct RecompressArgs {
    rpgpu_recompress_job job;
    uint64_t nb;              // job.in_batch_capacity
    uint32_t* mode;           // nb: effective codec | kRcCompress | RPGPU_RECOMPRESS_F_* << 16
    uint64_t* bblk;           // nb + 1: 64 KiB blocks per input batch -> exclusive scan (the batch's first block)
    uint64_t* bscr;           // nb + 1: block scratch bytes per input batch -> exclusive scan
    uint64_t* bpos;           // nb + 1: output bytes per input batch -> exclusive scan
    uint64_t* bcnt;           // nb + 1: low half 1 per batch, high half its pack pieces -> exclusive scan
    uint32_t* clen;           // nb: output payload bytes per batch
    CompBlock* blocks;        // block_cap, zeroed per call
    uint64_t block_cap;
    uint64_t* slot_off;       // block_cap: where each block compresses to in `scratch`
    uint32_t* sizes;          // block_cap: the block kernels' output sizes
    uint8_t* scratch;
    uint64_t scratch_cap;
    uint64_t* spos;           // nb: rpgpu_stamp positions of the compressed batches
    uint32_t* splen;          // nb: their payload lengths
    uint32_t* counters;       // the words RecompressCounter names
    uint32_t device_gzip;     // rpgpu_set_device_gzip: gzip batches are compressed here (one block each)
};
enum RecompressCounter : uint32_t {
    kRcStampCount = 0,   // compressed batches to stamp: k_recompress_pack lists them; k_stamp (its d_n)
    kRcStampCursor = 1,  // k_stamp's claim cursor
    kRcBadInput = 2,     // an input entry lies outside in_capacity, or the plan outgrew the block array / scratch
    kRcCount = 3
};
// what the block array and the block scratch must hold for any input within the capacities
uint64_t recompress_block_cap(uint64_t in_capacity, uint64_t in_batch_capacity, uint64_t snappy_frag);
uint64_t recompress_scratch_cap(uint64_t in_capacity, uint64_t block_cap);
hipError_t launch_recompress_plan(const RecompressArgs& a, void* scan_tmp, size_t scan_bytes, hipStream_t s);
hipError_t launch_recompress_layout(const RecompressArgs& a, void* scan_tmp, size_t scan_bytes, hipStream_t s);
hipError_t launch_recompress_pack(const RecompressArgs& a, uint32_t cus, hipStream_t s);
hipError_t launch_recompress_meta(const RecompressArgs& a, hipStream_t s);  // after the stamp

}  // namespace rp
