/*
 * rpgpu.h — C-ABI boundary of the MI355X record-batch validation/decode engine.
 *
 * This is the drop-in boundary for Redpanda's batch hot path.
 * Every entry point below replaces one reference interface; the reference
 * file:line it stands in for is cited next to it (paths relative to
 * /root/reference/src/v).  Plain pointers and sizes only — no HIP, torch or
 * C++ types cross this boundary, and no exception ever does: every call
 * returns an int status (0 = ok, <0 = rpgpu_status).
 *
 * Layouts of the per-batch result, the per-record index and the segment
 * summary are part of the contract: the CPU oracle (oracle/) emits the same
 * structs, so parity is a memcmp.
 */
#ifndef RPGPU_H_
#define RPGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Constants                                                                 */
/* ------------------------------------------------------------------------ */

/* model::packed_record_batch_header_size (model/record.h:473-487): the
 * comment there says 57 but the fields sum to 61. */
#define RPGPU_HEADER_SIZE 61u
/* kafka::internal::kafka_header_size (kafka/protocol/kafka_batch_adapter.h:25-37) */
#define RPGPU_KAFKA_HEADER_SIZE 61u
/* bytes of the Kafka CRC prefix rebuilt big-endian from the header
 * (model/record_utils.cc:68-80: attrs..record_count) */
#define RPGPU_CRC_PREFIX_SIZE 40u

/* model::compression (model/compression.h:35-48) */
enum rpgpu_codec {
    RPGPU_CODEC_NONE = 0,
    RPGPU_CODEC_GZIP = 1,
    RPGPU_CODEC_SNAPPY = 2, /* snappy-java framing, falls back to raw snappy */
    RPGPU_CODEC_LZ4 = 3,    /* LZ4 frame */
    RPGPU_CODEC_ZSTD = 4,
};

/* storage::parser_errc (storage/parser_errc.h:18-25), same numbering. */
enum rpgpu_parser_errc {
    RPGPU_ERRC_NONE = 0,
    RPGPU_ERRC_END_OF_STREAM = 1,
    RPGPU_ERRC_HEADER_ONLY_CRC_MISSMATCH = 2,
    RPGPU_ERRC_INPUT_STREAM_NOT_ENOUGH_BYTES = 3,
    RPGPU_ERRC_FALLOCATED_FILE_READ_ZERO_BYTES_FOR_HEADER = 4,
    RPGPU_ERRC_NOT_ENOUGH_BYTES_IN_PARSER_FOR_ONE_RECORD = 5,
};

/* Library status codes (return values). */
enum rpgpu_status {
    RPGPU_OK = 0,
    RPGPU_E_INVALID = -1,      /* bad argument */
    RPGPU_E_NO_DEVICE = -2,    /* no HIP device / HIP call failed */
    RPGPU_E_NOMEM = -3,        /* device or host allocation failed */
    RPGPU_E_OVERFLOW = -4,     /* caller-provided output capacity too small */
    RPGPU_E_CODEC = -5,        /* uncompress failed (maps to std::runtime_error) */
    RPGPU_E_UNSUPPORTED = -6,  /* codec not decoded by this engine (gzip/zstd) */
    RPGPU_E_HIP = -7,          /* kernel launch / runtime error */
};
/* rpgpu_poll: the job is still running (a positive, non-error status). */
#define RPGPU_PENDING 1

/* ------------------------------------------------------------------------ */
/* Per-batch verdict flags (rpgpu_batch_result.flags).  Each bit is pinned    */
/* to one reference function ("composite verdict").         */
/* ------------------------------------------------------------------------ */
#define RPGPU_F_HEADER_OK (1u << 0)      /* read_header_impl accepted: header_crc != 0 and == internal_header_only_crc (storage/parser.cc:139-176) */
#define RPGPU_F_COMPLETE (1u << 1)       /* size_bytes-61 payload bytes present (storage/parser.cc:206-216) */
#define RPGPU_F_CRC_OK (1u << 2)         /* (uint32)hdr.crc == crc32c(BE hdr40 ++ stored payload) (storage/log_replayer.cc:62-79, model/record_utils.cc:68-91) */
#define RPGPU_F_COMPRESSED (1u << 3)     /* attrs codec != none */
#define RPGPU_F_CODEC_INVALID (1u << 4)  /* codec value 5..7: record_batch_attributes::compression() throws (model/record.h:283-300) */
#define RPGPU_F_CODEC_UNSUPPORTED (1u << 5) /* zstd in a job without RPGPU_JOB_DECODE (kept from the host-only zstd path) */
#define RPGPU_F_CODEC_OK (1u << 6)       /* compressor::uncompress succeeded (compression/compression.cc:34-55) */
#define RPGPU_F_PARSED (1u << 7)         /* a record walk was run over the (decoded) payload */
#define RPGPU_F_PARSE_ASYNC_OK (1u << 8) /* model::for_each_record completed without throwing (model/record.h:680-697) */
#define RPGPU_F_PARSE_OK (1u << 9)       /* record_batch::for_each_record: no throw AND no trailing bytes (model/record.h:616-627) */
#define RPGPU_F_INDEX_WRITTEN (1u << 10) /* record index entries [index_base, index_base+records_parsed) are valid */
#define RPGPU_F_WIRE_V2 (1u << 11)       /* wire layout: magic == 2 (kafka/protocol/kafka_batch_adapter.cc:39-43) */
#define RPGPU_F_DECODE_OVERFLOW (1u << 12) /* decoded bytes did not fit the reserved arena slot */

/* rpgpu_batch_result.parse_err: why the record walk stopped (0 = no error). */
enum rpgpu_parse_err {
    RPGPU_PARSE_ERR_NONE = 0,
    RPGPU_PARSE_ERR_ATTR_EOF = 1,        /* consume_type<int8_t> out_of_range (bytes/details/io_iterator_consumer.h:64-84) */
    RPGPU_PARSE_ERR_COPY_NEGATIVE = 2,   /* iobuf_copy with (int)len < 0 -> bad_alloc (bytes/iobuf.cc:133-157) */
    RPGPU_PARSE_ERR_HEADER_RESERVE = 3,  /* headers.reserve(count) throws (model/record_utils.cc:99) */
    RPGPU_PARSE_ERR_TRAILING = 4,        /* sync for_each_record: bytes left after record_count records */
    RPGPU_PARSE_ERR_INDEX_CAPACITY = 5,  /* more records than the reserved index slots (record_count > payload) */
};

/* Reference-environment limit for headers.reserve(header_count): libstdc++
 * throws length_error above max_size() and Seastar throws bad_alloc when the
 * shard cannot allocate count*sizeof(record_header) (=64 B).  The latter is
 * environment dependent; this engine pins it at 2 GiB of reservation. */
#define RPGPU_MAX_HEADER_RESERVE (1ll << 25)

/* ------------------------------------------------------------------------ */
/* Output layouts                                                            */
/* ------------------------------------------------------------------------ */

/* One entry per batch reached by the continuous_batch_parser chain whose
 * header passed read_header_impl (storage/parser.cc:139-176), in chain order.
 * 128 bytes. */
typedef struct rpgpu_batch_result {
    uint64_t file_pos;            /* physical offset of the header in its segment */
    int64_t base_offset;          /* record_batch_header fields as decoded by   */
    int64_t first_timestamp;      /* storage::header_from_iobuf                 */
    int64_t max_timestamp;        /* (storage/parser.cc:36-76)                  */
    int64_t producer_id;
    int32_t size_bytes;           /* stored size (header + payload) */
    int32_t record_count;
    int32_t last_offset_delta;
    int32_t base_sequence;
    uint32_t header_crc;          /* stored header_crc */
    uint32_t crc;                 /* stored crc (as uint32) */
    uint32_t crc_computed;        /* crc32c(BE hdr40 ++ stored payload) */
    uint32_t header_crc_computed; /* internal_header_only_crc(header) */
    uint32_t flags;               /* RPGPU_F_* */
    uint32_t segment;             /* segment index within the job */
    uint64_t index_base;          /* first record-index slot of this batch */
    uint64_t decoded_off;         /* offset of the decoded payload in the decoded arena (compressed batches) */
    uint32_t records_parsed;      /* records fully parsed before stop */
    uint32_t decoded_len;         /* decoded payload bytes (== stored payload len when not compressed) */
    uint32_t decoded_crc;         /* reset_size_checksum_metadata: new crc over decoded payload (storage/parser_utils.cc:114-120) */
    uint32_t decoded_header_crc;  /* reset_size_checksum_metadata: new header_crc */
    int16_t attrs;
    int16_t producer_epoch;
    int8_t type;
    uint8_t parse_err;            /* rpgpu_parse_err */
    uint16_t reserved0;
    uint64_t reserved1;
} rpgpu_batch_result;

/* One entry per parsed record (model/record_utils.cc:94-181).  Positions are
 * byte offsets inside the batch's (decoded) payload.  64 bytes. */
typedef struct rpgpu_record_index {
    uint32_t batch;               /* job-wide batch ordinal */
    uint32_t rec_pos;             /* offset of the record's length varint */
    int64_t ts_delta;             /* timestamp_delta */
    int32_t length;               /* record::size_bytes (length varint, int32) */
    int32_t offset_delta;         /* static_cast<int32_t>(offset delta varint) */
    int32_t key_len;              /* key_length as stored by model::record (int32) */
    uint32_t key_pos;             /* first key byte */
    int32_t val_len;
    uint32_t val_pos;
    int32_t hdr_count;            /* number of record headers */
    uint32_t hdr_pos;             /* first byte after the header-count varint */
    uint32_t end_pos;             /* first byte after this record */
    int8_t attrs;                 /* record attributes byte */
    uint8_t pad[3];
    uint32_t reserved[2];
} rpgpu_record_index;

/* Per segment: where and why the parser chain stopped, and the
 * log_replayer checkpoint (storage/log_replayer.cc:62-79, log_replayer.h:159-165). */
typedef struct rpgpu_segment_summary {
    uint64_t first_batch;         /* job-wide ordinal of the segment's first batch */
    uint64_t n_batches;           /* batches with a valid header on the chain */
    uint64_t terminal_pos;        /* file position where the chain stopped */
    uint64_t bytes_consumed;      /* continuous_batch_parser::_bytes_consumed */
    int32_t terminal_errc;        /* rpgpu_parser_errc that ended the chain */
    int32_t terminal_eof;         /* 1 if the stop came from a short read (input_stream::eof()) */
    int32_t has_checkpoint;       /* checkpoint fields valid */
    uint32_t first_bad;           /* chain ordinal of the first batch failing crc (== n_batches if none) */
    int64_t ckpt_last_offset;     /* checkpoint.last_offset */
    uint64_t ckpt_truncate_pos;   /* checkpoint.truncate_file_pos */
    uint64_t n_records;           /* index slots reserved for this segment */
    uint64_t reserved[2];
} rpgpu_segment_summary;

/* Whole-job totals, written by the device. */
typedef struct rpgpu_job_totals {
    uint64_t n_batches;
    uint64_t n_records;           /* index slots used */
    uint64_t decoded_bytes;       /* arena bytes reserved */
    uint64_t batch_capacity_needed;
    uint64_t record_capacity_needed;
    uint64_t decoded_capacity_needed;
    uint32_t overflow;            /* nonzero: an output capacity was too small */
    uint32_t n_rewalks;           /* discovery chunks whose speculative entry had to be re-walked */
    uint64_t reserved[2];
} rpgpu_job_totals;

/* ------------------------------------------------------------------------ */
/* Context / memory                                                          */
/* ------------------------------------------------------------------------ */

typedef struct rpgpu_ctx rpgpu_ctx;

/* Number of visible HIP devices (0 when none). */
int rpgpu_device_count(void);
/* One context per host thread or Seastar shard (ownership
 * row): it owns a HIP stream pair and device scratch.  Not thread-safe. */
int rpgpu_create(int device, rpgpu_ctx** out);
int rpgpu_destroy(rpgpu_ctx* ctx);
const char* rpgpu_strerror(int status);
const char* rpgpu_last_error(rpgpu_ctx* ctx);

int rpgpu_dev_alloc(rpgpu_ctx* ctx, size_t bytes, void** out);
int rpgpu_dev_free(rpgpu_ctx* ctx, void* p);
/* pinned host memory for the double-buffered H2D staging */
int rpgpu_host_alloc(rpgpu_ctx* ctx, size_t bytes, void** out);
int rpgpu_host_free(rpgpu_ctx* ctx, void* p);
int rpgpu_memcpy_h2d(rpgpu_ctx* ctx, void* dst, const void* src, size_t n, void* stream);
int rpgpu_memcpy_d2h(rpgpu_ctx* ctx, void* dst, const void* src, size_t n, void* stream);
int rpgpu_memset(rpgpu_ctx* ctx, void* dst, int value, size_t n, void* stream);
int rpgpu_sync(rpgpu_ctx* ctx, void* stream);

/* ------------------------------------------------------------------------ */
/* crc::crc32c (hashing/crc32c.h:19-40)                                      */
/* ------------------------------------------------------------------------ */

/* google crc32c::Extend(crc, p, n) semantics: Extend(0, p, n) is the standard
 * CRC32C (Castagnoli, reflected 0x82F63B78, init/xorout ~0).  Host-side
 * (SSE4.2) for the small per-call sizes crc::crc32c sees; bulk segment CRC
 * runs on the GPU through rpgpu_submit. Pure, thread-safe, no allocation. */
uint32_t rpgpu_crc32c_extend(uint32_t crc, const uint8_t* p, size_t n);

/* ------------------------------------------------------------------------ */
/* Segment engine (new; replaces the per-batch loops of                      */
/* storage::continuous_batch_parser::consume (storage/parser.cc:218-254),    */
/* log_replayer::recover_in_thread (storage/log_replayer.cc:95-114),         */
/* storage::internal::decompress_batch (storage/parser_utils.cc:43-60) and   */
/* kafka_batch_adapter::adapt (kafka/protocol/kafka_batch_adapter.cc:126)).  */
/* ------------------------------------------------------------------------ */

enum rpgpu_layout {
    RPGPU_LAYOUT_DISK = 0, /* Redpanda on-disk: 61-byte LE header (storage/segment_appender_utils.cc:28-54) */
    RPGPU_LAYOUT_WIRE = 1, /* Kafka v2 wire: BE header (kafka/protocol/kafka_batch_adapter.cc:32-91) */
};

#define RPGPU_JOB_CRC (1u << 0)     /* compute the payload crc (always on in recovery) */
#define RPGPU_JOB_PARSE (1u << 1)   /* walk records into the index */
#define RPGPU_JOB_DECODE (1u << 2)  /* uncompress lz4/snappy/gzip/zstd payloads into the arena (on the device) */
/* With RPGPU_JOB_DECODE: decode zstd batches on the host instead (SURVEY.md
 * §8(b)'s CPU fallback: stream_zstd::do_uncompress over libzstd,
 * compression/stream_zstd.cc:152-178), into the same arena, then CRC and walk
 * them on the device like every other decoded payload.  Same plan and
 * verdicts as the device decoder; the submit then synchronizes on its stream
 * once the chain is planned (the payloads' sizes and bytes cross to the host
 * and back), so rpgpu_submit_async returns after that point. */
#define RPGPU_JOB_HOST_CODECS (1u << 3)

/* All pointers are DEVICE pointers, caller-owned.  Segments are concatenated
 * in d_data; segment s spans [d_seg_offsets[s], d_seg_offsets[s+1]). */
typedef struct rpgpu_job {
    const uint8_t* d_data;
    const uint64_t* d_seg_offsets;   /* n_segments + 1 entries */
    const uint64_t* h_seg_offsets;   /* HOST copy of the same offsets (sizes the launch grids) */
    uint32_t n_segments;
    uint32_t layout;                 /* rpgpu_layout */
    uint32_t flags;                  /* RPGPU_JOB_* */
    uint32_t chunk_bytes;            /* discovery chunk size (0 = default 256 KiB) */
    rpgpu_batch_result* d_batches;   /* capacity batch_capacity */
    uint64_t batch_capacity;
    rpgpu_record_index* d_records;   /* capacity record_capacity (may be NULL if !PARSE) */
    uint64_t record_capacity;
    uint8_t* d_decoded;              /* decoded arena (may be NULL if !DECODE); bytes are defined only at
                                        [decoded_off, +decoded_len) of batches with RPGPU_F_CODEC_OK (the
                                        reference throws and keeps nothing for the others); 16-B aligned */
    uint64_t decoded_capacity;
    rpgpu_segment_summary* d_summaries; /* n_segments entries */
    rpgpu_job_totals* d_totals;      /* one entry */
    uint64_t* d_valid_bitmap;        /* optional: 1 bit per batch, set = crc_ok && header_ok (&& parse_ok if PARSE) */
    /* Optional chain seeds (the index-seeded mode of SURVEY.md §8(b)): known
     * batch header positions of each segment, ascending, e.g. the
     * position_index of its .base_index (storage/index_state.h:23-100,
     * index_state::hydrate_from_buffer, storage/index_state.cc:104-186).
     * Segment s's seeds are d_seeds[d_seed_offsets[s] .. d_seed_offsets[s+1]).
     * Discovery then enters each chunk by following the chain from the last
     * seed before it instead of scanning its bytes.  Seeds are verified like
     * any discovered header (a wrong or stale index only costs re-walks);
     * results are identical with or without them.  NULL = scan. */
    const uint64_t* d_seeds;
    const uint64_t* d_seed_offsets;  /* device, n_segments + 1 entries */
} rpgpu_job;

/* Enqueue the whole pipeline (discover -> resolve -> plan -> validate/decode)
 * on `stream` (hipStream_t, NULL = the context's stream).  Asynchronous:
 * results are valid after rpgpu_sync / an event on that stream.  Capacity
 * overflow is reported in d_totals (overflow != 0), never by writing out of
 * bounds. */
int rpgpu_submit(rpgpu_ctx* ctx, const rpgpu_job* job, void* stream);

/* Asynchronous completion for a reactor that must not block (SURVEY.md
 * §8(b) segment-engine row; storage::continuous_batch_parser::consume
 * returns a future, storage/parser.h:94-136): the same pipeline as
 * rpgpu_submit, plus a completion event on the launch stream.
 * rpgpu_poll is non-blocking: RPGPU_OK once every output is written,
 * RPGPU_PENDING while the job runs, < 0 on a device error.  rpgpu_wait
 * blocks until then.  rpgpu_release frees the handle (after completion or
 * not: the job itself is not cancelled). */
typedef struct rpgpu_pending rpgpu_pending;
int rpgpu_submit_async(rpgpu_ctx* ctx, const rpgpu_job* job, void* stream, rpgpu_pending** out);
int rpgpu_poll(rpgpu_pending* p);
int rpgpu_wait(rpgpu_pending* p);
int rpgpu_release(rpgpu_pending* p);

/* Output sizes a job needs, before it runs (the segment-engine row's "sized
 * by a query call").  Reads only d_data, d_seg_offsets, h_seg_offsets,
 * n_segments, layout, flags and chunk_bytes of `job`; the chain is
 * discovered and planned into context scratch.  Synchronous on `stream`. */
typedef struct rpgpu_capacity {
    uint64_t n_batches;          /* batch_capacity needed */
    uint64_t record_capacity;    /* record index slots needed (RPGPU_JOB_PARSE) */
    uint64_t decoded_capacity;   /* decoded arena bytes needed (RPGPU_JOB_DECODE; 0 otherwise) */
    uint64_t reserved;
} rpgpu_capacity;
int rpgpu_query_capacity(rpgpu_ctx* ctx, const rpgpu_job* job, void* stream, rpgpu_capacity* out);

/* Device time of the pipeline stages, measured with HIP events recorded on
 * the launch stream, averaged over every timed rpgpu_submit since the
 * previous call (milliseconds; the call resets the average).  Indices:
 * 0 = whole pipeline, 1 = discover, 2 = resolve+emit+plan, 3 = validate,
 * 4 = decode (0 when the job has no RPGPU_JOB_DECODE), 5 = lane record walk
 * of stored payloads (k_walk; 0 without RPGPU_JOB_PARSE). */
int rpgpu_last_timings(rpgpu_ctx* ctx, float* ms, int n);
/* Enable/disable per-kernel event timing (off by default). */
int rpgpu_set_timing(rpgpu_ctx* ctx, int enable);

/* ------------------------------------------------------------------------ */
/* storage::segment_index rebuild during recovery                            */
/* (checksumming_consumer::consume_batch_end -> segment_index::maybe_track,  */
/* storage/log_replayer.cc:62-74, storage/segment_index.cc:58-72 ->          */
/* index_state::maybe_index, storage/index_state.cc:48-95).                  */
/* ------------------------------------------------------------------------ */

/* segment_index::default_data_buffer_step (storage/segment_index.h:49) */
#define RPGPU_INDEX_DEFAULT_STEP 32768u

/* Per segment: the index_state header fields (storage/index_state.h:37-65)
 * after replaying maybe_track over the segment's crc-good batch prefix
 * [0, summary.first_bad).  64 bytes. */
typedef struct rpgpu_index_state {
    int64_t base_offset;          /* IN: the segment's base offset (index_state.base_offset, kept by reset()) */
    int64_t max_offset;           /* last tracked batch's last_offset */
    int64_t base_timestamp;       /* first tracked batch's first_timestamp */
    int64_t max_timestamp;        /* max over tracked batches of max(first_timestamp, max_timestamp) */
    uint64_t first_entry;         /* entries of this segment live at [first_entry, first_entry + n_entries)
                                     of the entry arrays (== summary.first_batch) */
    uint64_t n_entries;           /* relative_offset_index.size() */
    int64_t assert_batch;         /* -1, or the segment ordinal of the first tracked batch whose
                                     base_offset < base_offset: the reference vasserts (aborts) there,
                                     so tracking stops before it */
    uint64_t tracked;             /* batches replayed through maybe_track */
} rpgpu_index_state;

/* Device pointers.  d_batches/d_summaries are the outputs of a completed
 * disk-layout rpgpu_submit (same stream, or synchronised).  d_states has
 * n_segments entries with base_offset filled in by the caller.  The three
 * entry arrays (relative_offset_index, relative_time_index, position_index)
 * need batch_capacity slots each.  step = segment_index::_step. */
int rpgpu_segment_index(rpgpu_ctx* ctx, const rpgpu_batch_result* d_batches, uint64_t batch_capacity,
                        const rpgpu_segment_summary* d_summaries, uint32_t n_segments, uint64_t step,
                        rpgpu_index_state* d_states, uint32_t* d_rel_offset, uint32_t* d_rel_time,
                        uint64_t* d_position, void* stream);

/* ------------------------------------------------------------------------ */
/* Write side: header stamping of batches about to be written (SURVEY.md     */
/* §8(f) row 3)                                                              */
/* ------------------------------------------------------------------------ */
/* disk_log_appender::operator() (storage/disk_log_appender.cc:72-74): the
 * batch gets the appender's next offset as base_offset, the appender moves
 * on to last_offset + 1 (:113-119). */
#define RPGPU_STAMP_OFFSETS (1u << 0)
/* storage::internal::reset_size_checksum_metadata (storage/parser_utils.cc:
 * 114-120): size_bytes = 61 + payload bytes, crc = crc_record_batch. */
#define RPGPU_STAMP_CRC (1u << 1)

/* n disk-layout batches in the device buffer d_data (16-byte aligned, with 16
 * readable bytes past the last payload): batch i's 61-byte header at
 * d_pos[i], its payload (d_payload_len[i] bytes) right after it.  In place,
 * in batch order: RPGPU_STAMP_OFFSETS numbers them from next_offset,
 * RPGPU_STAMP_CRC resets size and crc, and header_crc
 * (model::internal_header_only_crc) is always recomputed last.  Batches must
 * not overlap.  Asynchronous on `stream`. */
int rpgpu_stamp(rpgpu_ctx* ctx, uint8_t* d_data, const uint64_t* d_pos, const uint32_t* d_payload_len, uint32_t n,
                int64_t next_offset, uint32_t flags, void* stream);

/* kafka::writer_serialize_batch (kafka/protocol/response_writer.h:241-276)
 * for batches [first, first + n) of a completed disk-layout job (its
 * d_batches, over the job's d_data / d_seg_offsets): each batch's Kafka v2
 * wire header (big endian; batch_length = size_bytes - 12, partition leader
 * epoch 0, magic 2, the stored crc) followed by its payload, back to back in
 * d_wire (capacity: the batches' size_bytes summed).  *d_total (a device
 * u64) receives the record set's length.  Asynchronous on `stream`. */
int rpgpu_serialize_wire(rpgpu_ctx* ctx, const uint8_t* d_data, const uint64_t* d_seg_offsets,
                         const rpgpu_batch_result* d_batches, uint64_t first, uint32_t n, uint8_t* d_wire,
                         uint64_t* d_total, void* stream);

/* ------------------------------------------------------------------------ */
/* compression::compressor::uncompress (compression/compression.h:21-24)     */
/* ------------------------------------------------------------------------ */

/* Decode one payload (host pointers).  LZ4 and snappy run on the device;
 * gzip and zstd run on the host, the reference's own loops over zlib /
 * libzstd (gzip_compressor.cc:161-230, stream_zstd.cc:152-178: the CPU
 * fallback of SURVEY.md §8(b)).  *out_len receives the decoded size;
 * returns RPGPU_E_CODEC where the reference throws std::runtime_error,
 * RPGPU_E_OVERFLOW if cap is too small (out_len then holds the size needed),
 * RPGPU_E_UNSUPPORTED when zlib / libzstd cannot be loaded.  ctx may be
 * NULL for gzip / zstd (no device work). */
int rpgpu_uncompress(rpgpu_ctx* ctx, int codec, const void* in, size_t n,
                     void* out, size_t cap, size_t* out_len);

/* n payloads in one device round trip (the per-batch call sites
 * storage/parser_utils.cc:51 and kafka/protocol/kafka_batch_adapter.cc:259,
 * batched).  Arrays of n entries; status[i] is what rpgpu_uncompress would
 * return for payload i.  Returns RPGPU_OK when every payload has a status. */
int rpgpu_uncompress_batch(rpgpu_ctx* ctx, uint32_t n, const int* codecs, const void* const* in,
                           const size_t* in_len, void* const* out, const size_t* cap, size_t* out_len,
                           int* status);

/* ------------------------------------------------------------------------ */
/* compression::compressor::compress (compression/compression.cc:17-33): the */
/* write side's storage::internal::compress_batch (storage/parser_utils.cc:   */
/* 97-111).  SURVEY.md §8(f) row 3.                                          */
/* ------------------------------------------------------------------------ */

/* Bytes compressor::compress can produce for n input bytes: the LZ4 frame
 * (lz4_frame_compressor.cc:72-113) or the snappy-java stream over frag-byte
 * iobuf fragments (snappy_java_compressor.cc:58-75; frag 0 = one fragment),
 * or a safe bound for the host gzip / zstd streams.  0 for RPGPU_CODEC_NONE. */
size_t rpgpu_compress_bound(int codec, size_t n, size_t frag);

/* n payloads compressed on the device in one round trip (host pointers), the
 * bytes liblz4 1.9.3 / libsnappy 1.1.8 produce through the reference's
 * wrappers, bit for bit: RPGPU_CODEC_LZ4 -> LZ4 frame {independent 64 KiB
 * blocks, content size, level 1}; RPGPU_CODEC_SNAPPY -> snappy-java with one
 * chunk per frag[i]-byte fragment (frag may be NULL: one fragment, a
 * contiguous iobuf).  status[i]: RPGPU_OK; RPGPU_E_OVERFLOW when cap[i] <
 * the output (out_len[i] then holds its size); RPGPU_E_CODEC for
 * RPGPU_CODEC_NONE (the reference throws "nothing to compress").  gzip and
 * zstd run on the host, the reference's loops over zlib / libzstd
 * (gzip_compressor.cc:126-161, stream_zstd.cc:84-104; RPGPU_E_UNSUPPORTED
 * when the library cannot be loaded).  With rpgpu_set_device_gzip on (and a
 * non-NULL ctx), gzip payloads are staged and compressed on the device in the
 * same round trip, over frag[i]-byte fragments: the same bytes, statuses and
 * sizes as the host path gives with zlib 1.2.11. */
int rpgpu_compress_batch(rpgpu_ctx* ctx, uint32_t n, const int* codecs, const void* const* in, const size_t* in_len,
                         const size_t* frag, void* const* out, const size_t* cap, size_t* out_len, int* status);

/* gzip compression on the device (off by default; off, every call behaves as
 * without it): gzip_compressor::compress (gzip_compressor.cc:126-161) --
 * deflateInit2(Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15 + 16, 8,
 * Z_DEFAULT_STRATEGY), one deflate(Z_NO_FLUSH) per fragment, Z_FINISH -- with
 * the bytes of zlib 1.2.11, one lane per payload (k_deflate).  It applies to
 * rpgpu_compress_batch and to rpgpu_recompress (see there).  A payload whose deflateBound, n + (n >> 12) +
 * (n >> 14) + (n >> 25) + 25, plus 61 does not fit int32 stays on the host. */
int rpgpu_set_device_gzip(rpgpu_ctx* ctx, int enable);
/* Device milliseconds of k_deflate in the last rpgpu_compress_batch that ran
 * gzip payloads on the device under rpgpu_set_timing (HIP events on the
 * call's stream); RPGPU_E_INVALID when there was none. */
int rpgpu_gzip_device_ms(rpgpu_ctx* ctx, float* ms);
/* *n = gzip payloads compressed on the device by this context so far */
int rpgpu_gzip_device_payloads(rpgpu_ctx* ctx, uint64_t* n);

/* ------------------------------------------------------------------------ */
/* Host segment path (log_replayer over files, storage/log_replayer.cc:       */
/* 95-114): pinned, double-buffered H2D of host-resident segments.  Segments */
/* are copied in staging groups on a copy stream while the previous group    */
/* validates, and each group's outputs come back while the next one runs.    */
/* Outputs are HOST pointers and hold exactly what ONE rpgpu_submit over all */
/* the segments returns: job-wide batch ordinals (record_index.batch),       */
/* index_base, decoded_off and summary.first_batch.                          */
/* ------------------------------------------------------------------------ */
typedef struct rpgpu_host_job {
    const uint8_t* const* segments;  /* host pointers (pinned or pageable) */
    const uint64_t* seg_sizes;
    uint32_t n_segments;
    uint32_t layout;
    uint32_t flags;
    uint32_t group_kib;              /* staging group size in KiB (0 = 256 MiB): segments are copied and
                                        validated in groups of at most this many bytes (a larger segment
                                        is a group of its own) */
    rpgpu_batch_result* batches;     /* host, capacity batch_capacity */
    uint64_t batch_capacity;
    rpgpu_segment_summary* summaries; /* host, n_segments */
    rpgpu_job_totals* totals;        /* host */
    /* optional (NULL / 0: not returned): the per-record index
     * (RPGPU_JOB_PARSE) and the decoded arena (RPGPU_JOB_DECODE); a capacity
     * that is too small sets totals.overflow bit 2 / 4, as on the device */
    rpgpu_record_index* records;
    uint64_t record_capacity;
    uint8_t* decoded;
    uint64_t decoded_capacity;
    /* optional segment index rebuild (rpgpu_segment_index over each group's
     * results, disk layout): index_step != 0 fills index_states[n_segments]
     * (base_offset is an IN field) and the three entry arrays (batch_capacity
     * entries each; segment s's entries at [first_entry, first_entry +
     * n_entries), first_entry == its summary.first_batch) */
    uint64_t index_step;
    rpgpu_index_state* index_states;
    uint32_t* rel_offset;
    uint32_t* rel_time;
    uint64_t* position;
} rpgpu_host_job;

int rpgpu_validate_host(rpgpu_ctx* ctx, const rpgpu_host_job* job);

/* Decoded-size plan of one lz4 / snappy payload from its frame structure
 * alone (the arena rule rpgpu_submit reserves per batch): an upper bound of
 * what compressor::uncompress returns for a payload it accepts; 0 for an
 * empty, unplannable or gzip / zstd payload (the caller then grows on
 * RPGPU_E_OVERFLOW).  Host only, no context. */
uint64_t rpgpu_uncompress_bound(int codec, const void* in, size_t n);

/* rpgpu_stamp over a HOST buffer, in place (storage::stamp_batches): staged
 * through the context's pinned and device scratch (grow-only), one H2D, the
 * kernels, one D2H.  Synchronous.  d_pos / d_payload_len as rpgpu_stamp,
 * but host arrays. */
int rpgpu_stamp_host(rpgpu_ctx* ctx, uint8_t* buf, size_t len, const uint64_t* pos, const uint32_t* payload_len,
                     uint32_t n, int64_t next_offset, uint32_t flags);

/* ------------------------------------------------------------------------ */
/* Key compaction of segments (storage::internal::self_compact_segment's     */
/* three reducers: compaction_key_reducer, compacted_offset_list_reducer and */
/* copy_data_segment_reducer, storage/compaction_reducers.cc:34-222,         */
/* storage/segment_utils.cc:197-201, :306-365).                              */
/* ------------------------------------------------------------------------ */
/* rpgpu_compact_segment.status */
enum rpgpu_compact_status {
    RPGPU_COMPACT_OK = 0,
    /* summary.first_bad != n_batches, or a batch lacks one of HEADER_OK,
     * COMPLETE, CRC_OK, PARSED, PARSE_OK, INDEX_WRITTEN (CODEC_OK when
     * compressed) or has DECODE_OVERFLOW, or the source job overflowed: the
     * reference throws or asserts on such a batch */
    RPGPU_COMPACT_NOT_CLEAN = 1,
    /* record offsets base_offset + offset_delta are not strictly increasing in
     * natural order (batch chain order, then record order), or one of them
     * does not fit [0, 2^32) relative to the first batch's base_offset: the
     * reference's result then depends on how compacted_offset_list aliases
     * offsets, which real segments never show */
    RPGPU_COMPACT_OFFSETS = 2,
};
/* spill_key_index::max_key_size (storage/spill_key_index.h:36): keys are
 * compared by their first 65515 bytes */
#define RPGPU_COMPACT_MAX_KEY 65515u

#define RPGPU_COMPACT_F_REWRITTEN (1u << 0) /* some records dropped: payload re-encoded, header rebuilt */

/* One entry per batch of the compacted output, in output order.  32 bytes. */
typedef struct rpgpu_compact_batch {
    uint64_t out_pos;      /* header position in d_out */
    uint32_t src_batch;    /* job-wide ordinal of the source batch */
    uint32_t payload_len;  /* bytes after the 61-byte header */
    uint32_t codec;        /* the source batch's codec (rpgpu_codec); the output is never compressed */
    uint32_t kept;         /* records in the output batch */
    uint32_t flags;        /* RPGPU_COMPACT_F_* */
    uint32_t reserved;
} rpgpu_compact_batch;

/* Per segment.  56 bytes. */
typedef struct rpgpu_compact_segment {
    uint32_t status;       /* rpgpu_compact_status; not OK: empty output, no keep bits */
    uint32_t reserved;
    uint64_t records_in;   /* records of the segment (0 unless OK) */
    uint64_t records_kept;
    uint64_t batches_in;
    uint64_t batches_out;
    uint64_t batches_rewritten;
    uint64_t bytes_out;
} rpgpu_compact_segment;

/* Whole call.  88 bytes. */
typedef struct rpgpu_compact_totals {
    uint64_t records_in, records_kept, batches_in, batches_out, batches_rewritten, bytes_out;
    uint64_t out_capacity_needed;        /* bytes_out + 16 */
    uint64_t out_batch_capacity_needed;  /* batches_out */
    uint32_t overflow;                   /* bit 0: out_capacity, bit 1: out_batch_capacity too small; nothing
                                            is then written to d_out / d_out_batches */
    uint32_t key_compare_mismatches;     /* key table slots whose tag matched a record of another key
                                            (resolved by comparing the key bytes; a count of work, not an
                                            error, and not reproducible from run to run) */
    uint64_t reserved[2];
} rpgpu_compact_totals;

/* All pointers are DEVICE pointers, caller-owned.  The first block is the
 * input and the outputs of a completed disk-layout rpgpu_submit with
 * RPGPU_JOB_CRC | RPGPU_JOB_PARSE | RPGPU_JOB_DECODE (same stream, or
 * synchronised). */
typedef struct rpgpu_compact_job {
    const uint8_t* d_data;
    const uint64_t* d_seg_offsets;       /* n_segments + 1 */
    uint32_t n_segments;
    uint32_t reserved;
    const rpgpu_batch_result* d_batches;
    uint64_t batch_capacity;             /* a bound of the source job's totals.n_batches (its batch_capacity, or
                                            the total itself): sizes grids and scratch */
    const rpgpu_record_index* d_records;
    uint64_t record_capacity;            /* likewise for totals.n_records; below 2^32 - 1 */
    const uint8_t* d_decoded;            /* may be NULL when no batch is compressed */
    const rpgpu_segment_summary* d_summaries;
    const rpgpu_job_totals* d_totals;
    /* outputs */
    uint64_t* d_keep;                    /* (record_capacity + 63) / 64 words: bit i = record-index slot i survives;
                                            zeroed by the call */
    uint8_t* d_out;                      /* the compacted segments back to back; 16-byte aligned */
    uint64_t out_capacity;               /* bytes, including 16 spare bytes past the last batch.  The sum of
                                            (61 + decoded_len) over the job's batches, plus 16, is always enough,
                                            except for a record whose header count runs past the end of its
                                            payload: the reference materialises that many empty headers and
                                            append_record_to_buffer writes two bytes for each */
    uint64_t* d_out_seg_offsets;         /* n_segments + 1: segment s's output is [s, s + 1) */
    rpgpu_compact_batch* d_out_batches;
    uint64_t out_batch_capacity;
    rpgpu_compact_segment* d_seg;        /* n_segments */
    rpgpu_compact_totals* d_ctotals;     /* one */
} rpgpu_compact_job;

/* For every segment of the job: which records survive key compaction, and
 * the compacted segment, i.e. the batches copy_data_segment_reducer::filter
 * returns, in order, back to back, headers stamped
 * (reset_size_checksum_metadata + header_crc).
 *   keep set   compaction_key_reducer with unbounded memory (its eviction
 *              under _max_mem only ever keeps more and follows absl's
 *              iteration order: not reproduced), then compacted_offset_list:
 *              per segment, of the records sharing a key (the first
 *              min(key_len, 65515) key bytes; null and empty are one key) the
 *              last in natural order survives.  Keys never match across
 *              segments; the batch type plays no part.
 *   filter     no record kept: the batch is dropped.  All kept: the batch
 *              passes with its (decoded) payload verbatim, a compressed one in
 *              its decompress_batch form (compression bits cleared, size / crc
 *              / header_crc reset = decoded_crc / decoded_header_crc).
 *              Otherwise the payload is append_record_to_buffer over the kept
 *              records (varints re-encoded canonically, the length field kept
 *              as parsed) and the header gets first_timestamp += ts_delta of
 *              the first kept record, max_timestamp = new first_timestamp +
 *              ts_delta of the last kept one unless attrs bit 3 (log append
 *              time) is set, record_count, compression bits cleared.
 * Recompression (do_compaction's compress_batch) is left to the caller:
 * every output batch reports its source codec for rpgpu_compress_batch.
 * A segment that is not eligible (rpgpu_compact_status) gets an empty output
 * and no keep bits; a segment without batches is OK and empty.
 * Asynchronous on `stream`; never writes out of bounds: a capacity that is
 * too small sets d_ctotals->overflow and reports the sizes needed.  NULL or
 * inconsistent arguments return RPGPU_E_INVALID without touching a device. */
int rpgpu_compact(rpgpu_ctx* ctx, const rpgpu_compact_job* job, void* stream);

/* sizeof of the compaction structs as compiled into the library: 0 =
 * rpgpu_compact_batch, 1 = rpgpu_compact_segment, 2 = rpgpu_compact_totals,
 * 3 = rpgpu_compact_job (0 for any other value). */
size_t rpgpu_compact_sizeof(int which);

/* Device time of the last timed rpgpu_compact (rpgpu_set_timing), in
 * milliseconds: 0 = whole call, 1 = eligibility + key insert, 2 = keep pass,
 * 3 = size pass + scans, 4 = write pass, 5 = stamp.  Synchronises on the
 * call's last event. */
int rpgpu_compact_timings(rpgpu_ctx* ctx, float* ms, int n);

/* ------------------------------------------------------------------------ */
/* Recompression of compacted batches: storage::internal::compress_batch     */
/* (storage/parser_utils.cc:82-120) as copy_data_segment_reducer::           */
/* do_compaction calls it on every batch filter() returns                    */
/* (storage/compaction_reducers.cc:223-258), and compress_batch_consumer     */
/* (parser_utils.cc:62-80).  Device-resident: rpgpu_compact's outputs in,    */
/* the on-disk compacted segments and the results of a validation job over   */
/* them out.                                                                 */
/* ------------------------------------------------------------------------ */
/* rpgpu_recompress_job.codec: every batch gets its rpgpu_compact_batch.codec,
 * do_compaction's `original` codec */
#define RPGPU_RECOMPRESS_SOURCE_CODEC 0xFFFFFFFFu

/* rpgpu_recompress_batch.flags */
#define RPGPU_RECOMPRESS_F_COMPRESSED (1u << 0) /* LZ4 / snappy (gzip with rpgpu_set_device_gzip): compressed here,
                                                   header restamped */
#define RPGPU_RECOMPRESS_F_HOST (1u << 1)       /* zstd (gzip without rpgpu_set_device_gzip): copied uncompressed,
                                                   the host's to finish with rpgpu_compress_batch */
#define RPGPU_RECOMPRESS_F_BAD_CODEC (1u << 2)  /* codec value 5..7: copied uncompressed */
#define RPGPU_RECOMPRESS_F_TOO_LARGE (1u << 3)  /* the compressed size bound (or a snappy fragment's bound, which
                                                   snappy-java frames as int32; for device gzip, deflateBound)
                                                   does not fit size_bytes: copied uncompressed */

/* One entry per output batch, in output (= input) order.  32 bytes. */
typedef struct rpgpu_recompress_batch {
    uint64_t out_pos;         /* header position in d_out */
    uint32_t in_batch;        /* ordinal of the batch in d_in_batches */
    uint32_t payload_len;     /* bytes after the 61-byte header in d_out */
    uint32_t in_payload_len;  /* the uncompressed payload's bytes */
    uint32_t codec;           /* the codec the batch was to get: the job's, or the entry's with
                                 RPGPU_RECOMPRESS_SOURCE_CODEC; RPGPU_CODEC_NONE for a batch below min_batch_bytes */
    uint32_t flags;           /* RPGPU_RECOMPRESS_F_*; 0: copied verbatim (codec none, or below min_batch_bytes) */
    uint32_t reserved;
} rpgpu_recompress_batch;

/* Whole call.  64 bytes. */
typedef struct rpgpu_recompress_totals {
    uint64_t batches_out;
    uint64_t batches_compressed;         /* RPGPU_RECOMPRESS_F_COMPRESSED */
    uint64_t batches_host;               /* RPGPU_RECOMPRESS_F_HOST (zstd batches only with rpgpu_set_device_gzip) */
    uint64_t bytes_in;                   /* 61 + payload_len over the input batches */
    uint64_t bytes_out;
    uint64_t out_capacity_needed;        /* bytes_out + 16 */
    uint64_t out_batch_capacity_needed;  /* batches_out */
    uint32_t overflow;                   /* bit 0: out_capacity, bit 1: out_batch_capacity too small: nothing is
                                            written to d_out / d_out_entries / d_out_batches, the sizes needed are
                                            reported.  Bit 2: the source d_ctotals->overflow != 0, or the input
                                            entries do not describe batches inside [0, in_capacity - 16): nothing
                                            is written, every count is 0 and every segment offset 0 */
    uint32_t reserved;
} rpgpu_recompress_totals;

/* All pointers are DEVICE pointers, caller-owned.  The first block is the
 * outputs of a completed rpgpu_compact (same stream, or synchronised): every
 * input batch is an uncompressed disk-layout batch, its stamped header at
 * out_pos and payload_len bytes behind it. */
typedef struct rpgpu_recompress_job {
    const uint8_t* d_in;                 /* rpgpu_compact's d_out */
    uint64_t in_capacity;                /* its out_capacity (with the 16 spare bytes): bounds the input bytes and
                                            sizes scratch */
    const uint64_t* d_in_seg_offsets;    /* n_segments + 1: rpgpu_compact's d_out_seg_offsets */
    uint32_t n_segments;
    uint32_t codec;                      /* RPGPU_RECOMPRESS_SOURCE_CODEC, or an rpgpu_codec value every batch gets
                                            (compress_batch_consumer's _compression_type; 5..7: see the flags) */
    const rpgpu_compact_batch* d_in_batches;
    uint64_t in_batch_capacity;          /* rpgpu_compact's out_batch_capacity */
    const rpgpu_compact_totals* d_ctotals; /* batches_out is the batch count, read on the device */
    uint64_t min_batch_bytes;            /* a batch with 61 + payload_len below it is copied verbatim
                                            (compress_batch_consumer's `>= _threshold`); 0: none */
    uint64_t snappy_frag;                /* the iobuf fragment size of every snappy payload, as rpgpu_compress_batch's
                                            frag (0: one fragment); a non-zero value below 4096 is invalid */
    /* outputs */
    uint8_t* d_out;                      /* the batches back to back, in input order; 16-byte aligned */
    uint64_t out_capacity;               /* bytes, including 16 spare bytes past the last batch.  The sum over the
                                            input batches of 61 + max(payload_len, rpgpu_compress_bound(codec,
                                            payload_len, snappy_frag)), plus 16, is always enough: a copied batch
                                            keeps its bytes; an LZ4 frame is at most 15 header bytes, a size word
                                            and at most the block's own bytes per 64 KiB block (a block that does
                                            not shrink is stored raw) and the end mark; a snappy-java payload is 16
                                            header bytes and per fragment a length word and a RawCompress output of
                                            at most snappy::MaxCompressedLength(fragment) -- the terms of
                                            rpgpu_compress_bound; a gzip payload compressed here
                                            (rpgpu_set_device_gzip) is at most deflateBound, payload_len +
                                            (payload_len >> 12) + (payload_len >> 14) + (payload_len >> 25) + 25,
                                            which rpgpu_compress_bound(RPGPU_CODEC_GZIP, ...) exceeds */
    uint64_t* d_out_seg_offsets;         /* n_segments + 1: segment s's output is [s, s + 1) */
    rpgpu_recompress_batch* d_out_entries;
    rpgpu_batch_result* d_out_batches;   /* one per output batch, in output order */
    uint64_t out_batch_capacity;         /* of d_out_entries and of d_out_batches */
    rpgpu_segment_summary* d_out_summaries; /* n_segments */
    rpgpu_recompress_totals* d_rtotals;  /* one */
} rpgpu_recompress_job;

/* Per batch, by its effective codec (the job's, or the entry's):
 *   LZ4, snappy   the payload becomes exactly what rpgpu_compress_batch
 *                 returns for those bytes (snappy: over snappy_frag-byte
 *                 fragments); the header is the input header with attrs |=
 *                 codec, size_bytes = 61 + the compressed length, crc =
 *                 crc_record_batch over the new header and payload, then
 *                 header_crc (compress_batch + reset_size_checksum_metadata);
 *                 every other field is unchanged.  The compressed form is
 *                 kept even when it is larger, as the reference keeps it.
 *   none, or 61 + payload_len < min_batch_bytes
 *                 the batch's bytes verbatim.
 *   gzip, zstd    the batch's bytes verbatim, still uncompressed (the log
 *                 stays valid), flagged RPGPU_RECOMPRESS_F_HOST.
 *   gzip, with rpgpu_set_device_gzip on
 *                 compressed where it lies, as LZ4 above: the payload becomes
 *                 what rpgpu_compress_batch returns for those bytes fed as
 *                 ONE fragment (frag 0), RPGPU_RECOMPRESS_F_COMPRESSED.  The
 *                 iobuf fragments of a rewritten payload are not known here;
 *                 zlib 1.2.11's output did not depend on the fragmentation in
 *                 any of 1800 fragmentations of 300 inputs tried (nor in this
 *                 project's tests), but that is observed, not proven, so the
 *                 reference's bytes are promised relative to one fragment, as
 *                 snappy's are relative to snappy_frag.  A payload whose
 *                 deflateBound plus 61 does not fit int32 is copied
 *                 uncompressed, RPGPU_RECOMPRESS_F_TOO_LARGE.  batches_host
 *                 then counts zstd batches only.
 *   5..7          verbatim, RPGPU_RECOMPRESS_F_BAD_CODEC.
 * LZ4 frames do not depend on the iobuf's fragmentation
 * (lz4_frame_compressor.cc:69-113), so the reference's bytes are promised
 * outright; snappy-java's are promised relative to snappy_frag.
 *
 * d_out_batches and d_out_summaries hold exactly what a disk-layout
 * rpgpu_submit with RPGPU_JOB_CRC alone over d_out / d_out_seg_offsets
 * reports (index_base = decoded_off = 0, decoded_len = payload_len for an
 * uncompressed batch and 0 for a compressed one), so rpgpu_segment_index
 * and rpgpu_fetch take them without another validation pass.
 *
 * Asynchronous on `stream`; never writes out of bounds: a capacity that is
 * too small sets d_rtotals->overflow and reports the sizes needed.  NULL or
 * inconsistent arguments return RPGPU_E_INVALID without touching a device. */
int rpgpu_recompress(rpgpu_ctx* ctx, const rpgpu_recompress_job* job, void* stream);

/* sizeof of the recompression structs as compiled into the library: 0 =
 * rpgpu_recompress_batch, 1 = rpgpu_recompress_totals, 2 = rpgpu_batch_result,
 * 3 = rpgpu_recompress_job (0 for any other value). */
size_t rpgpu_recompress_sizeof(int which);

/* Device time of the last timed rpgpu_recompress (rpgpu_set_timing), in
 * milliseconds: 0 = whole call, 1 = plan, 2 = block compression, 3 = scans +
 * layout, 4 = pack + copy, 5 = stamp + output metadata.  Synchronises on the
 * call's last event. */
int rpgpu_recompress_timings(rpgpu_ctx* ctx, float* ms, int n);

/* ------------------------------------------------------------------------ */
/* Produce path: validated Kafka v2 record sets -> the bytes the log         */
/* receives (kafka_batch_adapter::adapt, kafka/protocol/                     */
/* kafka_batch_adapter.cc:32-91, :126-188; the partition verdict of          */
/* kafka/server/handlers/produce.cc:364-412; set_max_timestamp for append    */
/* time topics, produce.cc:223-232, model/record.h:598-608;                  */
/* disk_log_appender::operator(), storage/disk_log_appender.cc:72-74,        */
/* :113-119).                                                                */
/* ------------------------------------------------------------------------ */
/* rpgpu_append_set.status: what the produce handler answers for the
 * partition.  Per batch the first failing test wins, in the order
 * batch_reader::consume_batch / adapt() meet them:
 *   not RPGPU_F_COMPLETE        MALFORMED        (share() / skip throws)
 *   not RPGPU_F_WIRE_V2         CORRUPT_MESSAGE  (produce.cc:385 tests valid_crc before v2_format; the
 *                                                 reference leaves valid_crc unset for a batch that is not v2,
 *                                                 this surface pins it to false)
 *   not RPGPU_F_CRC_OK          CORRUPT_MESSAGE
 *   RPGPU_F_CODEC_INVALID       MALFORMED        (attrs.compression() throws out of adapt)
 *   not compressed and not
 *   RPGPU_F_PARSE_OK            INVALID_RECORD   (adapt leaves `batch` empty)
 */
enum rpgpu_append_status {
    RPGPU_APPEND_OK = 0,
    RPGPU_APPEND_CORRUPT_MESSAGE = 1,
    RPGPU_APPEND_INVALID_RECORD = 2,
    RPGPU_APPEND_MALFORMED = 3,
    RPGPU_APPEND_SOURCE_OVERFLOW = 4, /* the source job's totals.overflow != 0: every set gets this */
};

/* rpgpu_append_job.flags.  Without it the produce rule holds: only the first
 * batch on a set's chain is looked at and appended, whatever follows is
 * ignored (adapt()'s remainder is dropped), and a set without a batch on its
 * chain (empty, shorter than 61 bytes, batch_length + 12 < 61) is MALFORMED.
 * With it, the loop of kafka/protocol/kafka_batch_adapter.h:44-49: every
 * batch on the chain is appended in chain order; the set is accepted only if
 * every batch is and the chain ended with RPGPU_ERRC_END_OF_STREAM (an empty
 * set: the loop does not run, nothing is appended, status OK); otherwise its
 * status is the first failing batch's, or MALFORMED for a bad terminal. */
#define RPGPU_APPEND_ALL_BATCHES (1u << 0)

/* d_append_time[s] for a topic with create time: batches keep their
 * timestamps.  Any other value t applies set_max_timestamp(append_time, t). */
#define RPGPU_APPEND_CREATE_TIME INT64_MIN

/* Per record set (partition).  40 bytes. */
typedef struct rpgpu_append_set {
    uint32_t status;      /* rpgpu_append_status; not OK: nothing written, no offsets consumed */
    uint32_t first_bad;   /* set-relative chain ordinal of the batch that decided the status, or the chain's
                             batch count when no batch did (0 for SOURCE_OVERFLOW) */
    uint64_t n_batches;   /* batches appended */
    int64_t base_offset;  /* first offset assigned (= next_offset) */
    int64_t last_offset;  /* last offset assigned; next_offset - 1 when nothing was appended: the produce
                             response's value and, + 1, the next call's next_offset */
    uint64_t bytes_out;
} rpgpu_append_set;

/* Whole call.  64 bytes. */
typedef struct rpgpu_append_totals {
    uint64_t sets_ok;
    uint64_t batches_out;
    uint64_t bytes_out;
    uint64_t out_capacity_needed;        /* bytes_out + 16 */
    uint64_t out_batch_capacity_needed;  /* batches_out */
    uint32_t overflow;                   /* bit 0: out_capacity, bit 1: out_batch_capacity too small; nothing
                                            is then written to d_out / d_out_batches */
    uint32_t reserved0;
    uint64_t reserved[2];
} rpgpu_append_totals;

/* All pointers are DEVICE pointers, caller-owned.  The first block is the
 * input and the outputs of a completed RPGPU_LAYOUT_WIRE rpgpu_submit with at
 * least RPGPU_JOB_CRC | RPGPU_JOB_PARSE (same stream, or synchronised); one
 * segment of that job is one partition's record set. */
typedef struct rpgpu_append_job {
    const uint8_t* d_data;
    const uint64_t* d_seg_offsets;       /* n_segments + 1 */
    uint32_t n_segments;
    uint32_t flags;                      /* RPGPU_APPEND_* */
    const rpgpu_batch_result* d_batches;
    uint64_t batch_capacity;             /* a bound of the source job's totals.n_batches (its batch_capacity, or
                                            the total itself): sizes grids and scratch */
    const rpgpu_segment_summary* d_summaries;
    const rpgpu_job_totals* d_totals;
    const int64_t* d_next_offset;        /* n_segments: each partition's appender _idx */
    const int64_t* d_append_time;        /* n_segments, or NULL (every topic uses create time) */
    /* outputs */
    uint8_t* d_out;                      /* the accepted sets back to back, in set order; 16-byte aligned */
    uint64_t out_capacity;               /* bytes, including 16 spare bytes past the last batch: the source
                                            batches' size_bytes summed, plus 16, is always enough */
    uint64_t* d_out_seg_offsets;         /* n_segments + 1: set s's bytes are [s, s + 1) */
    rpgpu_batch_result* d_out_batches;   /* one per appended batch, in output order */
    uint64_t out_batch_capacity;
    rpgpu_segment_summary* d_out_summaries; /* n_segments */
    rpgpu_append_set* d_sets;            /* n_segments */
    rpgpu_append_totals* d_atotals;      /* one */
} rpgpu_append_job;

/* Every appended batch is its 61-byte little-endian disk header
 * (storage/segment_appender_utils.cc:28-54) followed by its payload verbatim:
 * header_crc = internal_header_only_crc of the final header, size_bytes =
 * batch_length + 12, base_offset = the set's next_offset for its first batch
 * and the previous base_offset + last_offset_delta + 1 after that, type 1
 * (raft_data), crc as on the wire, attrs .. record_count byte-reversed.  For
 * a set with an append time t every appended batch gets attrs bit 3 and
 * max_timestamp = t, and crc (crc_record_batch) is recomputed before
 * header_crc.
 *
 * d_out_batches[i] holds what a disk-layout rpgpu_submit over d_out /
 * d_out_seg_offsets with the source job's flags reports for that batch,
 * except: index_base and decoded_off keep the source entry's values (the
 * source job's record index and decoded arena stay valid for the payload:
 * record positions are payload-relative, but record_index.batch keeps the
 * source ordinals, so rpgpu_compact over these outputs is not promised), and
 * decoded_crc / decoded_header_crc are 0 (they describe decompress_batch's
 * form of the batch, which the append does not produce).  d_out_summaries[s]
 * is that job's summary of output segment s with n_records = 0 (the record
 * index stays the source's); a rejected or empty set gets the summary of an
 * empty segment.  Both feed rpgpu_segment_index and rpgpu_serialize_wire
 * without another validation pass.
 *
 * Asynchronous on `stream`; never writes out of bounds: a capacity that is
 * too small sets d_atotals->overflow and reports the sizes needed.  NULL or
 * inconsistent arguments return RPGPU_E_INVALID without touching a device. */
int rpgpu_append_wire(rpgpu_ctx* ctx, const rpgpu_append_job* job, void* stream);

/* sizeof of the append structs as compiled into the library: 0 =
 * rpgpu_append_set, 1 = rpgpu_append_totals, 2 = rpgpu_batch_result (the
 * entries of d_out_batches), 3 = rpgpu_append_job (0 for any other value). */
size_t rpgpu_append_sizeof(int which);

/* Device time of the last timed rpgpu_append_wire (rpgpu_set_timing), in
 * milliseconds: 0 = whole call, 1 = verdicts + sizes, 2 = scans + plan,
 * 3 = copy, 4 = append-time stamp, 5 = output metadata.  Synchronises on the
 * call's last event. */
int rpgpu_append_timings(rpgpu_ctx* ctx, float* ms, int n);

/* ------------------------------------------------------------------------ */
/* Fetch path: the log read of a Kafka fetch, many partitions per call.      */
/* storage::log_reader over the partition's segments, driven by              */
/* skipping_consumer (storage/log_reader.cc:26-119, :212-343) under a        */
/* log_reader_config (storage/types.h:201-270); the accepted batches folded  */
/* through kafka_batch_serializer (kafka/protocol/batch_consumer.h:27-78)    */
/* into the partition's wire record set (kafka/server/handlers/fetch.cc:     */
/* 128-173).  disk_log_impl::timequery is the same read with a 2048-byte     */
/* budget and a timestamp bound (storage/disk_log_impl.cc:861-917).          */
/* ------------------------------------------------------------------------ */
enum rpgpu_fetch_status {
    RPGPU_FETCH_OK = 0,
    RPGPU_FETCH_OFFSETS = 1,         /* a visited batch's base_offset lies below the consumer's expected offset:
                                        the reference throws "incorrect offset encountered reading from disk log" */
    RPGPU_FETCH_SOURCE_OVERFLOW = 2, /* the source job's totals.overflow != 0: every partition gets this */
};

/* rpgpu_fetch_request.flags */
#define RPGPU_FETCH_STRICT_MAX_BYTES (1u << 0) /* log_reader_config::strict_max_bytes */
#define RPGPU_FETCH_TYPE_FILTER (1u << 1)      /* type_filter has a value (type 0 is a legal value) */
#define RPGPU_FETCH_FIRST_TIMESTAMP (1u << 2)  /* first_timestamp has a value */

/* Per partition: the log_reader_config of its read.  40 bytes. */
typedef struct rpgpu_fetch_request {
    int64_t start_offset;    /* inclusive */
    int64_t max_offset;      /* inclusive */
    uint64_t max_bytes;
    int64_t first_timestamp; /* with RPGPU_FETCH_FIRST_TIMESTAMP */
    uint32_t flags;          /* RPGPU_FETCH_*; other bits are ignored */
    int8_t type_filter;      /* with RPGPU_FETCH_TYPE_FILTER */
    uint8_t pad[3];
} rpgpu_fetch_request;

/* Per partition.  64 bytes. */
typedef struct rpgpu_fetch_part {
    uint32_t status;         /* rpgpu_fetch_status; not OK: nothing written, n_batches = bytes_out = 0 */
    uint32_t over_budget;    /* log_reader_config::over_budget when the read ended */
    uint64_t n_batches;      /* batches returned */
    uint32_t first_out;      /* their first slot in d_out_batches (slots are counted in 32 bits:
                                out_batch_capacity < 2^31) */
    uint32_t record_count;   /* kafka_batch_serializer::result::record_count: the returned batches' record_count
                                summed with uint32 wraparound, as the serializer does.  It shares first_out's
                                eight bytes so that the struct stays 64 bytes */
    uint64_t bytes_out;
    int64_t base_offset;     /* kafka_batch_serializer::result; INT64_MIN (model::offset{}) when nothing was returned */
    int64_t last_offset;     /* likewise.  With RPGPU_FETCH_OFFSETS the two hold what the reference's exception
                                names: base_offset the expected batch offset, last_offset the actual one */
    int64_t next_offset;     /* _config.start_offset when the read ended: the next fetch's start */
    int64_t first_timestamp; /* the first returned batch's (timequery_result.time); -1 when none */
} rpgpu_fetch_part;

/* One entry per returned batch, in output order.  16 bytes. */
typedef struct rpgpu_fetch_batch {
    uint64_t out_pos;   /* its wire header's position in d_out */
    uint32_t src_batch; /* job-wide ordinal of the source batch */
    uint32_t partition;
} rpgpu_fetch_batch;

/* Whole call.  64 bytes. */
typedef struct rpgpu_fetch_totals {
    uint64_t parts_ok;
    uint64_t batches_out;
    uint64_t bytes_out;
    uint64_t out_capacity_needed;       /* bytes_out + 16 */
    uint64_t out_batch_capacity_needed; /* batches_out */
    uint32_t overflow;                  /* bit 0: out_capacity, bit 1: out_batch_capacity too small; nothing is
                                           then written to d_out / d_out_batches */
    uint32_t reserved0;
    uint64_t reserved[2];
} rpgpu_fetch_totals;

/* All pointers are DEVICE pointers, caller-owned.  The first block is the
 * input and the outputs of a completed RPGPU_LAYOUT_DISK rpgpu_submit with at
 * least RPGPU_JOB_CRC (same stream, or synchronised). */
typedef struct rpgpu_fetch_job {
    const uint8_t* d_data;
    const uint64_t* d_seg_offsets;       /* n_segments + 1 */
    uint32_t n_segments;
    uint32_t n_partitions;
    const rpgpu_batch_result* d_batches;
    uint64_t batch_capacity;             /* a bound of the source job's totals.n_batches (its batch_capacity, or
                                            the total itself): sizes grids and scratch */
    const rpgpu_segment_summary* d_summaries;
    const rpgpu_job_totals* d_totals;
    /* partition p is the job's segments [d_part_segments[p],
     * d_part_segments[p + 1]), in log order: n_partitions + 1 ascending
     * entries; equal neighbours give a partition without segments.  Entries
     * are clamped to n_segments and to their predecessor on the device. */
    const uint32_t* d_part_segments;
    const rpgpu_fetch_request* d_requests; /* n_partitions */
    /* optional entry index: all three NULL, or the outputs of
     * rpgpu_segment_index over this job (batch_capacity entries each) */
    const rpgpu_index_state* d_index_states;
    const uint32_t* d_rel_offset;
    const uint64_t* d_position;
    /* outputs */
    uint8_t* d_out;                      /* the partitions' record sets back to back; 16-byte aligned */
    uint64_t out_capacity;               /* bytes, including 16 spare bytes past the last batch: the partitions'
                                            max_bytes summed, plus each partition's largest batch, plus 16 always
                                            suffices; so does the source bytes + 16 */
    uint64_t* d_out_part_offsets;        /* n_partitions + 1: partition p's bytes are [p, p + 1) */
    rpgpu_fetch_batch* d_out_batches;
    uint64_t out_batch_capacity;
    rpgpu_fetch_part* d_parts;           /* n_partitions */
    rpgpu_fetch_totals* d_ftotals;       /* one */
} rpgpu_fetch_job;

/* The read, exactly.  Arithmetic on offsets wraps (two's complement int64);
 * last_offset = base_offset + last_offset_delta.
 *
 * A segment's chain for this call is its RPGPU_F_COMPLETE batches, in chain
 * order (an incomplete batch can only be the last, and the reference never
 * delivers it).  A segment without one is empty and is skipped.  A segment's
 * dirty_offset is the last_offset of its last chain batch.  CRC flags play no
 * part: skipping_consumer does not check the batch crc, a batch without
 * RPGPU_F_CRC_OK is returned verbatim.  The batch cache is cold, there is no
 * timeout and no abort source.
 *
 * Per partition: start = start_offset, consumed = 0, over_budget = false.
 * For each non-empty segment in order:
 *   1. start > dirty_offset: next segment (find_next_valid_iterator).
 *   2. Otherwise a fresh consumer starts with expected = INT64_MIN,
 *   3. at the segment's first chain batch, or
 *   4. with the index arrays at the chain batch whose file_pos is
 *      segment_index::find_nearest(start)'s position (storage/segment.cc:
 *      451-459, storage/segment_index.cc:95-120; `start` as it is when the
 *      segment is entered; needle = (uint32)(start - index_state.base_offset),
 *      std::lower_bound over the segment's relative offsets, the last entry
 *      when it runs off the end, then downwards to the first entry <= needle;
 *      no entry, an empty index or start < base_offset: the first chain
 *      batch).  If no chain batch has that position, the first one with
 *      file_pos >= it.
 * Then for each batch b from there, the first rule that applies:
 *   1. b.base_offset < expected: status RPGPU_FETCH_OFFSETS, the read ends
 *      and nothing of the partition is returned.
 *   2. b.base_offset > max_offset: the read ends.
 *   3. (strict || consumed != 0) && consumed + (uint64)(int64)b.size_bytes >
 *      max_bytes, in wrapping uint64 arithmetic: over_budget = true, the
 *      read ends.
 *   4. b.last_offset < start: expected = b.last_offset + 1, next batch.
 *   5. type filter set and != b.type: start = expected = b.last_offset + 1,
 *      next batch.
 *   6. first timestamp set and > b.first_timestamp: as 5.
 *   7. The batch is returned; expected = start = b.last_offset + 1, consumed
 *      += size_bytes; b.last_offset >= max_offset or consumed > max_bytes:
 *      the read ends.  With consumed == max_bytes it goes on, and rule 3 ends
 *      it at the next batch it visits.
 * Running off a segment's chain moves to the next segment, whatever its
 * terminal_errc is: a torn or fallocated tail is invisible to a reader, whose
 * `start` is then past the segment's dirty_offset.  Rule 1 counts only at a
 * batch the reader visits: not beyond the stop point, and not across
 * segments (every segment gets a fresh consumer).
 *
 * The output: partition p's returned batches in order, each as
 * kafka::writer_serialize_batch writes it (kafka/protocol/response_writer.h:
 * 241-276, rpgpu_serialize_wire's transform; base_offset stays the log's),
 * back to back in d_out[d_out_part_offsets[p], d_out_part_offsets[p + 1]),
 * the partitions back to back in partition order.  A partition whose status
 * is not OK returns nothing; its next_offset and over_budget are those of
 * the moment the read ended (SOURCE_OVERFLOW: start_offset, 0).
 *
 * Asynchronous on `stream`; never writes out of bounds: a capacity that is
 * too small sets d_ftotals->overflow and reports the sizes needed (d_parts
 * and d_out_part_offsets are written all the same).  NULL or inconsistent
 * arguments return RPGPU_E_INVALID without touching a device. */
int rpgpu_fetch(rpgpu_ctx* ctx, const rpgpu_fetch_job* job, void* stream);

/* sizeof of the fetch structs as compiled into the library: 0 =
 * rpgpu_fetch_request, 1 = rpgpu_fetch_part, 2 = rpgpu_fetch_batch, 3 =
 * rpgpu_fetch_totals, 4 = rpgpu_fetch_job (0 for any other value). */
size_t rpgpu_fetch_sizeof(int which);

/* Device time of the last timed rpgpu_fetch (rpgpu_set_timing), in
 * milliseconds: 0 = whole call, 1 = select, 2 = scans + plan, 3 = copy,
 * 4 = output metadata (d_out_batches is written by the copy's first piece of
 * each batch, so this is the empty interval behind it).  Synchronises on the
 * call's last event. */
int rpgpu_fetch_timings(rpgpu_ctx* ctx, float* ms, int n);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RPGPU_H_ */
