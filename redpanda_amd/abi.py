"""numpy mirrors of the C-ABI data layouts declared in include/rpgpu.h.

These are layouts only (no logic): the product wrapper (`redpanda_amd._lib`),
the tests and the oracle wrapper all view device/host result buffers through
them, so parity checks are plain array comparisons.
"""
import numpy as np

HEADER_SIZE = 61

CODEC_NONE, CODEC_GZIP, CODEC_SNAPPY, CODEC_LZ4, CODEC_ZSTD = 0, 1, 2, 3, 4
# rpgpu_status
OK, E_INVALID, E_NO_DEVICE, E_NOMEM, E_OVERFLOW, E_CODEC, E_UNSUPPORTED, E_HIP = 0, -1, -2, -3, -4, -5, -6, -7
PENDING = 1
# rpgpu_stamp flags
STAMP_OFFSETS, STAMP_CRC = 1, 2

ERRC_NONE = 0
ERRC_END_OF_STREAM = 1
ERRC_HEADER_ONLY_CRC_MISSMATCH = 2
ERRC_INPUT_STREAM_NOT_ENOUGH_BYTES = 3
ERRC_FALLOCATED_FILE_READ_ZERO_BYTES_FOR_HEADER = 4
ERRC_NOT_ENOUGH_BYTES_IN_PARSER_FOR_ONE_RECORD = 5

F_HEADER_OK = 1 << 0
F_COMPLETE = 1 << 1
F_CRC_OK = 1 << 2
F_COMPRESSED = 1 << 3
F_CODEC_INVALID = 1 << 4
F_CODEC_UNSUPPORTED = 1 << 5
F_CODEC_OK = 1 << 6
F_PARSED = 1 << 7
F_PARSE_ASYNC_OK = 1 << 8
F_PARSE_OK = 1 << 9
F_INDEX_WRITTEN = 1 << 10
F_WIRE_V2 = 1 << 11
F_DECODE_OVERFLOW = 1 << 12

PARSE_ERR_NONE = 0
PARSE_ERR_ATTR_EOF = 1
PARSE_ERR_COPY_NEGATIVE = 2
PARSE_ERR_HEADER_RESERVE = 3
PARSE_ERR_TRAILING = 4
PARSE_ERR_INDEX_CAPACITY = 5

JOB_CRC = 1 << 0
JOB_PARSE = 1 << 1
JOB_DECODE = 1 << 2
JOB_HOST_CODECS = 1 << 3

LAYOUT_DISK = 0
LAYOUT_WIRE = 1

BATCH_RESULT = np.dtype([
    ("file_pos", "<u8"), ("base_offset", "<i8"), ("first_timestamp", "<i8"),
    ("max_timestamp", "<i8"), ("producer_id", "<i8"), ("size_bytes", "<i4"),
    ("record_count", "<i4"), ("last_offset_delta", "<i4"), ("base_sequence", "<i4"),
    ("header_crc", "<u4"), ("crc", "<u4"), ("crc_computed", "<u4"),
    ("header_crc_computed", "<u4"), ("flags", "<u4"), ("segment", "<u4"),
    ("index_base", "<u8"), ("decoded_off", "<u8"), ("records_parsed", "<u4"),
    ("decoded_len", "<u4"), ("decoded_crc", "<u4"), ("decoded_header_crc", "<u4"),
    ("attrs", "<i2"), ("producer_epoch", "<i2"), ("type", "i1"), ("parse_err", "u1"),
    ("reserved0", "<u2"), ("reserved1", "<u8"),
])
assert BATCH_RESULT.itemsize == 128

RECORD_INDEX = np.dtype([
    ("batch", "<u4"), ("rec_pos", "<u4"), ("ts_delta", "<i8"), ("length", "<i4"),
    ("offset_delta", "<i4"), ("key_len", "<i4"), ("key_pos", "<u4"), ("val_len", "<i4"),
    ("val_pos", "<u4"), ("hdr_count", "<i4"), ("hdr_pos", "<u4"), ("end_pos", "<u4"),
    ("attrs", "i1"), ("pad", "u1", (3,)), ("reserved", "<u4", (2,)),
])
assert RECORD_INDEX.itemsize == 64

SEGMENT_SUMMARY = np.dtype([
    ("first_batch", "<u8"), ("n_batches", "<u8"), ("terminal_pos", "<u8"),
    ("bytes_consumed", "<u8"), ("terminal_errc", "<i4"), ("terminal_eof", "<i4"),
    ("has_checkpoint", "<i4"), ("first_bad", "<u4"), ("ckpt_last_offset", "<i8"),
    ("ckpt_truncate_pos", "<u8"), ("n_records", "<u8"), ("reserved", "<u8", (2,)),
])
assert SEGMENT_SUMMARY.itemsize == 88

# rpgpu_index_state (include/rpgpu.h): index_state header after recovery
INDEX_STATE = np.dtype([
    ("base_offset", "<i8"), ("max_offset", "<i8"), ("base_timestamp", "<i8"),
    ("max_timestamp", "<i8"), ("first_entry", "<u8"), ("n_entries", "<u8"),
    ("assert_batch", "<i8"), ("tracked", "<u8"),
])
assert INDEX_STATE.itemsize == 64
INDEX_DEFAULT_STEP = 32768  # segment_index::default_data_buffer_step (storage/segment_index.h:49)

JOB_TOTALS = np.dtype([
    ("n_batches", "<u8"), ("n_records", "<u8"), ("decoded_bytes", "<u8"),
    ("batch_capacity_needed", "<u8"), ("record_capacity_needed", "<u8"),
    ("decoded_capacity_needed", "<u8"), ("overflow", "<u4"), ("n_rewalks", "<u4"),
    ("reserved", "<u8", (2,)),
])
assert JOB_TOTALS.itemsize == 72

# rpgpu_compact (include/rpgpu.h): key compaction of segments
COMPACT_OK, COMPACT_NOT_CLEAN, COMPACT_OFFSETS = 0, 1, 2
COMPACT_MAX_KEY = 65515  # spill_key_index::max_key_size (storage/spill_key_index.h:36)
COMPACT_F_REWRITTEN = 1 << 0

COMPACT_BATCH = np.dtype([
    ("out_pos", "<u8"), ("src_batch", "<u4"), ("payload_len", "<u4"), ("codec", "<u4"), ("kept", "<u4"),
    ("flags", "<u4"), ("reserved", "<u4"),
])
assert COMPACT_BATCH.itemsize == 32
COMPACT_SEGMENT = np.dtype([
    ("status", "<u4"), ("reserved", "<u4"), ("records_in", "<u8"), ("records_kept", "<u8"), ("batches_in", "<u8"),
    ("batches_out", "<u8"), ("batches_rewritten", "<u8"), ("bytes_out", "<u8"),
])
assert COMPACT_SEGMENT.itemsize == 56
COMPACT_TOTALS = np.dtype([
    ("records_in", "<u8"), ("records_kept", "<u8"), ("batches_in", "<u8"), ("batches_out", "<u8"),
    ("batches_rewritten", "<u8"), ("bytes_out", "<u8"), ("out_capacity_needed", "<u8"),
    ("out_batch_capacity_needed", "<u8"), ("overflow", "<u4"), ("key_compare_mismatches", "<u4"),
    ("reserved", "<u8", (2,)),
])
assert COMPACT_TOTALS.itemsize == 88
COMPACT_BATCH_COMPARE_FIELDS = [n for n in COMPACT_BATCH.names if n != "reserved"]
COMPACT_SEGMENT_COMPARE_FIELDS = [n for n in COMPACT_SEGMENT.names if n != "reserved"]
# key_compare_mismatches counts work (it depends on the insertion order), not a result
COMPACT_TOTALS_COMPARE_FIELDS = [n for n in COMPACT_TOTALS.names if n not in ("reserved", "key_compare_mismatches")]

# rpgpu_recompress (include/rpgpu.h): recompression of compacted batches
RECOMPRESS_SOURCE_CODEC = 0xFFFFFFFF
RECOMPRESS_F_COMPRESSED, RECOMPRESS_F_HOST, RECOMPRESS_F_BAD_CODEC, RECOMPRESS_F_TOO_LARGE = 1 << 0, 1 << 1, 1 << 2, 1 << 3

RECOMPRESS_BATCH = np.dtype([
    ("out_pos", "<u8"), ("in_batch", "<u4"), ("payload_len", "<u4"), ("in_payload_len", "<u4"), ("codec", "<u4"),
    ("flags", "<u4"), ("reserved", "<u4"),
])
assert RECOMPRESS_BATCH.itemsize == 32
RECOMPRESS_TOTALS = np.dtype([
    ("batches_out", "<u8"), ("batches_compressed", "<u8"), ("batches_host", "<u8"), ("bytes_in", "<u8"),
    ("bytes_out", "<u8"), ("out_capacity_needed", "<u8"), ("out_batch_capacity_needed", "<u8"), ("overflow", "<u4"),
    ("reserved", "<u4"),
])
assert RECOMPRESS_TOTALS.itemsize == 64
RECOMPRESS_BATCH_COMPARE_FIELDS = [n for n in RECOMPRESS_BATCH.names if n != "reserved"]
RECOMPRESS_TOTALS_COMPARE_FIELDS = [n for n in RECOMPRESS_TOTALS.names if n != "reserved"]

# rpgpu_append_wire (include/rpgpu.h): produce-path append of wire record sets
APPEND_OK, APPEND_CORRUPT_MESSAGE, APPEND_INVALID_RECORD, APPEND_MALFORMED, APPEND_SOURCE_OVERFLOW = 0, 1, 2, 3, 4
APPEND_ALL_BATCHES = 1 << 0
APPEND_CREATE_TIME = -(1 << 63)  # INT64_MIN: the topic uses create time

APPEND_SET = np.dtype([
    ("status", "<u4"), ("first_bad", "<u4"), ("n_batches", "<u8"), ("base_offset", "<i8"), ("last_offset", "<i8"),
    ("bytes_out", "<u8"),
])
assert APPEND_SET.itemsize == 40
APPEND_TOTALS = np.dtype([
    ("sets_ok", "<u8"), ("batches_out", "<u8"), ("bytes_out", "<u8"), ("out_capacity_needed", "<u8"),
    ("out_batch_capacity_needed", "<u8"), ("overflow", "<u4"), ("reserved0", "<u4"), ("reserved", "<u8", (2,)),
])
assert APPEND_TOTALS.itemsize == 64
APPEND_SET_COMPARE_FIELDS = list(APPEND_SET.names)
APPEND_TOTALS_COMPARE_FIELDS = [n for n in APPEND_TOTALS.names if not n.startswith("reserved")]
# d_out_summaries: n_records is 0 by contract (the record index stays the source job's)
APPEND_SUMMARY_COMPARE_FIELDS = [n for n in SEGMENT_SUMMARY.names if n != "reserved"]

# rpgpu_fetch (include/rpgpu.h): the fetch path's log read
FETCH_OK, FETCH_OFFSETS, FETCH_SOURCE_OVERFLOW = 0, 1, 2
FETCH_STRICT_MAX_BYTES, FETCH_TYPE_FILTER, FETCH_FIRST_TIMESTAMP = 1 << 0, 1 << 1, 1 << 2
OFFSET_MIN = -(1 << 63)  # model::offset{}: base_offset / last_offset of a read that returned nothing

FETCH_REQUEST = np.dtype([
    ("start_offset", "<i8"), ("max_offset", "<i8"), ("max_bytes", "<u8"), ("first_timestamp", "<i8"),
    ("flags", "<u4"), ("type_filter", "i1"), ("pad", "u1", (3,)),
])
assert FETCH_REQUEST.itemsize == 40
FETCH_PART = np.dtype([
    ("status", "<u4"), ("over_budget", "<u4"), ("n_batches", "<u8"), ("first_out", "<u4"), ("record_count", "<u4"),
    ("bytes_out", "<u8"), ("base_offset", "<i8"), ("last_offset", "<i8"), ("next_offset", "<i8"),
    ("first_timestamp", "<i8"),
])
assert FETCH_PART.itemsize == 64
FETCH_BATCH = np.dtype([("out_pos", "<u8"), ("src_batch", "<u4"), ("partition", "<u4")])
assert FETCH_BATCH.itemsize == 16
FETCH_TOTALS = np.dtype([
    ("parts_ok", "<u8"), ("batches_out", "<u8"), ("bytes_out", "<u8"), ("out_capacity_needed", "<u8"),
    ("out_batch_capacity_needed", "<u8"), ("overflow", "<u4"), ("reserved0", "<u4"), ("reserved", "<u8", (2,)),
])
assert FETCH_TOTALS.itemsize == 64
FETCH_PART_COMPARE_FIELDS = list(FETCH_PART.names)
FETCH_BATCH_COMPARE_FIELDS = list(FETCH_BATCH.names)
FETCH_TOTALS_COMPARE_FIELDS = [n for n in FETCH_TOTALS.names if not n.startswith("reserved")]

# fields of rpgpu_batch_result that are outputs of the engine and compared
# bit-exactly against the oracle (reserved fields excluded)
BATCH_COMPARE_FIELDS = [n for n in BATCH_RESULT.names if not n.startswith("reserved")]
RECORD_COMPARE_FIELDS = [n for n in RECORD_INDEX.names if n not in ("pad", "reserved")]
SUMMARY_COMPARE_FIELDS = [n for n in SEGMENT_SUMMARY.names if n != "reserved"]
