// rp_runtime.hip — host side of the C-ABI (include/rpgpu.h): contexts,
// constant tables, the submit pipeline, memory helpers, the host CRC32C
// behind crc::crc32c and the synthetic segment generator.
#include <hip/hip_runtime.h>
#include <nmmintrin.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "rp_device.h"
#include "rp_hostcodec.h"

namespace rp {

// ---------------------------------------------------------------------------
// GF(2) helpers for the CRC tables (reflected CRC32C)
// ---------------------------------------------------------------------------
static uint32_t raw_step_zero(uint32_t c, const uint32_t* t0) { return t0[c & 0xFF] ^ (c >> 8); }

static void build_tables(Tables* T) {
    uint32_t t0[256];
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        t0[i] = c;
    }
    // T_d[b]: raw CRC of byte b followed by d zero bytes
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t c = t0[b];
        for (uint32_t d = 0; d < 57; d++) {
            T->hdr[d][b] = c;
            if (d < 4) T->slice[d][b] = c;
            c = raw_step_zero(c, t0);
        }
    }
    // braid tables: byte b followed by 1023 - t zero bytes
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t c = t0[b];
        for (uint32_t z = 0; z < kBraidSkip; z++) c = raw_step_zero(c, t0);
        for (int t = 3; t >= 0; t--) {
            T->braid[t][b] = c;  // t = 3: 1020 zeros ... t = 0: 1023 zeros
            c = raw_step_zero(c, t0);
        }
    }
    // shift tables: state byte j (value b << 8j) advanced over 16 << m zero bytes
    for (uint32_t m = 0; m < kShiftLevels; m++) {
        const uint64_t n = 16ull << m;
        for (uint32_t j = 0; j < 4; j++) {
            for (uint32_t b = 0; b < 256; b++) {
                uint32_t c = b << (8 * j);
                for (uint64_t z = 0; z < n; z++) c = raw_step_zero(c, t0);
                T->shift[m][j][b] = c;
            }
        }
    }
    uint32_t c = 0xFFFFFFFFu;
    for (int z = 0; z < 40; z++) c = raw_step_zero(c, t0);
    T->c40 = c;
    for (int z = 40; z < 57; z++) c = raw_step_zero(c, t0);
    T->c57 = c;
    T->pad[0] = T->pad[1] = 0;
    // x^(8 * 16 k) (reflected, bit 31 = x^0): mulx multiplies by x
    auto mulx = [](uint32_t a) { return (a & 1u) ? (a >> 1) ^ kCrcPoly : a >> 1; };
    auto invx = [](uint32_t a) { return (a & 0x80000000u) ? ((a ^ kCrcPoly) << 1) | 1u : a << 1; };
    uint32_t e = 0x80000000u;
    for (uint32_t k = 0; k < 64; k++) {
        T->lane_rowend[63 - k] = e;
        for (int b = 0; b < 128; b++) e = mulx(e);
    }
    e = 0x80000000u;
    for (uint32_t z = 0; z < 1024; z++) {
        T->inv_shift[z] = e;
        for (int b = 0; b < 8; b++) e = invx(e);
    }
}

// the combine tables take ~2^13 * 1024 zero-steps; build them once per process
static const Tables* host_tables() {
    static Tables* T = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        T = new Tables;
        build_tables(T);
    });
    return T;
}

// A grow-only buffer the context owns, in device or pinned host memory:
// grow() (below) is the only place one is allocated or replaced, release()
// the only place one is freed.
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    template <class T>
    T* as() const { return (T*)p; }
    void release() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
    }
};

// a side stream of a job and the events of its fork and join (Fork, below)
struct Side {
    hipStream_t stream = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
};

}  // namespace rp

using namespace rp;

struct rpgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    Tables* d_tables = nullptr;
    Buf ws;  // the submit pipeline's device workspace
    bool timing = false;
    // one event set per timed submit: start, discover done, plan done,
    // decode done, validate done, walk done, end; resolved lazily by
    // rpgpu_last_timings
    std::vector<std::array<hipEvent_t, 7>> ev_sets;
    size_t ev_used = 0;
    uint32_t cu_count = 256;
    Buf uws;                       // rpgpu_uncompress staging (device)
    Buf qws;                       // rpgpu_query_capacity scratch (summaries, totals, batch results)
    Buf bh{nullptr, 0, true}, bd;  // rpgpu_uncompress_batch / rpgpu_compress_batch staging: pinned host and device
    Buf sws;                       // rpgpu_stamp workspace (offset steps, scan temporaries, claim cursor)
    Buf iws;                       // rpgpu_segment_index workspace (piece tables)
    // rpgpu_compact workspace (key table, per-batch plan, scan temporaries);
    // its stage events (rpgpu_set_timing)
    Buf cws;
    hipEvent_t cev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool cev_live = false;
    // rpgpu_append_wire workspace (verdicts, per-batch plan, scan temporaries,
    // the append-time stamp list); its stage events (rpgpu_set_timing)
    Buf aws;
    hipEvent_t aev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool aev_live = false;
    // rpgpu_fetch workspace (per-batch plan, per-partition read state, scan
    // temporaries); its stage events (rpgpu_set_timing)
    Buf fws;
    hipEvent_t fev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool fev_live = false;
    // rpgpu_recompress workspace (per-batch plan, the block array, the block
    // kernels' scratch, scan temporaries, the stamp list); its stage events
    // (rpgpu_set_timing)
    Buf rws;
    hipEvent_t rev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool rev_live = false;
    // k_lz_exec parse records (kRecsPerLane per lane of each resident wave),
    // allocated on the first decode job
    Buf seqs;
    uint32_t exec_waves = 0;
    Buf pool;  // k_lz_walk record pool (slabs) and its chain links
    // k_lzf_walk's 8-byte records (independent-block fast path); without it
    // every piece takes the walk / exec kernels
    Buf fpool;
    std::string err;
    // Context scratch (ws, pool, seqs, sws, iws) is shared by every job on
    // the context, whichever stream it is launched on: each async entry
    // point makes its stream wait for the previous job's last event (a
    // device-side wait, no host sync) and records its own at the end, and a
    // scratch buffer is only freed for growth once that event completed.
    hipEvent_t ws_ev = nullptr;
    bool ws_live = false;
    // rpgpu_validate_host: a copy stream and two staging slots (segment
    // bytes in, per-batch results out), used alternately so the H2D copy of
    // group g + 1 runs while group g validates
    hipStream_t copy = nullptr;
    // the zstd members' first pass (k_zparse) beside k_members_first's gzip
    // members, the listed LZ4 blocks (k_lzf_walk) beside k_lz_walk, the LZ4F
    // content checksums beside k_decode_finish
    Side side;
    // k_raw_copy beside k_lzf_walk and k_lz_walk; the gzip members the split
    // decode does not plan, beside it
    Side side2;
    struct HostSlot {
        // device staging, in elements of the named type
        Buf d_data, d_offs, d_batches, d_records, d_decoded, d_sums, d_tot;
        Buf h_tot{nullptr, 0, true};
        // segment index rebuild (rpgpu_host_job.index_step)
        Buf d_ist, d_ro, d_rt, d_ps;
        hipEvent_t h2d = nullptr, done = nullptr;
        std::vector<uint64_t> h_offs;
        std::vector<rpgpu_index_state> h_ist;
    } hs[2];
    Buf sth{nullptr, 0, true}, std_;  // rpgpu_stamp_host staging (pinned host + device)
    // RPGPU_JOB_HOST_CODECS: the host step's items and staging (device and
    // pinned host); hc_n = items of the job being enqueued
    Buf hc_items, hc_items_h{nullptr, 0, true}, hc_in, hc_in_h{nullptr, 0, true}, hc_out, hc_out_h{nullptr, 0, true},
        hc_small{nullptr, 0, true};
    uint32_t hc_n = 0;
    Buf gz_pool;   // gzip / zstd first-pass output pool (k_members_first)
    Buf gzs_pool;  // the gzip split decode's chunk symbols
    // rpgpu_set_device_gzip: gzip payloads are deflated on the device
    // (k_deflate, k_deflate_blocks); dfw: the list cursor, then the streams'
    // work areas (grow-only, at most kDeflateStreams of df::kWorkBytes); dev:
    // k_deflate's events in rpgpu_compress_batch (rpgpu_set_timing)
    bool device_gzip = false;
    uint64_t gzip_dev_payloads = 0;
    Buf dfw;
    hipEvent_t dev[2] = {nullptr, nullptr};
    bool dev_live = false;
};

namespace {

int fail(rpgpu_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    if (c) {
        c->err = what;
        if (e != hipSuccess) {
            c->err += ": ";
            c->err += hipGetErrorString(e);
        }
    }
    return code;
}

#define HIPCHK(ctx, call)                                                   \
    do {                                                                    \
        hipError_t _e = (call);                                             \
        if (_e != hipSuccess) return fail((ctx), RPGPU_E_HIP, #call, _e);   \
    } while (0)

// ordering of jobs that share the context scratch (see rpgpu_ctx::ws_ev)
int ws_acquire(rpgpu_ctx* c, hipStream_t s) {
    if (c->ws_live) HIPCHK(c, hipStreamWaitEvent(s, c->ws_ev, 0));
    return RPGPU_OK;
}
int ws_release(rpgpu_ctx* c, hipStream_t s) {
    if (!c->ws_ev) HIPCHK(c, hipEventCreateWithFlags(&c->ws_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ws_ev, s));
    c->ws_live = true;
    return RPGPU_OK;
}
// before freeing scratch for growth: the previous job (any stream) is done
int ws_drain(rpgpu_ctx* c, hipStream_t s) {
    if (c->ws_live) HIPCHK(c, hipEventSynchronize(c->ws_ev));
    HIPCHK(c, hipStreamSynchronize(s));
    return RPGPU_OK;
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Grow `b` to at least `want` bytes (never shrinks).  The buffer may still be
// in use by earlier work on the context, on any stream, so that work is
// drained before the old buffer is freed.  On failure `b` is left empty.
int grow(rpgpu_ctx* c, Buf& b, size_t want, hipStream_t s, const char* what) {
    if (want <= b.bytes) return RPGPU_OK;
    if (b.p) {
        if (int rc = ws_drain(c, s)) return rc;
        b.release();
    }
    if ((b.pinned ? hipHostMalloc(&b.p, want, hipHostMallocDefault) : hipMalloc(&b.p, want)) != hipSuccess) {
        b.p = nullptr;
        return fail(c, RPGPU_E_NOMEM, what);
    }
    b.bytes = want;
    return RPGPU_OK;
}

// A pool the job can do without (fpool, gz_pool, gzs_pool): failing to get it
// is not an error, the job takes its fallback path with the same results.
int grow_optional(rpgpu_ctx* c, Buf& b, size_t want, hipStream_t s) {
    const int rc = grow(c, b, want, s, "");
    if (rc != RPGPU_E_NOMEM) return rc;
    (void)hipGetLastError();
    c->err.clear();
    return RPGPU_OK;
}

// The context scratch for the length of one job: the stream waits for the
// previous job on construction and records this job's end on every way out.
// release() is the success path (its status is the job's); after an error
// return the destructor records the event and the job's own error stands.
class ScratchScope {
    rpgpu_ctx* c_;
    hipStream_t s_;
    int rc_;

  public:
    ScratchScope(rpgpu_ctx* c, hipStream_t s) : c_(c), s_(s), rc_(ws_acquire(c, s)) {}
    ScratchScope(const ScratchScope&) = delete;
    int acquired() { return rc_; }  // not RPGPU_OK: nothing is held, return it
    int release() {
        rc_ = -1;
        return ws_release(c_, s_);
    }
    ~ScratchScope() {
        if (rc_ != RPGPU_OK) return;
        const std::string own = c_->err;
        (void)ws_release(c_, s_);
        c_->err = own;
    }
};

// Everything the diagnostic build (librpgpu_diag.so, -DRPGPU_DIAG, loaded
// with RPGPU_VARIANT=diag) can change, read from the environment once, on
// first use.  The product library reads no environment: there diag() is the
// defaults below, a constant.
struct Diag {
    bool debug_sync = false;          // RPGPU_DEBUG_SYNC=1: synchronize after every stage and name the one that failed
    uint64_t split_min = 0;           // RPGPU_SPLIT_MIN_KIB=n: the split-CRC threshold, at least 64 bytes (0: from the job)
    uint32_t pool_slabs = ~0u;        // RPGPU_POOL_SLABS=n: at most n record-pool slabs (k_lz_exec walks what is cut short)
    bool crc_compose = true;          // RPGPU_CRC_COMPOSE=0: k_validate streams every stored payload
    bool dchain = true;               // RPGPU_DCHAIN=0: k_validate_decoded chains the records itself
    bool lzf = true;                  // RPGPU_LZF=0: every LZ4 piece through the walk / exec kernels
    uint64_t frec_cap = ~0ull;        // RPGPU_FREC_CAP=n: at most n fast-path records (listed groups mix with walked ones)
    size_t inf_pool = 0;              // RPGPU_INF_POOL_KIB=n: the gzip / zstd first-pass pool, at least 4 KiB (0: from the job)
    uint32_t zs_fast = 1;             // RPGPU_ZS_FAST=0: every zstd member through the wave decoder
    bool gzs = true;                  // RPGPU_GZS=0: every gzip member serial
    bool xxh_side = true;             // RPGPU_XXH_SIDE=0: the content checksums inside k_decode_finish
    uint32_t lzwalk_wgs = 0;          // RPGPU_LZWALK_WGS=n: k_lz_walk's grid in workgroups (0: 16 per CU)
    uint32_t walk_wgs = 8;            // RPGPU_WALK_WGS=n: k_walk's workgroups per CU
    bool host_codec_missing = false;  // RPGPU_HOST_CODEC_MISSING=1: act as if libzstd could not be loaded
    bool index_serial = false;        // RPGPU_INDEX_SERIAL=1: the one-wave-per-segment index walk
    uint32_t ckey_tag_mask = ~0u;     // RPGPU_CKEY_TAG_BITS=n: n tag bits in the compaction key table
};
#ifdef RPGPU_DIAG
Diag diag_from_env() {
    Diag d;
    auto diag_env = [](const char* name) { return getenv(name); };
    auto is = [&](const char* name, char v) { const char* e = diag_env(name); return e && *e == v; };
    d.debug_sync = is("RPGPU_DEBUG_SYNC", '1');
    if (const char* e = diag_env("RPGPU_SPLIT_MIN_KIB")) d.split_min = std::max<uint64_t>(strtoull(e, nullptr, 10) << 10, 64);
    if (const char* e = diag_env("RPGPU_POOL_SLABS")) d.pool_slabs = (uint32_t)atoi(e);
    d.crc_compose = !is("RPGPU_CRC_COMPOSE", '0');
    d.dchain = !is("RPGPU_DCHAIN", '0');
    d.lzf = !is("RPGPU_LZF", '0');
    if (const char* e = diag_env("RPGPU_FREC_CAP")) d.frec_cap = strtoull(e, nullptr, 10);
    if (const char* e = diag_env("RPGPU_INF_POOL_KIB")) d.inf_pool = std::max<size_t>(strtoull(e, nullptr, 10) << 10, 4096);
    d.zs_fast = is("RPGPU_ZS_FAST", '0') ? 0u : 1u;
    if (is("RPGPU_GZS", '0')) d.gzs = false;
    d.xxh_side = !is("RPGPU_XXH_SIDE", '0');
    if (const char* e = diag_env("RPGPU_LZWALK_WGS")) d.lzwalk_wgs = (uint32_t)atoi(e);
    if (const char* e = diag_env("RPGPU_WALK_WGS")) d.walk_wgs = (uint32_t)atoi(e);
    d.host_codec_missing = is("RPGPU_HOST_CODEC_MISSING", '1');
    d.index_serial = is("RPGPU_INDEX_SERIAL", '1');
    if (const char* e = diag_env("RPGPU_CKEY_TAG_BITS")) {
        // probes start at the tag, so that different keys meet on one tag
        const int bits = atoi(e);
        if (bits >= 0 && bits < 32) d.ckey_tag_mask = (1u << bits) - 1u;
    }
    return d;
}
const Diag& diag() {
    static const Diag d = diag_from_env();
    return d;
}
#else
constexpr Diag kNoDiag{};
constexpr const Diag& diag() { return kNoDiag; }
#endif

// A side stream is created at the device's highest stream priority.  HIP
// spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues (4 here)
// round robin, and a side stream that lands on the caller's queue runs after
// it instead of beside it (C6's member pass measured 64 ms alone, 77 ms after
// the bench's H2D stanza had created its copy streams); a priority of its own
// gives it a queue of its own.  (The default priority was measured on the
// raw-copy stream and lost: DESIGN.md §5.)
hipError_t side_stream_create(hipStream_t* out) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
        return hipStreamCreateWithPriority(out, hipStreamNonBlocking, greatest);
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

// One fork of a job's stream `s` onto a side stream of the context: open()
// makes the side stream (created on first use, with its two events) wait for
// what `s` holds now, join() makes `s` wait for what the side stream holds
// then (or held at end(), where the caller marked the side stream's part
// complete as soon as it was enqueued).  The destructor joins if join() was
// not reached, so that an error return still orders `s`, where the scratch is
// released, after the side stream's kernels.
class Fork {
    hipStream_t s_ = nullptr;
    Side* side_ = nullptr;
    bool ended_ = false;

  public:
    Fork() = default;
    Fork(const Fork&) = delete;
    ~Fork() { (void)join(); }
    // at: an open fork of the same stream with nothing enqueued on `s` since;
    // this one then forks at the same point (it waits for that fork's event)
    hipError_t open(hipStream_t s, Side& sd, const Fork* at = nullptr) {
        hipError_t e = sd.stream ? hipSuccess : side_stream_create(&sd.stream);
        if (e == hipSuccess && !sd.fork_ev) e = hipEventCreateWithFlags(&sd.fork_ev, hipEventDisableTiming);
        if (e == hipSuccess && !sd.join_ev) e = hipEventCreateWithFlags(&sd.join_ev, hipEventDisableTiming);
        if (e == hipSuccess && !at) e = hipEventRecord(sd.fork_ev, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(sd.stream, at ? at->side_->fork_ev : sd.fork_ev, 0);
        if (e == hipSuccess) {
            s_ = s;
            side_ = &sd;
        }
        return e;
    }
    // the side stream's part is enqueued: its end is recorded now, join() waits for it
    hipError_t end() {
        const hipError_t e = hipEventRecord(side_->join_ev, side_->stream);
        ended_ = e == hipSuccess;
        return e;
    }
    hipError_t join() {  // nothing to do when the fork was never opened
        if (!side_) return hipSuccess;
        Side* sd = side_;
        side_ = nullptr;
        const hipError_t e = ended_ ? hipSuccess : hipEventRecord(sd->join_ev, sd->stream);
        return e == hipSuccess ? hipStreamWaitEvent(s_, sd->join_ev, 0) : e;
    }
};

// gzip / zstd: the CPU fallback behind compressor::uncompress (rp_hostcodec.cpp)
int host_codec(rpgpu_ctx* c, int codec, const void* in, size_t n, void* out, size_t cap, size_t* out_len) {
    const int rc = host_uncompress(codec, (const uint8_t*)in, n, (uint8_t*)out, cap, out_len);
    if (rc == 0) return RPGPU_OK;
    if (rc == kHostCodecOverflow) return fail(c, RPGPU_E_OVERFLOW, "rpgpu_uncompress: output capacity too small");
    if (rc == kHostCodecMissing) return fail(c, RPGPU_E_UNSUPPORTED, "rpgpu_uncompress: zlib / libzstd not loadable");
    *out_len = 0;
    return fail(c, RPGPU_E_CODEC, codec == RPGPU_CODEC_GZIP ? "gzip uncompress error" : "ZSTD error");
}

}  // namespace

extern "C" {

int rpgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rpgpu_create(int device, rpgpu_ctx** out) {
    if (!out) return RPGPU_E_INVALID;
    *out = nullptr;
    int n = rpgpu_device_count();
    if (n <= 0 || device < 0 || device >= n) return RPGPU_E_NO_DEVICE;
    rpgpu_ctx* c = new rpgpu_ctx;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return RPGPU_E_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->cu_count = (uint32_t)prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return RPGPU_E_HIP; }
    if (hipMalloc(&c->d_tables, sizeof(Tables)) != hipSuccess) { delete c; return RPGPU_E_NOMEM; }
    if (hipMemcpy(c->d_tables, host_tables(), sizeof(Tables), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(c->d_tables);
        delete c;
        return RPGPU_E_HIP;
    }
    *out = c;
    return RPGPU_OK;
}

int rpgpu_destroy(rpgpu_ctx* c) {
    if (!c) return RPGPU_E_INVALID;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->ws_live) (void)hipEventSynchronize(c->ws_ev);
    for (Side* sd : {&c->side, &c->side2}) {
        if (sd->stream) { (void)hipStreamSynchronize(sd->stream); (void)hipStreamDestroy(sd->stream); }
        if (sd->fork_ev) (void)hipEventDestroy(sd->fork_ev);
        if (sd->join_ev) (void)hipEventDestroy(sd->join_ev);
    }
    if (c->copy) { (void)hipStreamSynchronize(c->copy); (void)hipStreamDestroy(c->copy); }
    for (Buf* b : {&c->ws, &c->uws, &c->qws, &c->bh, &c->bd, &c->sws, &c->iws, &c->cws, &c->aws, &c->fws, &c->rws, &c->dfw, &c->seqs, &c->pool, &c->fpool,
                   &c->sth, &c->std_, &c->hc_items, &c->hc_items_h, &c->hc_in, &c->hc_in_h, &c->hc_out, &c->hc_out_h,
                   &c->hc_small, &c->gz_pool, &c->gzs_pool})
        b->release();
    for (auto& h : c->hs) {
        for (Buf* b : {&h.d_data, &h.d_offs, &h.d_batches, &h.d_records, &h.d_decoded, &h.d_sums, &h.d_tot, &h.h_tot,
                       &h.d_ist, &h.d_ro, &h.d_rt, &h.d_ps})
            b->release();
        if (h.h2d) hipEventDestroy(h.h2d);
        if (h.done) hipEventDestroy(h.done);
    }
    if (c->d_tables) hipFree(c->d_tables);
    for (hipEvent_t e : c->cev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->aev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->fev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->rev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->dev)
        if (e) hipEventDestroy(e);
    if (c->ws_ev) (void)hipEventDestroy(c->ws_ev);
    for (auto& set : c->ev_sets)
        for (auto& e : set) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return RPGPU_OK;
}

const char* rpgpu_strerror(int s) {
    switch (s) {
    case RPGPU_OK: return "ok";
    case RPGPU_E_INVALID: return "invalid argument";
    case RPGPU_E_NO_DEVICE: return "no HIP device";
    case RPGPU_E_NOMEM: return "out of memory";
    case RPGPU_E_OVERFLOW: return "output capacity too small";
    case RPGPU_E_CODEC: return "uncompress failed";
    case RPGPU_E_UNSUPPORTED: return "codec not supported by the engine";
    case RPGPU_E_HIP: return "HIP runtime error";
    }
    return "unknown";
}

const char* rpgpu_last_error(rpgpu_ctx* c) { return c ? c->err.c_str() : ""; }

int rpgpu_dev_alloc(rpgpu_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return RPGPU_E_INVALID;
    hipSetDevice(c->device);
    if (hipMalloc(out, bytes ? bytes : 1) != hipSuccess) return fail(c, RPGPU_E_NOMEM, "hipMalloc");
    return RPGPU_OK;
}
int rpgpu_dev_free(rpgpu_ctx* c, void* p) {
    if (!c) return RPGPU_E_INVALID;
    hipSetDevice(c->device);
    HIPCHK(c, hipFree(p));
    return RPGPU_OK;
}
int rpgpu_host_alloc(rpgpu_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return RPGPU_E_INVALID;
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return fail(c, RPGPU_E_NOMEM, "hipHostMalloc");
    return RPGPU_OK;
}
int rpgpu_host_free(rpgpu_ctx* c, void* p) {
    if (!c) return RPGPU_E_INVALID;
    HIPCHK(c, hipHostFree(p));
    return RPGPU_OK;
}
static hipStream_t pick(rpgpu_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }
int rpgpu_memcpy_h2d(rpgpu_ctx* c, void* dst, const void* src, size_t n, void* s) {
    if (!c) return RPGPU_E_INVALID;
    HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, pick(c, s)));
    return RPGPU_OK;
}
int rpgpu_memcpy_d2h(rpgpu_ctx* c, void* dst, const void* src, size_t n, void* s) {
    if (!c) return RPGPU_E_INVALID;
    HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, pick(c, s)));
    return RPGPU_OK;
}
int rpgpu_memset(rpgpu_ctx* c, void* dst, int v, size_t n, void* s) {
    if (!c) return RPGPU_E_INVALID;
    HIPCHK(c, hipMemsetAsync(dst, v, n, pick(c, s)));
    return RPGPU_OK;
}
int rpgpu_sync(rpgpu_ctx* c, void* s) {
    if (!c) return RPGPU_E_INVALID;
    HIPCHK(c, hipStreamSynchronize(pick(c, s)));
    return RPGPU_OK;
}

int rpgpu_set_timing(rpgpu_ctx* c, int enable) {
    if (!c) return RPGPU_E_INVALID;
    c->timing = enable != 0;
    return RPGPU_OK;
}

int rpgpu_set_device_gzip(rpgpu_ctx* c, int enable) {
    if (!c) return RPGPU_E_INVALID;
    c->device_gzip = enable != 0;
    return RPGPU_OK;
}

int rpgpu_gzip_device_ms(rpgpu_ctx* c, float* ms) {
    if (!c || !ms) return RPGPU_E_INVALID;
    if (!c->dev_live) return fail(c, RPGPU_E_INVALID, "rpgpu_gzip_device_ms: no timed device gzip in rpgpu_compress_batch");
    HIPCHK(c, hipEventSynchronize(c->dev[1]));
    HIPCHK(c, hipEventElapsedTime(ms, c->dev[0], c->dev[1]));
    return RPGPU_OK;
}

int rpgpu_gzip_device_payloads(rpgpu_ctx* c, uint64_t* n) {
    if (!c || !n) return RPGPU_E_INVALID;
    *n = c->gzip_dev_payloads;
    return RPGPU_OK;
}

// Averages over every timed submit since the previous call (then resets).
// ms[0] whole pipeline, [1] discover, [2] resolve+emit+plan, [3] validate,
// [4] decode, [5] lane record walk.
int rpgpu_last_timings(rpgpu_ctx* c, float* ms, int n) {
    if (!c || !ms) return RPGPU_E_INVALID;
    if (c->ev_used == 0) return fail(c, RPGPU_E_INVALID, "rpgpu_last_timings: no timed submit");
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < c->ev_used; i++) {
        auto& e = c->ev_sets[i];
        HIPCHK(c, hipEventSynchronize(e[6]));
        const int pairs[6][2] = {{0, 6}, {0, 1}, {1, 2}, {3, 4}, {2, 3}, {4, 5}};
        for (int k = 0; k < 6; k++) {
            float t = 0;
            HIPCHK(c, hipEventElapsedTime(&t, e[pairs[k][0]], e[pairs[k][1]]));
            acc[k] += t;
        }
    }
    for (int i = 0; i < n && i < 6; i++) ms[i] = (float)(acc[i] / (double)c->ev_used);
    c->ev_used = 0;
    return RPGPU_OK;
}

// ---------------------------------------------------------------------------
// submit
// ---------------------------------------------------------------------------
}  // extern "C"

namespace {
// device addresses of the plan a stopped submit leaves in the workspace
struct PlanPtrs {
    const uint64_t* n_batches;  // chunk_count[total_chunks]
    const uint64_t* slots;      // exclusive scan of index slots (batch_capacity + 1)
    const uint64_t* dcap;       // exclusive scan of decode bytes (batch_capacity + 1)
};
enum SubmitStop { kRunAll = 0, kStopAfterCount = 1, kStopAfterPlan = 2 };
int submit_impl(rpgpu_ctx* c, const rpgpu_job* job, void* stream, int stop, PlanPtrs* plan);
}  // namespace

extern "C" {

int rpgpu_submit(rpgpu_ctx* c, const rpgpu_job* job, void* stream) { return submit_impl(c, job, stream, kRunAll, nullptr); }

}  // extern "C"

namespace {
int submit_body(rpgpu_ctx* c, const rpgpu_job* job, hipStream_t s, int stop, PlanPtrs* plan);

// every job on a context is ordered after the previous one (rpgpu_ctx::ws_ev)
int submit_impl(rpgpu_ctx* c, const rpgpu_job* job, void* stream, int stop, PlanPtrs* plan) {
    if (!c) return RPGPU_E_INVALID;
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    if (int rc = submit_body(c, job, s, stop, plan)) return rc;
    return scratch.release();
}

// host-codec staging: 25 % slack over the job's bytes, whole pages
int grow_staging(rpgpu_ctx* c, Buf& b, size_t want, hipStream_t s) {
    if (want <= b.bytes) return RPGPU_OK;
    return grow(c, b, std::max<size_t>(align_up(want + want / 4, 4096), 4096), s, "host codec staging");
}

// RPGPU_JOB_HOST_CODECS: the batches k_emit put on the host list (zstd) cross
// to the host, are decoded by stream_zstd::do_uncompress's loop over libzstd
// (rp_hostcodec.cpp; compression/stream_zstd.cc:152-178) on a few threads,
// and come back: their arena reservations and index slots are patched in
// before the scans (the same rule as every codec: the decoded size rounded up
// to 16, 0 when the reference throws), the bytes wait in device staging for
// k_host_scatter.  Synchronizes the stream three times.
int host_codec_step(rpgpu_ctx* c, const DeviceJob& j, hipStream_t s) {
    if (int rc = grow_staging(c, c->hc_small, 64, s)) return rc;
    uint32_t* cnt = (uint32_t*)c->hc_small.p;
    HIPCHK(c, hipMemcpyAsync(cnt, j.counters + kCtrHostCount, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint32_t n = *cnt;
    if (n == 0) return RPGPU_OK;
    const size_t ib = (size_t)n * sizeof(HostItem);
    if (int rc = grow_staging(c, c->hc_items, ib, s)) return rc;
    if (int rc = grow_staging(c, c->hc_items_h, ib, s)) return rc;
    HostItem* dit = (HostItem*)c->hc_items.p;
    HostItem* hit = (HostItem*)c->hc_items_h.p;
    HIPCHK(c, launch_host_desc(j, dit, n, s));
    HIPCHK(c, hipMemcpyAsync(hit, dit, ib, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    uint64_t in_total = 0;
    for (uint32_t i = 0; i < n; i++) {
        hit[i].stage = in_total;
        in_total += align_up(hit[i].n, 16);
    }
    if (int rc = grow_staging(c, c->hc_in, in_total + 16, s)) return rc;
    if (int rc = grow_staging(c, c->hc_in_h, in_total + 16, s)) return rc;
    HIPCHK(c, hipMemcpyAsync(dit, hit, ib, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_host_gather(j, dit, n, (uint8_t*)c->hc_in.p, s));
    HIPCHK(c, hipMemcpyAsync(c->hc_in_h.p, c->hc_in.p, in_total, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // decode: compressor::uncompress throws on an empty payload
    // (compression/compression.cc:34-55), then the reference loop
    std::vector<std::vector<uint8_t>> outs(n);
    const uint8_t* in = (const uint8_t*)c->hc_in_h.p;
    std::atomic<uint32_t> next{0};
    std::atomic<bool> missing{false};
    const bool force_missing = diag().host_codec_missing;  // diagnostic build: tests the unsupported path
    auto work = [&]() {
        for (uint32_t i; (i = next.fetch_add(1)) < n;) {
            HostItem& it = hit[i];
            it.status = -1;
            it.out_len = 0;
            if (it.n == 0) continue;
            std::vector<uint8_t>& o = outs[i];
            o.resize((size_t)it.n * 4 + 4096);
            size_t len = 0;
            int rc = force_missing ? kHostCodecMissing
                                   : host_uncompress(kHostZstd, in + it.stage, it.n, o.data(), o.size(), &len);
            if (rc == kHostCodecOverflow) {
                o.resize(len);
                rc = host_uncompress(kHostZstd, in + it.stage, it.n, o.data(), o.size(), &len);
            }
            if (rc == kHostCodecMissing) missing = true;
            if (rc == 0) {
                it.status = 0;
                it.out_len = len;
            }
        }
    };
    const uint32_t nt = std::min<uint32_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), n);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    // a payload libzstd never saw is not corrupt: the job is unsupported here
    // (rpgpu_uncompress answers RPGPU_E_UNSUPPORTED the same way)
    if (missing) return fail(c, RPGPU_E_UNSUPPORTED, "RPGPU_JOB_HOST_CODECS: libzstd not loadable");
    uint64_t out_total = 0;
    for (uint32_t i = 0; i < n; i++) {
        HostItem& it = hit[i];
        it.cap = it.status == 0 ? align_up(it.out_len, 16) : 0;
        it.stage = out_total;
        out_total += it.cap;
    }
    if (int rc = grow_staging(c, c->hc_out, out_total + 16, s)) return rc;
    if (int rc = grow_staging(c, c->hc_out_h, out_total + 16, s)) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (hit[i].status == 0) memcpy((uint8_t*)c->hc_out_h.p + hit[i].stage, outs[i].data(), hit[i].out_len);
    HIPCHK(c, hipMemcpyAsync(c->hc_out.p, c->hc_out_h.p, out_total, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dit, hit, ib, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_host_patch(j, dit, n, s));
    // the pinned copies are read by the copies just queued: done before this
    // context's next host step rewrites them (it syncs the stream first)
    c->hc_n = n;
    return RPGPU_OK;
}

int check_job(rpgpu_ctx* c, const rpgpu_job* job) {
    if (!c || !job || !job->d_data || !job->d_seg_offsets || !job->h_seg_offsets || job->n_segments == 0 ||
        !job->d_batches || !job->d_summaries || !job->d_totals)
        return fail(c, RPGPU_E_INVALID, "rpgpu_submit: missing argument");
    if (((uintptr_t)job->d_data & 15) != 0) return fail(c, RPGPU_E_INVALID, "rpgpu_submit: d_data must be 16-byte aligned");
    if (job->layout != RPGPU_LAYOUT_DISK && job->layout != RPGPU_LAYOUT_WIRE)
        return fail(c, RPGPU_E_INVALID, "rpgpu_submit: unknown layout");
    if ((job->flags & RPGPU_JOB_PARSE) && !job->d_records && job->record_capacity)
        return fail(c, RPGPU_E_INVALID, "rpgpu_submit: PARSE needs d_records");
    return RPGPU_OK;
}

// Where each table of a job lies in the workspace (byte offsets, 256-byte
// aligned), the capacities they were sized for and the bytes needed in all.
struct Layout {
    uint64_t tc;  // chunks of the job (every segment at least one)
    uint64_t zcap, gcap, bl_cap, split_min, split_cap;
    size_t cbase, chunks, ccount, centry, segterm, slots, dcap, counters, dlist, slist, llist, fbad;
    size_t ilist, istate, ioff, itot, hlist, zitems, gzsmem, gzsit;
    size_t blocks, plans, pstate, longl, wlong, rawl, lanel, lzfl, lzft, split, spart, scan;
    size_t wdesc, wverd;
    size_t need;
};

Layout job_layout(const rpgpu_job* job, uint32_t cu_count) {
    Layout L;
    const uint32_t nseg = job->n_segments;
    const uint32_t cs = job->chunk_bytes ? job->chunk_bytes : (256u << 10);
    const uint64_t bcap = job->batch_capacity, data_len = job->h_seg_offsets[nseg];
    // chunk table from the host offsets
    uint64_t tc = 0;
    for (uint32_t i = 0; i < nseg; i++) {
        const uint64_t len = job->h_seg_offsets[i + 1] - job->h_seg_offsets[i];
        uint64_t nc = (len + cs - 1) / cs;
        tc += nc ? nc : 1;
    }
    L.tc = tc;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    L.cbase = take((nseg + 1) * 8);
    L.chunks = take(tc * sizeof(ChunkRec));
    L.ccount = take((tc + 1) * 8);
    L.centry = take(tc * 8);
    L.segterm = take(nseg * sizeof(SegTerm));
    L.slots = take((bcap + 1) * 8);
    L.dcap = take((bcap + 1) * 8);
    L.counters = take(kCounterBytes);
    L.dlist = take((bcap + 1) * 4);
    L.slist = take((bcap + 1) * 4);
    L.llist = take((bcap + 1) * 4);
    L.fbad = take((size_t)nseg * 4);
    const bool decode_job = (job->flags & RPGPU_JOB_DECODE) != 0;
    L.ilist = take(decode_job ? (bcap + 1) * 4 : 0);
    L.istate = take(decode_job ? (bcap + 1) * 4 : 0);
    L.ioff = take(decode_job ? (bcap + 1) * 8 : 0);
    L.itot = take(decode_job ? (bcap + 1) * 8 : 0);
    const bool host_job = decode_job && (job->flags & RPGPU_JOB_HOST_CODECS);
    L.hlist = take(host_job ? (bcap + 1) * 4 : 0);
    // zstd literal blocks planned ahead (k_zplan -> k_zlits): a 128 KiB block
    // each at most, so the job's bytes / 16 KiB + 8 per batch is ample (past
    // it, blocks decode in place)
    L.zcap = decode_job ? std::min<uint64_t>(data_len / 16384 + 8 * bcap + 64, 0x7FFFFFFFull) : 0;
    L.zitems = take(L.zcap * 8);
    // gzip split decode: per member its first item and chunk count; items:
    // one per kGzsChunk deflate bytes of the split members, one more each
    L.gzsmem = take(decode_job ? 2 * (bcap + 1) * 4 : 0);
    L.gcap = decode_job ? std::min<uint64_t>(data_len / kGzsChunk + bcap + 64, 0x7FFFFFFFull) : 0;
    L.gzsit = take(L.gcap * sizeof(GzsItem));
    // block-parallel decode: one item per LZ4F block / snappy-java chunk
    const bool dec = decode_job && job->d_decoded;
    L.bl_cap = dec ? std::min<uint64_t>(data_len / 16384 + 2 * bcap + 64, 0x7FFFFFFFull) : 0;
    L.blocks = take(L.bl_cap * sizeof(BlockItem));
    L.plans = take(dec ? (bcap + 1) * sizeof(FramePlan) : 0);
    L.pstate = take(L.bl_cap * sizeof(PieceState));
    L.longl = take(L.bl_cap * 4);
    L.wlong = take(L.bl_cap * 4);
    L.rawl = take(L.bl_cap * 4);
    L.lanel = take(L.bl_cap * 4);
    L.lzfl = take(L.bl_cap * 4);
    L.lzft = take(L.bl_cap * 4);
    // the diagnostic override: scripts/bench_skew.py A/B
    L.split_min = diag().split_min ? diag().split_min
                                   : std::max<uint64_t>(kSplitMin, 2 * data_len / ((uint64_t)cu_count * kVWaves));
    L.split_cap = std::min<uint64_t>(data_len / L.split_min + 1, bcap + 1);
    L.split = take(L.split_cap * 4);
    L.spart = take(L.split_cap * kSplitParts * 4);
    L.scan = take(scan_temp_bytes(std::max<uint64_t>(tc, bcap)) + 64);
    // k_emit -> k_walk descriptors and k_walk -> k_finalize_bitmap verdicts
    const bool parse_job = (job->flags & RPGPU_JOB_PARSE) != 0;
    L.wdesc = take(parse_job ? (bcap + 1) * sizeof(WalkDesc) : 0);
    L.wverd = take(parse_job ? (bcap + 1) * 8 : 0);
    L.need = off;
    return L;
}

// Grows the context's workspace and pools to the job's size and points the
// DeviceJob at them.  The pools a job can do without (grow_optional) leave
// their pointers null when they cannot be had.
int bind_job(rpgpu_ctx* c, const rpgpu_job* job, const Layout& L, hipStream_t s, int stop, DeviceJob& j) {
    const uint32_t nseg = job->n_segments;
    const uint64_t data_len = job->h_seg_offsets[nseg];
    const bool dec = (job->flags & RPGPU_JOB_DECODE) && job->d_decoded;
    if (dec && !c->seqs.p) {
        const uint32_t waves = c->cu_count * lz_exec_wgs_per_cu();
        if (int rc = grow(c, c->seqs, (size_t)waves * kRecsPerLane * sizeof(SeqRec), s, "decode sequence workspace")) return rc;
        c->exec_waves = waves;
    }
    // record pool: a compressed LZ4 byte yields at most 1/3 record (16 B),
    // typical data far fewer (C2: 0.33 B of records per stored byte); sized
    // from the job's bytes, clamped; pieces that do not fit are walked by
    // k_lz_exec itself
    const size_t slab_bytes = kSlabRecs * sizeof(SeqRec) + 4;
    const size_t pool_want = dec ? std::min<size_t>(std::max<size_t>(data_len / 2, 256ull << 20), 8ull << 30) : 0;
    if (int rc = grow(c, c->pool, pool_want, s, "decode record pool")) return rc;
    if (int rc = grow(c, c->ws, L.need, s, "workspace")) return rc;
    uint8_t* ws = c->ws.as<uint8_t>();

    j.data = job->d_data;
    j.data_len = data_len;
    j.seg_off = job->d_seg_offsets;
    j.chunk_base = (const uint64_t*)(ws + L.cbase);
    j.n_segments = nseg;
    j.flags = job->flags;
    j.layout = job->layout;
    j.chunk_bytes = job->chunk_bytes ? job->chunk_bytes : (256u << 10);
    j.total_chunks = (uint32_t)L.tc;
    j.chunks = (ChunkRec*)(ws + L.chunks);
    j.chunk_count = (uint64_t*)(ws + L.ccount);
    j.chunk_entry = (uint64_t*)(ws + L.centry);
    j.seg_term = (SegTerm*)(ws + L.segterm);
    j.batches = job->d_batches;
    j.batch_capacity = job->batch_capacity;
    j.slots = (uint64_t*)(ws + L.slots);
    j.dcap = (uint64_t*)(ws + L.dcap);
    j.records = job->d_records;
    j.record_capacity = job->d_records ? job->record_capacity : 0;
    j.decoded = job->d_decoded;
    j.decoded_capacity = job->d_decoded ? job->decoded_capacity : 0;
    j.summaries = job->d_summaries;
    j.totals = job->d_totals;
    j.bitmap = job->d_valid_bitmap;
    j.tables = c->d_tables;
    j.counters = (uint32_t*)(ws + L.counters);
    j.decode_list = (uint32_t*)(ws + L.dlist);
    j.seq_list = (uint32_t*)(ws + L.slist);
    j.link_list = (uint32_t*)(ws + L.llist);
    j.long_list = (uint32_t*)(ws + L.longl);
    j.wlong_list = (uint32_t*)(ws + L.wlong);
    j.raw_list = (dec && stop == kRunAll) ? (uint32_t*)(ws + L.rawl) : nullptr;
    j.lane_list = (uint32_t*)(ws + L.lanel);
    j.split_list = (uint32_t*)(ws + L.split);
    j.split_part = (uint32_t*)(ws + L.spart);
    j.split_capacity = (uint32_t)L.split_cap;
    j.split_min = L.split_min;
    j.seqs = c->seqs.as<SeqRec>();
    j.exec_waves = c->exec_waves;
    j.pstate = (PieceState*)(ws + L.pstate);
    // the diagnostic cap shrinks the record pool (exercises k_lz_exec's own
    // walk of the pieces the pool cuts short)
    j.pool_slabs = std::min((uint32_t)std::min<size_t>(c->pool.bytes / slab_bytes, 0xFFFFFFF0ull), diag().pool_slabs);
    j.pool = c->pool.as<SeqRec>();
    j.crc_compose = diag().crc_compose ? 1u : 0u;
    // the decoded payloads' record chains (k_dchain) reuse the record pool,
    // idle once decode is done: one u32 per index slot
    j.dchain = (dec && diag().dchain && c->pool.p && (uint64_t)c->pool.bytes / 4 >= j.record_capacity) ? c->pool.as<uint32_t>()
                                                                                                      : nullptr;
    j.slab_next = (uint32_t*)(c->pool.as<uint8_t>() + (size_t)j.pool_slabs * kSlabRecs * sizeof(SeqRec));
    // fast-path records: the planner reserves csize / 3 + 2 per listed LZ4
    // block (2.7 bytes per compressed byte; C2 uses 0.3 of the job's bytes),
    // 3x the job's bytes (a job of nothing but LZ4 blocks fits whole), 64 MiB
    // .. 16 GiB; a group of blocks that finds no room (and every group after
    // it) takes the walk / exec kernels, with the same results.  The
    // diagnostic record cap mixes listed groups with walked ones in small
    // jobs (tests/test_gpu_diag.py)
    j.frecs = nullptr;
    j.frec_cap = 0;
    j.lzf_list = nullptr;
    j.lzf_tail = nullptr;
    if (dec && diag().lzf && stop == kRunAll) {
        const size_t want = std::min<size_t>(std::max<size_t>(data_len * 3, 64ull << 20), 16ull << 30);
        if (int rc = grow_optional(c, c->fpool, want, s)) return rc;
        if (c->fpool.p) {
            j.frecs = c->fpool.as<uint2>();
            j.frec_cap = std::min<uint64_t>(c->fpool.bytes / sizeof(uint2), diag().frec_cap);
            j.lzf_list = (uint32_t*)(ws + L.lzfl);
            j.lzf_tail = (uint32_t*)(ws + L.lzft);
        }
    }
    j.seg_first_bad = (uint32_t*)(ws + L.fbad);
    j.seeds = (job->d_seeds && job->d_seed_offsets) ? job->d_seeds : nullptr;
    j.seed_off = j.seeds ? job->d_seed_offsets : nullptr;
    j.inf_list = (uint32_t*)(ws + L.ilist);
    j.inf_state = (uint32_t*)(ws + L.istate);
    j.inf_off = (uint64_t*)(ws + L.ioff);
    j.inf_total = (uint64_t*)(ws + L.itot);
    // gzip first-pass pool: twice the job's bytes, 256 MiB .. 2 GiB (members
    // that do not fit are decoded again, straight into the arena); the
    // diagnostic size exercises members that do not get a scratch slot.
    // Only a job that writes decoded bytes uses it (a planning run only sizes
    // members); failing to get it costs a second pass, never the job.
    j.inf_scratch = nullptr;
    j.inf_scratch_bytes = 0;
    j.inf_scratch_used = (uint64_t*)(j.counters + kCtrInfScratchUsed64);  // zeroed with the counters
    if (dec && stop == kRunAll) {
        const size_t want = diag().inf_pool ? diag().inf_pool
                                            : std::min<size_t>(std::max<size_t>(2 * data_len, 256ull << 20), 2ull << 30);
        if (int rc = grow_optional(c, c->gz_pool, want, s)) return rc;
        if (c->gz_pool.p) {
            j.inf_scratch = c->gz_pool.as<uint8_t>();
            j.inf_scratch_bytes = std::min<size_t>(c->gz_pool.bytes, want);
        }
    }
    j.zs_fast = diag().zs_fast;
    j.zs_split = 0;
    j.zs_items = (uint64_t*)(ws + L.zitems);
    j.zs_items_cap = (uint32_t)L.zcap;
    j.host_list = (uint32_t*)(ws + L.hlist);
    // the gzip split decode (with the scratch pool only: it writes the
    // members' bytes there)
    j.gzs_mem = nullptr;
    j.gzs_items = (GzsItem*)(ws + L.gzsit);
    j.gzs_items_cap = (uint32_t)L.gcap;
    j.gzs_pool = nullptr;
    j.gzs_pool_syms = 0;
    if (j.inf_scratch && diag().gzs && L.gcap) {
        const size_t want = std::min<size_t>(std::max<size_t>(2 * data_len, 64ull << 20), 4ull << 30);
        if (int rc = grow_optional(c, c->gzs_pool, want, s)) return rc;
        if (c->gzs_pool.p) {
            j.gzs_mem = (uint32_t*)(ws + L.gzsmem);
            j.gzs_pool = c->gzs_pool.as<uint16_t>();
            j.gzs_pool_syms = c->gzs_pool.bytes / 2;
        }
    }
    c->hc_n = 0;
    j.blocks = (BlockItem*)(ws + L.blocks);
    j.block_capacity = (uint32_t)L.bl_cap;
    j.plans = (FramePlan*)(ws + L.plans);
    j.walk_desc = (WalkDesc*)(ws + L.wdesc);
    j.walk_verdict = (uint64_t*)(ws + L.wverd);
    if (((uintptr_t)job->d_decoded & 15) != 0) return fail(c, RPGPU_E_INVALID, "rpgpu_submit: d_decoded must be 16-byte aligned");
    return RPGPU_OK;
}

// One launch (or scan) of the pipeline; with RPGPU_DEBUG_SYNC=1 (diagnostic
// build) every stage is synchronized and the one that failed is named (fault
// localisation).  Expects `c` and `s` in scope.
#define STAGE(name, call)                                                                  \
    do {                                                                                   \
        HIPCHK(c, (call));                                                                 \
        if (diag().debug_sync) {                                                           \
            fprintf(stderr, "[rpgpu] stage %s\n", name);                                   \
            fflush(stderr);                                                                \
            hipError_t _e = hipStreamSynchronize(s);                                       \
            if (_e == hipSuccess && c->side.stream) _e = hipStreamSynchronize(c->side.stream);   \
            if (_e == hipSuccess && c->side2.stream) _e = hipStreamSynchronize(c->side2.stream); \
            if (_e != hipSuccess) return fail(c, RPGPU_E_HIP, "stage " name " failed", _e); \
        }                                                                                  \
    } while (0)

// timing event i of a timed submit (ev = nullptr: not timed)
hipError_t mark(hipEvent_t* ev, int i, hipStream_t s) { return ev ? hipEventRecord(ev[i], s) : hipSuccess; }

// discover -> resolve -> the batch count per chunk, scanned; then (emit) the
// batch results' slots.  A counting run (kStopAfterCount) stops before emit.
int stage_discover(rpgpu_ctx* c, const DeviceJob& j, hipStream_t s, hipEvent_t* ev, uint64_t* scan_tmp, bool emit) {
    STAGE("chunk_base", launch_chunk_base(j, s));
    HIPCHK(c, hipMemsetAsync(j.counters, 0, kCounterBytes, s));
    HIPCHK(c, hipMemsetAsync(j.seg_first_bad, 0xFF, (size_t)j.n_segments * 4, s));
    STAGE("discover", launch_discover(j, s));
    HIPCHK(c, mark(ev, 1, s));
    STAGE("resolve", launch_resolve(j, s));
    STAGE("scan_chunks", scan_exclusive_u64(j.chunk_count, j.total_chunks, scan_tmp, 0, s));
    if (emit) STAGE("emit", launch_emit(j, s));
    return RPGPU_OK;
}

// gzip / zstd members: the first pass (their arena bytes, index slots and,
// when they fit the pool, their output), the host-codec step, then the scans
// of the index slots and the arena reservations
int stage_members(rpgpu_ctx* c, DeviceJob& j, hipStream_t s, uint64_t* scan_tmp) {
    const uint32_t cus = c->cu_count;
    if (j.flags & RPGPU_JOB_DECODE) {
        // zstd members on the side stream when the lane parser can run (it
        // needs the scratch pool), gzip members (and, otherwise, zstd ones) here
        const bool split = j.inf_scratch && j.zs_fast;
        STAGE("zstamps", launch_zstamps(s, 0));
        Fork zfork;
        if (split) {
            j.zs_split = 1;
            HIPCHK(c, zfork.open(s, c->side));
            STAGE("zplan", launch_zplan(j, c->side.stream, cus * 4));
            STAGE("zparse", launch_zparse(j, c->side.stream, cus * 4));
            HIPCHK(c, zfork.end());
        }
        // the split decode's members first, then the serial first pass over
        // the rest and over the members the split decode did not close
        if (j.gzs_mem) {
            STAGE("gzsplan", launch_gzsplan(j, s));
            // the members it did not plan (below 16 KiB stored, FHCRC: one
            // wave each) beside the split decode's k_gzsdecode, on the
            // raw-copy stream (idle until the decode stage), the rest after
            // it.  (Forked before k_gzsfind instead, they slowed it 14.3 ->
            // 19.9 ms: C6 resolve+plan 58.9 against 56.7 ms.)
            STAGE("gzsfind", launch_gzsplit(j, s, cus, 1));
            Fork mfork;
            HIPCHK(c, mfork.open(s, c->side2));
            STAGE("inflate_plan", launch_inflate_plan(j, c->side2.stream, cus * 4, 1));
            HIPCHK(c, mfork.end());
            STAGE("gzsplit", launch_gzsplit(j, s, cus, 2));
            STAGE("inflate_plan", launch_inflate_plan(j, s, cus * 4, 2));
            HIPCHK(c, mfork.join());
        } else {
            STAGE("inflate_plan", launch_inflate_plan(j, s, cus * 4));
        }
        if (split) {
            HIPCHK(c, zfork.join());
            STAGE("zfallback", launch_zfallback(j, s, cus * 4));
        }
        // zstd members whose corrupt stream reads ring bytes the current
        // segment has overwritten: decoded again over libzstd's exact buffer
        STAGE("zexact", launch_zexact(j, s, 0));
        STAGE("zstamps", launch_zstamps(s, 1));
        // zstd members (RPGPU_JOB_HOST_CODECS): decoded on the host now, sized
        // before the scans like every other payload
        if (j.flags & RPGPU_JOB_HOST_CODECS)
            if (int rc = host_codec_step(c, j, s)) return rc;
    }
    const uint64_t* d_nb = j.chunk_count + j.total_chunks;
    STAGE("scan_slots", scan_exclusive_u64_devn(j.slots, d_nb, j.batch_capacity, scan_tmp, s));
    // without DECODE every reservation is 0 (k_emit): the scan would write
    // zeros over zeros; k_finalize_totals reads no total then
    if (j.flags & RPGPU_JOB_DECODE) STAGE("scan_dcap", scan_exclusive_u64_devn(j.dcap, d_nb, j.batch_capacity, scan_tmp, s));
    return RPGPU_OK;
}

// decode, before validate: k_validate checksums and walks the decoded
// payloads.  xside: the content checksums on the side stream.
int stage_decode(rpgpu_ctx* c, const DeviceJob& j, hipStream_t s, bool xside) {
    const uint32_t cus = c->cu_count;
    STAGE("decode", launch_decode(j, s, cus * 8));
    STAGE("decode_blocks", launch_decode_blocks(j, s, cus * 8));
    {
        // the listed LZ4 blocks (k_lzf_walk + k_lzf_tail) on the side
        // stream, every other piece (k_lz_walk) here: the planner fixed
        // the two sets (BlockItem.fast), so they run side by side
        const bool lzf = j.lzf_list != nullptr;
        Fork lzf_fork, raw_fork;
        if (lzf) {
            HIPCHK(c, lzf_fork.open(s, c->side));
            STAGE("lzf_walk", launch_lzf_walk(j, c->side.stream, cus));
            HIPCHK(c, lzf_fork.end());
        }
        // the raw copies on a stream of their own, so that neither walk
        // waits for them (C5: the longest raw snappy walk, ~3.7 ms, began
        // after ~0.45 ms of copies); without the side walk, before
        // k_lz_walk on the job's stream
        if (lzf && j.raw_list) {
            HIPCHK(c, raw_fork.open(s, c->side2, &lzf_fork));
            STAGE("raw_copy", launch_raw_copy(j, c->side2.stream, cus));
            HIPCHK(c, raw_fork.end());
        } else {
            STAGE("raw_copy", launch_raw_copy(j, s, cus));
        }
        STAGE("lz_walk", launch_lz_walk(j, s, diag().lzwalk_wgs ? diag().lzwalk_wgs : cus * 16));
        HIPCHK(c, lzf_fork.join());
        HIPCHK(c, raw_fork.join());
    }
    STAGE("lz_exec", launch_lz_exec(j, s));
    // the gzip / zstd members first: k_zexec's workgroups take a CU's
    // registers each and did not fit beside k_content_xxh's waves
    STAGE("inflate", launch_inflate(j, s, cus * 4));
    STAGE("zexec", launch_zexec(j, s));
    STAGE("zexact", launch_zexact(j, s, 1));
    if (c->hc_n) STAGE("host_scatter", launch_host_scatter(j, c->hc_items.as<const HostItem>(), c->hc_n,
                                                           c->hc_out.as<const uint8_t>(), s));
    Fork xfork;
    if (xside) {
        // k_crc_compose (no dependence on the decoded bytes) before the
        // fork, for the same reason.  Then the LZ4F content checksums
        // (serial XXH32 chains, ~1 ms per MiB on one wave each: the rest
        // of the chip idles) on the side stream beside k_decode_finish
        // and the decoded payloads' record chains, which do not depend on
        // them (k_decode_finish gives a checksummed frame its verdict as
        // if it matched; k_content_apply takes it back after the join)
        STAGE("crc_compose", launch_crc_compose(j, s, cus));
        HIPCHK(c, xfork.open(s, c->side));
        STAGE("content_xxh", launch_content_xxh(j, c->side.stream, cus * 2));
    }
    STAGE("decode_finish", launch_decode_finish(j, s, cus * 8, xside));
    if (xside) {
        STAGE("dchain", launch_dchain(j, s, cus));
        HIPCHK(c, xfork.join());
        STAGE("content_apply", launch_content_apply(j, s, cus));
    }
    return RPGPU_OK;
}

// validate -> walk -> finalize.  xside: k_crc_compose and k_dchain already
// ran in the decode stage.
int stage_validate(rpgpu_ctx* c, const DeviceJob& j, hipStream_t s, hipEvent_t* ev, bool xside) {
    const uint32_t cus = c->cu_count;
    STAGE("validate", launch_validate(j, s, cus, !xside));
    // the decoded payloads' record chains, then their walk.  (k_dchain on the
    // side stream beside k_crc_compose / k_validate measured slower than here:
    // C2 validate stage 4.36 against 3.72 ms, the chains' serial loads
    // queueing behind the two streams' HBM traffic)
    if (!xside) STAGE("dchain", launch_dchain(j, s, cus));
    STAGE("validate_decoded", launch_validate_decoded(j, s, cus));
    HIPCHK(c, mark(ev, 4, s));
    STAGE("walk", launch_walk(j, s, cus * diag().walk_wgs));
    HIPCHK(c, mark(ev, 5, s));
    STAGE("finalize", launch_finalize(j, s));
    HIPCHK(c, mark(ev, 6, s));
    return RPGPU_OK;
}
#undef STAGE

int submit_body(rpgpu_ctx* c, const rpgpu_job* job, hipStream_t s, int stop, PlanPtrs* plan) {
    if (int rc = check_job(c, job)) return rc;
    const Layout L = job_layout(job, c->cu_count);
    if (L.tc > 0xFFFFFFF0ull) return fail(c, RPGPU_E_INVALID, "rpgpu_submit: too many chunks");
    DeviceJob j;
    if (int rc = bind_job(c, job, L, s, stop, j)) return rc;
    uint64_t* scan_tmp = (uint64_t*)(c->ws.as<uint8_t>() + L.scan);
    if (plan) {
        plan->n_batches = j.chunk_count + L.tc;
        plan->slots = j.slots;
        plan->dcap = j.dcap;
    }
    // timed submits only: rpgpu_query_capacity's planning runs stop early
    // and record no timings
    hipEvent_t* ev = nullptr;
    if (c->timing && stop == kRunAll) {
        if (c->ev_used == c->ev_sets.size()) {
            std::array<hipEvent_t, 7> set;
            for (auto& e : set) HIPCHK(c, hipEventCreate(&e));
            c->ev_sets.push_back(set);
        }
        ev = c->ev_sets[c->ev_used++].data();
        HIPCHK(c, mark(ev, 0, s));
    }
    if (int rc = stage_discover(c, j, s, ev, scan_tmp, stop != kStopAfterCount)) return rc;
    if (stop == kStopAfterCount) return RPGPU_OK;
    if (int rc = stage_members(c, j, s, scan_tmp)) return rc;
    if (stop == kStopAfterPlan) return RPGPU_OK;
    HIPCHK(c, mark(ev, 2, s));
    const bool dec = (j.flags & RPGPU_JOB_DECODE) && j.decoded;
    const bool xside = dec && diag().xxh_side;
    if (dec)
        if (int rc = stage_decode(c, j, s, xside)) return rc;
    HIPCHK(c, mark(ev, 3, s));
    return stage_validate(c, j, s, ev, xside);
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// output sizing before the run (SURVEY §8(b) segment-engine row: "result
// arrays ... sized by a query call"): the chain is discovered and planned
// (discover -> resolve -> emit -> scans) into context scratch, twice: once to
// count the batches, once with that many result slots to plan the record
// index and the decode arena.  Synchronous.
// ---------------------------------------------------------------------------
int rpgpu_query_capacity(rpgpu_ctx* c, const rpgpu_job* job, void* stream, rpgpu_capacity* out) {
    if (!c || !job || !out) return RPGPU_E_INVALID;
    if (!job->d_data || !job->d_seg_offsets || !job->h_seg_offsets || job->n_segments == 0)
        return fail(c, RPGPU_E_INVALID, "rpgpu_query_capacity: missing argument");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    const uint32_t nseg = job->n_segments;
    const size_t fixed = align_up((size_t)nseg * sizeof(rpgpu_segment_summary), 256) + align_up(sizeof(rpgpu_job_totals), 256);
    int rc = grow(c, c->qws, fixed + 256, s, "rpgpu_query_capacity: scratch");
    if (rc) return rc;
    rpgpu_job q = *job;
    auto point = [&] {
        uint8_t* w = c->qws.as<uint8_t>();
        q.d_summaries = (rpgpu_segment_summary*)w;
        q.d_totals = (rpgpu_job_totals*)(w + align_up((size_t)nseg * sizeof(rpgpu_segment_summary), 256));
        q.d_batches = (rpgpu_batch_result*)(w + fixed);
    };
    point();
    q.batch_capacity = 0;
    q.d_records = nullptr;
    q.record_capacity = 0;
    q.d_decoded = nullptr;
    q.decoded_capacity = 0;
    q.d_valid_bitmap = nullptr;
    PlanPtrs pp;
    rc = submit_impl(c, &q, stream, kStopAfterCount, &pp);
    if (rc) return rc;
    uint64_t nb = 0;
    HIPCHK(c, hipMemcpyAsync(&nb, pp.n_batches, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    rc = grow(c, c->qws, fixed + (size_t)(nb + 1) * sizeof(rpgpu_batch_result), s, "rpgpu_query_capacity: scratch");
    if (rc) return rc;
    point();
    q.batch_capacity = nb;
    rc = submit_impl(c, &q, stream, kStopAfterPlan, &pp);
    if (rc) return rc;
    uint64_t v[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&v[0], pp.slots + nb, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&v[1], pp.dcap + nb, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    out->n_batches = nb;
    out->record_capacity = v[0];
    out->decoded_capacity = (job->flags & RPGPU_JOB_DECODE) ? v[1] : 0;
    out->reserved = 0;
    return RPGPU_OK;
}

// ---------------------------------------------------------------------------
// non-blocking completion (rpgpu_poll / rpgpu_wait on a job):
// rpgpu_submit followed by an event on the launch stream
// ---------------------------------------------------------------------------
struct rpgpu_pending {
    rpgpu_ctx* c;
    hipEvent_t ev;
};

int rpgpu_submit_async(rpgpu_ctx* c, const rpgpu_job* job, void* stream, rpgpu_pending** out) {
    if (!c || !out) return RPGPU_E_INVALID;
    *out = nullptr;
    const int rc = submit_impl(c, job, stream, kRunAll, nullptr);
    if (rc) return rc;
    rpgpu_pending* p = new rpgpu_pending{c, nullptr};
    hipError_t e = hipEventCreateWithFlags(&p->ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(p->ev, pick(c, stream));
    if (e != hipSuccess) {
        if (p->ev) (void)hipEventDestroy(p->ev);
        delete p;
        return fail(c, RPGPU_E_HIP, "rpgpu_submit_async: event", e);
    }
    *out = p;
    return RPGPU_OK;
}

int rpgpu_poll(rpgpu_pending* p) {
    if (!p) return RPGPU_E_INVALID;
    const hipError_t e = hipEventQuery(p->ev);
    if (e == hipSuccess) return RPGPU_OK;
    if (e == hipErrorNotReady) return RPGPU_PENDING;
    return fail(p->c, RPGPU_E_HIP, "rpgpu_poll", e);
}

int rpgpu_wait(rpgpu_pending* p) {
    if (!p) return RPGPU_E_INVALID;
    HIPCHK(p->c, hipEventSynchronize(p->ev));
    return RPGPU_OK;
}

int rpgpu_release(rpgpu_pending* p) {
    if (!p) return RPGPU_E_INVALID;
    (void)hipEventDestroy(p->ev);
    delete p;
    return RPGPU_OK;
}

// ---------------------------------------------------------------------------
// crc::crc32c host path (hashing/crc32c.h:19-40).  SSE4.2 crc32 instructions,
// the same arithmetic google crc32c's x86 path uses.
// ---------------------------------------------------------------------------
__attribute__((target("sse4.2"))) uint32_t rpgpu_crc32c_extend(uint32_t crc, const uint8_t* p, size_t n) {
    uint64_t l = crc ^ 0xFFFFFFFFu;
    while (n && ((uintptr_t)p & 7)) { l = _mm_crc32_u8((uint32_t)l, *p++); n--; }
    while (n >= 8) {
        uint64_t v;
        std::memcpy(&v, p, 8);
        l = _mm_crc32_u64(l, v);
        p += 8;
        n -= 8;
    }
    uint32_t s = (uint32_t)l;
    while (n) { s = _mm_crc32_u8(s, *p++); n--; }
    return s ^ 0xFFFFFFFFu;
}

}  // extern "C"

extern "C" {

// compression::compressor::uncompress (compression/compression.h:21-24) for
// one payload: staged to the device, decoded by one wave (rp_codec.hip).
// The reference throws std::runtime_error on empty input, on `none` and on
// any decode failure -> RPGPU_E_CODEC; gzip/zstd are not decoded here.
// segment_index rebuild over a completed job's results (storage/log_replayer.cc:62-74,
// storage/segment_index.cc:58-72, storage/index_state.cc:48-95); kernel in rp_index.hip
int rpgpu_segment_index(rpgpu_ctx* c, const rpgpu_batch_result* d_batches, uint64_t batch_capacity,
                        const rpgpu_segment_summary* d_summaries, uint32_t n_segments, uint64_t step,
                        rpgpu_index_state* d_states, uint32_t* d_rel_offset, uint32_t* d_rel_time,
                        uint64_t* d_position, void* stream) {
    if (!c) return RPGPU_E_INVALID;
    if (n_segments == 0) return RPGPU_OK;
    if (!d_batches || !d_summaries || !d_states || !d_rel_offset || !d_rel_time || !d_position)
        return fail(c, RPGPU_E_INVALID, "rpgpu_segment_index: missing argument");
    if (step >= (1ull << 62)) return fail(c, RPGPU_E_INVALID, "rpgpu_segment_index: step out of range");
    if (n_segments > 0x7FFFFFFFu) return fail(c, RPGPU_E_INVALID, "rpgpu_segment_index: too many segments");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    if (diag().index_serial) {  // diagnostic build: the A/B reference
        HIPCHK(c, launch_segment_index(d_batches, batch_capacity, d_summaries, n_segments, step, d_states, d_rel_offset,
                                       d_rel_time, d_position, s));
        return RPGPU_OK;
    }
    if (int rc = grow(c, c->iws, segment_index_ws_bytes(n_segments, batch_capacity), s, "rpgpu_segment_index workspace"))
        return rc;
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    HIPCHK(c, launch_segment_index_pieces(d_batches, batch_capacity, d_summaries, n_segments, step, d_states,
                                          d_rel_offset, d_rel_time, d_position, c->iws.p, s));
    return scratch.release();
}

int rpgpu_uncompress(rpgpu_ctx* c, int codec, const void* in, size_t n, void* out, size_t cap, size_t* out_len) {
    if ((!in && n) || !out_len || (!out && cap)) return RPGPU_E_INVALID;
    // gzip / zstd run on the host: no context needed (ctx may be NULL)
    if (!c && codec != RPGPU_CODEC_GZIP && codec != RPGPU_CODEC_ZSTD) return RPGPU_E_INVALID;
    *out_len = 0;
    if (codec < 0 || codec > RPGPU_CODEC_ZSTD) return fail(c, RPGPU_E_INVALID, "rpgpu_uncompress: unknown codec");
    // compressor::uncompress (compression/compression.cc:34-53): an empty
    // buffer throws before the codec dispatch
    if (n == 0) return fail(c, RPGPU_E_CODEC, "rpgpu_uncompress: asked to decompress an empty buffer");
    if (codec == RPGPU_CODEC_NONE) return fail(c, RPGPU_E_CODEC, "compressor: nothing to uncompress for 'none'");
    if (codec == RPGPU_CODEC_GZIP || codec == RPGPU_CODEC_ZSTD) return host_codec(c, codec, in, n, out, cap, out_len);
    hipSetDevice(c->device);
    const uint64_t dcap = decode_capacity_dev(codec, (const uint8_t*)in, n);
    const size_t in_sz = align_up(n + 16, 256), out_sz = align_up(dcap + 16, 256);
    const size_t need = in_sz + out_sz + 256;
    if (int rc = grow(c, c->uws, need, c->stream, "uncompress workspace")) return rc;
    uint8_t* d_in = c->uws.as<uint8_t>();
    uint8_t* d_out = d_in + in_sz;
    int64_t* d_res = (int64_t*)(d_out + out_sz);
    HIPCHK(c, hipMemsetAsync(d_in + n, 0, in_sz - n, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_uncompress_one(codec, d_in, n, d_out, out_sz, d_res, c->stream));
    int64_t res[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (res[0] != 0) return fail(c, RPGPU_E_CODEC, "rpgpu_uncompress: payload rejected");
    *out_len = (size_t)res[1];
    if ((size_t)res[1] > cap) return fail(c, RPGPU_E_OVERFLOW, "rpgpu_uncompress: output capacity too small");
    if (res[1]) HIPCHK(c, hipMemcpy(out, d_out, (size_t)res[1], hipMemcpyDeviceToHost));
    return RPGPU_OK;
}

// Write side: stamp the headers of n batches in place (rp_validate.hip
// k_stamp; disk_log_appender.cc:72-74 + parser_utils.cc:114-120).
int rpgpu_stamp(rpgpu_ctx* c, uint8_t* d_data, const uint64_t* d_pos, const uint32_t* d_payload_len, uint32_t n,
                int64_t next_offset, uint32_t flags, void* stream) {
    if (!c) return RPGPU_E_INVALID;
    if (n == 0) return RPGPU_OK;
    if (!d_data || !d_pos || ((flags & RPGPU_STAMP_CRC) && !d_payload_len) ||
        (flags & ~(RPGPU_STAMP_OFFSETS | RPGPU_STAMP_CRC)))
        return fail(c, RPGPU_E_INVALID, "rpgpu_stamp: bad argument");
    if (((uintptr_t)d_data & 15) != 0) return fail(c, RPGPU_E_INVALID, "rpgpu_stamp: d_data must be 16-byte aligned");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    const size_t o_steps = 0, o_scan = align_up((size_t)(n + 1) * 8, 256);
    const size_t o_cur = align_up(o_scan + scan_temp_bytes(n) + 64, 256), need = o_cur + 256;
    if (int rc = grow(c, c->sws, need, s, "rpgpu_stamp workspace")) return rc;
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    uint8_t* w = c->sws.as<uint8_t>();
    uint64_t* steps = (uint64_t*)(w + o_steps);
    uint32_t* cursor = (uint32_t*)(w + o_cur);
    HIPCHK(c, hipMemsetAsync(cursor, 0, 4, s));
    if (flags & RPGPU_STAMP_OFFSETS) {
        HIPCHK(c, launch_stamp_steps(d_data, d_pos, n, steps, s));
        HIPCHK(c, scan_exclusive_u64(steps, n, w + o_scan, scan_temp_bytes(n) + 64, s));
    }
    HIPCHK(c, launch_stamp(d_data, d_pos, d_payload_len, steps, next_offset, n, flags, c->d_tables, cursor, c->cu_count, s));
    return scratch.release();
}

// Key compaction over a completed job's outputs (kernels in rp_compact.hip).
size_t rpgpu_compact_sizeof(int which) {
    switch (which) {
    case 0: return sizeof(rpgpu_compact_batch);
    case 1: return sizeof(rpgpu_compact_segment);
    case 2: return sizeof(rpgpu_compact_totals);
    case 3: return sizeof(rpgpu_compact_job);
    default: return 0;
    }
}

int rpgpu_compact(rpgpu_ctx* c, const rpgpu_compact_job* job, void* stream) {
    if (!c || !job) return RPGPU_E_INVALID;
    if (!job->d_totals || !job->d_ctotals || !job->d_out_seg_offsets)
        return fail(c, RPGPU_E_INVALID, "rpgpu_compact: missing argument");
    if (job->n_segments && (!job->d_seg_offsets || !job->d_summaries || !job->d_seg))
        return fail(c, RPGPU_E_INVALID, "rpgpu_compact: missing segment arrays");
    if ((job->batch_capacity && (!job->d_batches || !job->d_data)) || (job->record_capacity && (!job->d_records || !job->d_keep)))
        return fail(c, RPGPU_E_INVALID, "rpgpu_compact: missing job outputs");
    if ((job->out_capacity && !job->d_out) || (job->out_batch_capacity && !job->d_out_batches))
        return fail(c, RPGPU_E_INVALID, "rpgpu_compact: missing output buffer");
    if (((uintptr_t)job->d_out & 15) != 0) return fail(c, RPGPU_E_INVALID, "rpgpu_compact: d_out must be 16-byte aligned");
    if (job->record_capacity >= 0xFFFFFFFFull || job->batch_capacity >= 0xFFFFFFFFull || job->n_segments > 0x7FFFFFFFu)
        return fail(c, RPGPU_E_INVALID, "rpgpu_compact: capacity out of range");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    const uint64_t nb = job->batch_capacity, nr = job->record_capacity, nseg = job->n_segments;
    uint64_t words = 64;
    while (words < 2 * nr) words <<= 1;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t o = need; need += align_up(bytes, 256); return o; };
    const size_t o_table = take(words * 8), o_state = take(nseg * 4), o_acc = take(nseg * 24);
    const size_t o_bpos = take((nb + 1) * 8), o_bcnt = take((nb + 1) * 8), o_bkept = take(nb * 4), o_bplen = take(nb * 4);
    const size_t o_spos = take(nb * 8), o_splen = take(nb * 4), o_scan = take(scan_temp_bytes(nb) + 64), o_cnt = take(256);
    need += 256;
    if (int rc = grow(c, c->cws, need, s, "rpgpu_compact workspace")) return rc;
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    uint8_t* w = c->cws.as<uint8_t>();
    CompactArgs a;
    a.job = *job;
    a.nb = nb;
    a.nr = nr;
    a.table = (uint64_t*)(w + o_table);
    a.table_mask = words - 1;
    a.tag_mask = diag().ckey_tag_mask;  // diagnostic build: few tag bits, so that different keys meet on one tag
    a.seg_state = (uint32_t*)(w + o_state);
    a.seg_acc = (uint64_t*)(w + o_acc);
    a.bpos = (uint64_t*)(w + o_bpos);
    a.bcnt = (uint64_t*)(w + o_bcnt);
    a.bkept = (uint32_t*)(w + o_bkept);
    a.bplen = (uint32_t*)(w + o_bplen);
    a.spos = (uint64_t*)(w + o_spos);
    a.splen = (uint32_t*)(w + o_splen);
    a.counters = (uint32_t*)(w + o_cnt);
    const bool timed = c->timing;
    auto mark = [&](int i) -> hipError_t {
        if (!timed) return hipSuccess;
        if (!c->cev[i]) {
            hipError_t e = hipEventCreate(&c->cev[i]);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(c->cev[i], s);
    };
    c->cev_live = false;
    HIPCHK(c, mark(0));
    HIPCHK(c, hipMemsetAsync(a.table, 0, words * 8, s));
    HIPCHK(c, hipMemsetAsync(a.counters, 0, 256, s));
    HIPCHK(c, hipMemsetAsync(a.bpos, 0, 8, s));
    HIPCHK(c, hipMemsetAsync(a.bcnt, 0, 8, s));
    if (nr) HIPCHK(c, hipMemsetAsync(job->d_keep, 0, (nr + 63) / 64 * 8, s));
    HIPCHK(c, hipMemsetAsync(job->d_ctotals, 0, sizeof(rpgpu_compact_totals), s));
    HIPCHK(c, launch_compact_insert(a, c->cu_count, s));
    HIPCHK(c, mark(1));
    HIPCHK(c, launch_compact_keep(a, c->cu_count, s));
    HIPCHK(c, mark(2));
    HIPCHK(c, launch_compact_size(a, c->cu_count, s));
    if (nb) {
        HIPCHK(c, scan_exclusive_u64(a.bpos, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
        HIPCHK(c, scan_exclusive_u64(a.bcnt, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
    }
    HIPCHK(c, launch_compact_plan(a, s));
    HIPCHK(c, mark(3));
    HIPCHK(c, launch_compact_write(a, c->cu_count, s));
    HIPCHK(c, mark(4));
    const uint64_t nstamp = std::min<uint64_t>(nb, job->out_batch_capacity);
    if (nstamp)
        HIPCHK(c, launch_stamp(job->d_out, a.spos, a.splen, nullptr, 0, (uint32_t)nstamp, RPGPU_STAMP_CRC, c->d_tables,
                               a.counters + kCcStampCursor, c->cu_count, s, a.counters + kCcStampCount));
    HIPCHK(c, mark(5));
    c->cev_live = timed;
    return scratch.release();
}

int rpgpu_compact_timings(rpgpu_ctx* c, float* ms, int n) {
    if (!c || !ms) return RPGPU_E_INVALID;
    if (!c->cev_live) return fail(c, RPGPU_E_INVALID, "rpgpu_compact_timings: no timed rpgpu_compact");
    HIPCHK(c, hipEventSynchronize(c->cev[5]));
    float v[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipEventElapsedTime(&v[0], c->cev[0], c->cev[5]));
    for (int i = 1; i < 6; i++) HIPCHK(c, hipEventElapsedTime(&v[i], c->cev[i - 1], c->cev[i]));
    for (int i = 0; i < n && i < 6; i++) ms[i] = v[i];
    return RPGPU_OK;
}

// Recompression of a completed rpgpu_compact's batches (kernels in
// rp_recompress.hip; the block kernels are rp_compress.hip's).
size_t rpgpu_recompress_sizeof(int which) {
    switch (which) {
    case 0: return sizeof(rpgpu_recompress_batch);
    case 1: return sizeof(rpgpu_recompress_totals);
    case 2: return sizeof(rpgpu_batch_result);
    case 3: return sizeof(rpgpu_recompress_job);
    default: return 0;
    }
}

int rpgpu_recompress(rpgpu_ctx* c, const rpgpu_recompress_job* job, void* stream) {
    if (!c || !job) return RPGPU_E_INVALID;
    if (!job->d_ctotals || !job->d_rtotals || !job->d_in_seg_offsets || !job->d_out_seg_offsets)
        return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: missing argument");
    if (job->n_segments && !job->d_out_summaries) return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: missing segment arrays");
    if (job->in_batch_capacity && (!job->d_in_batches || !job->d_in))
        return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: missing compaction outputs");
    if ((job->out_capacity && !job->d_out) || (job->out_batch_capacity && (!job->d_out_entries || !job->d_out_batches)))
        return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: missing output buffer");
    if (((uintptr_t)job->d_out & 15) != 0) return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: d_out must be 16-byte aligned");
    if (job->codec != RPGPU_RECOMPRESS_SOURCE_CODEC && job->codec > 7)
        return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: codec is neither an rpgpu_codec value nor SOURCE_CODEC");
    // smaller fragments would unbound the block count the scratch is sized for
    if (job->snappy_frag && job->snappy_frag < 4096)
        return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: snappy_frag below 4096");
    const uint64_t nb = job->in_batch_capacity, nseg = job->n_segments;
    const uint64_t block_cap = recompress_block_cap(job->in_capacity, nb, job->snappy_frag);
    // batch ordinals, block ordinals and pack pieces are counted in 32 bits
    if (nb >= 0x7FFFFFFFull || job->out_batch_capacity >= 0x7FFFFFFFull || nseg > 0x7FFFFFFFu || block_cap >= 0x7FFFFFFFull)
        return fail(c, RPGPU_E_INVALID, "rpgpu_recompress: capacity out of range");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    const uint64_t scratch_cap = recompress_scratch_cap(job->in_capacity, block_cap);
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t o = need; need += align_up(bytes, 256); return o; };
    // bblk, bscr, bpos and bcnt lie back to back: one memset zeroes the four
    const size_t plan_bytes = align_up((nb + 1) * 8, 256);
    const size_t o_bblk = take(plan_bytes), o_bscr = take(plan_bytes), o_bpos = take(plan_bytes), o_bcnt = take(plan_bytes);
    const size_t o_mode = take(nb * 4), o_clen = take(nb * 4), o_spos = take(nb * 8), o_splen = take(nb * 4);
    const size_t o_blocks = take(block_cap * sizeof(CompBlock)), o_slot = take(block_cap * 8), o_sizes = take(block_cap * 4);
    const size_t o_scan = take(scan_temp_bytes(nb) + 64), o_cnt = take(256), o_scr = take(scratch_cap + 16);
    need += 256;
    if (int rc = grow(c, c->rws, need, s, "rpgpu_recompress workspace")) return rc;
    // gzip batches (rpgpu_set_device_gzip): one stream each, at most one per input batch
    const bool dgzip = c->device_gzip && nb &&
                       (job->codec == RPGPU_RECOMPRESS_SOURCE_CODEC || job->codec == RPGPU_CODEC_GZIP);
    const uint32_t dstreams = (uint32_t)std::min<uint64_t>(nb, kDeflateStreams);
    if (dgzip)
        if (int rc = grow(c, c->dfw, deflate_work_bytes(dstreams), s, "gzip work areas")) return rc;
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    uint8_t* w = c->rws.as<uint8_t>();
    RecompressArgs a;
    a.job = *job;
    a.nb = nb;
    a.mode = (uint32_t*)(w + o_mode);
    a.bblk = (uint64_t*)(w + o_bblk);
    a.bscr = (uint64_t*)(w + o_bscr);
    a.bpos = (uint64_t*)(w + o_bpos);
    a.bcnt = (uint64_t*)(w + o_bcnt);
    a.clen = (uint32_t*)(w + o_clen);
    a.blocks = (CompBlock*)(w + o_blocks);
    a.block_cap = block_cap;
    a.slot_off = (uint64_t*)(w + o_slot);
    a.sizes = (uint32_t*)(w + o_sizes);
    a.scratch = w + o_scr;
    a.scratch_cap = scratch_cap;
    a.spos = (uint64_t*)(w + o_spos);
    a.splen = (uint32_t*)(w + o_splen);
    a.counters = (uint32_t*)(w + o_cnt);
    const bool timed = c->timing;
    auto mark = [&](int i) -> hipError_t {
        if (!timed) return hipSuccess;
        if (!c->rev[i]) {
            hipError_t e = hipEventCreate(&c->rev[i]);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(c->rev[i], s);
    };
    a.device_gzip = c->device_gzip ? 1u : 0u;
    c->rev_live = false;
    HIPCHK(c, mark(0));
    // the scans leave the totals at [nb]; without batches these zeroes are the totals
    HIPCHK(c, hipMemsetAsync(a.bblk, 0, 4 * plan_bytes, s));
    HIPCHK(c, hipMemsetAsync(a.counters, 0, 256, s));
    HIPCHK(c, hipMemsetAsync(job->d_rtotals, 0, sizeof(rpgpu_recompress_totals), s));
    // the block kernels run over the whole array: a block the plan does not fill has codec 0
    HIPCHK(c, hipMemsetAsync(a.blocks, 0, block_cap * sizeof(CompBlock), s));
    if (nb) HIPCHK(c, launch_recompress_plan(a, w + o_scan, scan_temp_bytes(nb) + 64, s));
    HIPCHK(c, mark(1));
    if (nb) {
        const bool any = job->codec == RPGPU_RECOMPRESS_SOURCE_CODEC;
        HIPCHK(c, launch_compress_blocks(job->d_in, a.blocks, (uint32_t)block_cap, a.scratch, a.slot_off, a.sizes,
                                         any || job->codec == RPGPU_CODEC_LZ4, any || job->codec == RPGPU_CODEC_SNAPPY, s));
        if (dgzip)
            HIPCHK(c, launch_deflate_blocks(job->d_in, a.blocks, (uint32_t)block_cap, a.scratch, a.slot_off, a.sizes,
                                            c->dfw.as<uint8_t>(), dstreams, s));
    }
    HIPCHK(c, mark(2));
    HIPCHK(c, launch_recompress_layout(a, w + o_scan, scan_temp_bytes(nb) + 64, s));
    HIPCHK(c, mark(3));
    if (nb) HIPCHK(c, launch_recompress_pack(a, c->cu_count, s));
    HIPCHK(c, mark(4));
    // compress_batch's reset_size_checksum_metadata, then header_crc
    const uint64_t nstamp = std::min<uint64_t>(nb, job->out_batch_capacity);
    if (nstamp && job->codec != RPGPU_CODEC_NONE)
        HIPCHK(c, launch_stamp(job->d_out, a.spos, a.splen, nullptr, 0, (uint32_t)nstamp, RPGPU_STAMP_CRC, c->d_tables,
                               a.counters + kRcStampCursor, c->cu_count, s, a.counters + kRcStampCount));
    if (nb) HIPCHK(c, launch_recompress_meta(a, s));
    HIPCHK(c, mark(5));
    c->rev_live = timed;
    return scratch.release();
}

int rpgpu_recompress_timings(rpgpu_ctx* c, float* ms, int n) {
    if (!c || !ms) return RPGPU_E_INVALID;
    if (!c->rev_live) return fail(c, RPGPU_E_INVALID, "rpgpu_recompress_timings: no timed rpgpu_recompress");
    HIPCHK(c, hipEventSynchronize(c->rev[5]));
    float v[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipEventElapsedTime(&v[0], c->rev[0], c->rev[5]));
    for (int i = 1; i < 6; i++) HIPCHK(c, hipEventElapsedTime(&v[i], c->rev[i - 1], c->rev[i]));
    for (int i = 0; i < n && i < 6; i++) ms[i] = v[i];
    return RPGPU_OK;
}

// The produce path's append over a completed wire-layout job's outputs
// (kernels in rp_append.hip).
size_t rpgpu_append_sizeof(int which) {
    switch (which) {
    case 0: return sizeof(rpgpu_append_set);
    case 1: return sizeof(rpgpu_append_totals);
    case 2: return sizeof(rpgpu_batch_result);
    case 3: return sizeof(rpgpu_append_job);
    default: return 0;
    }
}

int rpgpu_append_wire(rpgpu_ctx* c, const rpgpu_append_job* job, void* stream) {
    if (!c || !job) return RPGPU_E_INVALID;
    if (!job->d_totals || !job->d_atotals || !job->d_out_seg_offsets)
        return fail(c, RPGPU_E_INVALID, "rpgpu_append_wire: missing argument");
    if (job->n_segments && (!job->d_seg_offsets || !job->d_summaries || !job->d_next_offset || !job->d_sets ||
                            !job->d_out_summaries))
        return fail(c, RPGPU_E_INVALID, "rpgpu_append_wire: missing set arrays");
    if (job->batch_capacity && (!job->d_batches || !job->d_data))
        return fail(c, RPGPU_E_INVALID, "rpgpu_append_wire: missing job outputs");
    if ((job->out_capacity && !job->d_out) || (job->out_batch_capacity && !job->d_out_batches))
        return fail(c, RPGPU_E_INVALID, "rpgpu_append_wire: missing output buffer");
    if (((uintptr_t)job->d_out & 15) != 0)
        return fail(c, RPGPU_E_INVALID, "rpgpu_append_wire: d_out must be 16-byte aligned");
    if (job->flags & ~RPGPU_APPEND_ALL_BATCHES) return fail(c, RPGPU_E_INVALID, "rpgpu_append_wire: unknown flag");
    // batch ordinals and copy pieces are counted in 32 bits
    if (job->batch_capacity >= 0x7FFFFFFFull || job->n_segments > 0x7FFFFFFFu ||
        job->out_capacity / kAppendPiece >= 0x7FFFFFFFull)
        return fail(c, RPGPU_E_INVALID, "rpgpu_append_wire: capacity out of range");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    const uint64_t nb = job->batch_capacity, nseg = job->n_segments;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t o = need; need += align_up(bytes, 256); return o; };
    const size_t o_bad = take(nseg * 4), o_verdict = take(nb * 4), o_bpos = take((nb + 1) * 8), o_bcnt = take((nb + 1) * 8);
    const size_t o_bstep = take((nb + 1) * 8), o_spos = take(nb * 8), o_splen = take(nb * 4);
    const size_t o_scan = take(scan_temp_bytes(nb) + 64), o_cnt = take(256);
    need += 256;
    if (int rc = grow(c, c->aws, need, s, "rpgpu_append_wire workspace")) return rc;
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    uint8_t* w = c->aws.as<uint8_t>();
    AppendArgs a;
    a.job = *job;
    a.nb = nb;
    a.seg_bad = (uint32_t*)(w + o_bad);
    a.verdict = (uint32_t*)(w + o_verdict);
    a.bpos = (uint64_t*)(w + o_bpos);
    a.bcnt = (uint64_t*)(w + o_bcnt);
    a.bstep = (uint64_t*)(w + o_bstep);
    a.spos = (uint64_t*)(w + o_spos);
    a.splen = (uint32_t*)(w + o_splen);
    a.counters = (uint32_t*)(w + o_cnt);
    a.tables = c->d_tables;
    const bool timed = c->timing;
    auto mark = [&](int i) -> hipError_t {
        if (!timed) return hipSuccess;
        if (!c->aev[i]) {
            hipError_t e = hipEventCreate(&c->aev[i]);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(c->aev[i], s);
    };
    c->aev_live = false;
    HIPCHK(c, mark(0));
    if (nseg) HIPCHK(c, hipMemsetAsync(a.seg_bad, 0xFF, nseg * 4, s));
    HIPCHK(c, hipMemsetAsync(a.counters, 0, 256, s));
    // the scans leave the totals at [nb]; without batches these are the totals
    HIPCHK(c, hipMemsetAsync(a.bpos + nb, 0, 8, s));
    HIPCHK(c, hipMemsetAsync(a.bcnt + nb, 0, 8, s));
    HIPCHK(c, hipMemsetAsync(a.bstep + nb, 0, 8, s));
    HIPCHK(c, hipMemsetAsync(job->d_atotals, 0, sizeof(rpgpu_append_totals), s));
    if (nb) HIPCHK(c, launch_append_sizes(a, s));
    HIPCHK(c, mark(1));
    if (nb) {
        HIPCHK(c, scan_exclusive_u64(a.bpos, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
        HIPCHK(c, scan_exclusive_u64(a.bcnt, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
        HIPCHK(c, scan_exclusive_u64(a.bstep, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
    }
    HIPCHK(c, launch_append_plan(a, s));
    HIPCHK(c, mark(2));
    if (nb) HIPCHK(c, launch_append_copy(a, c->cu_count, s));
    HIPCHK(c, mark(3));
    // set_max_timestamp changed attrs / max_timestamp of the append-time
    // batches: crc_record_batch again, then header_crc (model/record.h:598-608)
    const uint64_t nstamp = std::min<uint64_t>(nb, job->out_batch_capacity);
    if (nstamp && job->d_append_time)
        HIPCHK(c, launch_stamp(job->d_out, a.spos, a.splen, nullptr, 0, (uint32_t)nstamp, RPGPU_STAMP_CRC, c->d_tables,
                               a.counters + kAcStampCursor, c->cu_count, s, a.counters + kAcStampCount));
    HIPCHK(c, mark(4));
    if (nb) HIPCHK(c, launch_append_meta(a, s));
    HIPCHK(c, mark(5));
    c->aev_live = timed;
    return scratch.release();
}

int rpgpu_append_timings(rpgpu_ctx* c, float* ms, int n) {
    if (!c || !ms) return RPGPU_E_INVALID;
    if (!c->aev_live) return fail(c, RPGPU_E_INVALID, "rpgpu_append_timings: no timed rpgpu_append_wire");
    HIPCHK(c, hipEventSynchronize(c->aev[5]));
    float v[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipEventElapsedTime(&v[0], c->aev[0], c->aev[5]));
    for (int i = 1; i < 6; i++) HIPCHK(c, hipEventElapsedTime(&v[i], c->aev[i - 1], c->aev[i]));
    for (int i = 0; i < n && i < 6; i++) ms[i] = v[i];
    return RPGPU_OK;
}

// The fetch path's log read over a completed disk-layout job's outputs
// (kernels in rp_fetch.hip).
size_t rpgpu_fetch_sizeof(int which) {
    switch (which) {
    case 0: return sizeof(rpgpu_fetch_request);
    case 1: return sizeof(rpgpu_fetch_part);
    case 2: return sizeof(rpgpu_fetch_batch);
    case 3: return sizeof(rpgpu_fetch_totals);
    case 4: return sizeof(rpgpu_fetch_job);
    default: return 0;
    }
}

int rpgpu_fetch(rpgpu_ctx* c, const rpgpu_fetch_job* job, void* stream) {
    if (!c || !job) return RPGPU_E_INVALID;
    if (!job->d_totals || !job->d_ftotals || !job->d_out_part_offsets || !job->d_part_segments)
        return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: missing argument");
    if (job->n_partitions && (!job->d_requests || !job->d_parts))
        return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: missing partition arrays");
    if (job->n_segments && (!job->d_seg_offsets || !job->d_summaries))
        return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: missing segment arrays");
    if (job->batch_capacity && (!job->d_batches || !job->d_data))
        return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: missing job outputs");
    const int have_index = (job->d_index_states != nullptr) + (job->d_rel_offset != nullptr) + (job->d_position != nullptr);
    if (have_index != 0 && have_index != 3)
        return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: the entry index needs all three arrays");
    if ((job->out_capacity && !job->d_out) || (job->out_batch_capacity && !job->d_out_batches))
        return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: missing output buffer");
    if (((uintptr_t)job->d_out & 15) != 0) return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: d_out must be 16-byte aligned");
    // batch ordinals, output slots and copy pieces are counted in 32 bits
    if (job->batch_capacity >= 0x7FFFFFFFull || job->n_segments > 0x7FFFFFFFu || job->n_partitions > 0x7FFFFFFFu ||
        job->out_batch_capacity >= 0x7FFFFFFFull || job->out_capacity / kAppendPiece >= 0x7FFFFFFFull)
        return fail(c, RPGPU_E_INVALID, "rpgpu_fetch: capacity out of range");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    const uint64_t nb = job->batch_capacity, np = job->n_partitions;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t o = need; need += align_up(bytes, 256); return o; };
    // bpos, bcnt and brec lie back to back: one memset zeroes the three
    const size_t plan_bytes = align_up((nb + 1) * 8, 256);
    const size_t o_bpos = take(plan_bytes), o_bcnt = take(plan_bytes), o_brec = take(plan_bytes);
    const size_t o_bpart = take(nb * 4), o_sel = take(np * sizeof(FetchSel));
    const size_t o_scan = take(scan_temp_bytes(nb) + 64);
    need += 256;
    if (int rc = grow(c, c->fws, need, s, "rpgpu_fetch workspace")) return rc;
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    uint8_t* w = c->fws.as<uint8_t>();
    FetchArgs a;
    a.job = *job;
    a.nb = nb;
    a.bpos = (uint64_t*)(w + o_bpos);
    a.bcnt = (uint64_t*)(w + o_bcnt);
    a.brec = (uint64_t*)(w + o_brec);
    a.bpart = (uint32_t*)(w + o_bpart);
    a.sel = (FetchSel*)(w + o_sel);
    const bool timed = c->timing;
    auto mark = [&](int i) -> hipError_t {
        if (!timed) return hipSuccess;
        if (!c->fev[i]) {
            hipError_t e = hipEventCreate(&c->fev[i]);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(c->fev[i], s);
    };
    c->fev_live = false;
    HIPCHK(c, mark(0));
    // k_fetch_select writes the returned batches only; the scans leave the
    // totals at [nb], without batches these zeroes are the totals
    HIPCHK(c, hipMemsetAsync(a.bpos, 0, 3 * plan_bytes, s));
    HIPCHK(c, hipMemsetAsync(job->d_ftotals, 0, sizeof(rpgpu_fetch_totals), s));
    if (np) HIPCHK(c, launch_fetch_select(a, s));
    HIPCHK(c, mark(1));
    if (nb) {
        HIPCHK(c, scan_exclusive_u64(a.bpos, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
        HIPCHK(c, scan_exclusive_u64(a.bcnt, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
        HIPCHK(c, scan_exclusive_u64(a.brec, nb, w + o_scan, scan_temp_bytes(nb) + 64, s));
    }
    HIPCHK(c, launch_fetch_plan(a, s));
    HIPCHK(c, mark(2));
    if (nb && np) HIPCHK(c, launch_fetch_copy(a, c->cu_count, s));
    HIPCHK(c, mark(3));
    HIPCHK(c, mark(4));
    c->fev_live = timed;
    return scratch.release();
}

int rpgpu_fetch_timings(rpgpu_ctx* c, float* ms, int n) {
    if (!c || !ms) return RPGPU_E_INVALID;
    if (!c->fev_live) return fail(c, RPGPU_E_INVALID, "rpgpu_fetch_timings: no timed rpgpu_fetch");
    HIPCHK(c, hipEventSynchronize(c->fev[4]));
    float v[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipEventElapsedTime(&v[0], c->fev[0], c->fev[4]));
    for (int i = 1; i < 5; i++) HIPCHK(c, hipEventElapsedTime(&v[i], c->fev[i - 1], c->fev[i]));
    for (int i = 0; i < n && i < 5; i++) ms[i] = v[i];
    return RPGPU_OK;
}

// kafka::writer_serialize_batch over batches [first, first + n) of a
// completed disk-layout job (kafka/protocol/response_writer.h:241-276):
// the Kafka v2 record set, back to back in d_wire; *d_total (device) gets
// its length.  Asynchronous on `stream`.
int rpgpu_serialize_wire(rpgpu_ctx* c, const uint8_t* d_data, const uint64_t* d_seg_offsets,
                         const rpgpu_batch_result* d_batches, uint64_t first, uint32_t n, uint8_t* d_wire,
                         uint64_t* d_total, void* stream) {
    if (!c) return RPGPU_E_INVALID;
    if (!d_data || !d_seg_offsets || !d_batches || !d_wire || !d_total)
        return fail(c, RPGPU_E_INVALID, "rpgpu_serialize_wire: missing argument");
    hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    const size_t o_dst = align_up((size_t)(n + 1) * 8, 256), o_scan = o_dst + align_up((size_t)(n + 1) * 8, 256);
    const size_t need = o_scan + scan_temp_bytes(n) + 256;
    if (int rc = grow(c, c->sws, need, s, "rpgpu_serialize_wire workspace")) return rc;
    ScratchScope scratch(c, s);
    if (int rc = scratch.acquired()) return rc;
    uint8_t* w = c->sws.as<uint8_t>();
    uint64_t* src = (uint64_t*)w;
    uint64_t* dst = (uint64_t*)(w + o_dst);
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(d_total, 0, 8, s));
        return scratch.release();
    }
    HIPCHK(c, launch_to_wire(d_data, d_wire, d_batches, d_seg_offsets, first, n, src, dst, w + o_scan,
                             scan_temp_bytes(n) + 64, c->cu_count * 8, s));
    HIPCHK(c, hipMemcpyAsync(d_total, dst + n, 8, hipMemcpyDeviceToDevice, s));
    return scratch.release();
}

// Many payloads per GPU round trip (the per-batch call sites of
// compressor::uncompress, storage/parser_utils.cc:51 and
// kafka/protocol/kafka_batch_adapter.cc:259, batched): lz4/snappy payloads
// are staged into one pinned buffer, copied once, decoded one per lane, and
// their outputs copied back once; gzip/zstd go to the host fallback; every
// payload gets its own status (the rpgpu_uncompress codes).
int rpgpu_uncompress_batch(rpgpu_ctx* c, uint32_t n, const int* codecs, const void* const* in, const size_t* in_len,
                           void* const* out, const size_t* cap, size_t* out_len, int* status) {
    if (!c || (n && (!codecs || !in || !in_len || !out || !cap || !out_len || !status))) return RPGPU_E_INVALID;
    std::vector<uint32_t> dev;  // payloads decoded on the device
    std::vector<UncItem> items;
    uint64_t in_total = 0, out_total = 0;
    for (uint32_t i = 0; i < n; i++) {
        out_len[i] = 0;
        const int codec = codecs[i];
        if (codec < 0 || codec > RPGPU_CODEC_ZSTD || (!in[i] && in_len[i])) { status[i] = RPGPU_E_INVALID; continue; }
        if (in_len[i] == 0 || codec == RPGPU_CODEC_NONE) { status[i] = RPGPU_E_CODEC; continue; }
        if (codec == RPGPU_CODEC_GZIP || codec == RPGPU_CODEC_ZSTD) {
            status[i] = host_codec(c, codec, in[i], in_len[i], out[i], cap[i], &out_len[i]);
            continue;
        }
        UncItem it;
        it.src = in_total;
        it.n = in_len[i];
        it.dst = out_total;
        it.cap = align_up(decode_capacity_dev(codec, (const uint8_t*)in[i], in_len[i]) + 16, 16);
        it.codec = codec;
        it.pad = 0;
        in_total += align_up(in_len[i], 16);
        out_total += it.cap;
        items.push_back(it);
        dev.push_back(i);
        status[i] = RPGPU_E_CODEC;
    }
    if (items.empty()) return RPGPU_OK;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const uint32_t m = (uint32_t)items.size();
    // device: [inputs + 16][items][results][outputs]; host (pinned): the same
    // first three parts, then the outputs coming back
    const size_t o_items = align_up(in_total + 16, 256), o_res = align_up(o_items + m * sizeof(UncItem), 256);
    const size_t o_out = align_up(o_res + (size_t)m * 16, 256), total = o_out + out_total;
    if (int rc = grow(c, c->bd, total, s, "uncompress batch staging")) return rc;
    if (int rc = grow(c, c->bh, total, s, "uncompress batch pinned staging")) return rc;
    uint8_t* h = c->bh.as<uint8_t>();
    uint8_t* d = c->bd.as<uint8_t>();
    std::memset(h + in_total, 0, o_items - in_total);
    for (uint32_t k = 0; k < m; k++) std::memcpy(h + items[k].src, in[dev[k]], items[k].n);
    std::memcpy(h + o_items, items.data(), m * sizeof(UncItem));
    HIPCHK(c, hipMemcpyAsync(d, h, o_res, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_uncompress_many((const UncItem*)(d + o_items), m, d, in_total + 16, d + o_out, (int64_t*)(d + o_res), s));
    HIPCHK(c, hipMemcpyAsync(h + o_res, d + o_res, total - o_res, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int64_t* res = (const int64_t*)(h + o_res);
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = dev[k];
        if (res[2 * k] != 0) { status[i] = RPGPU_E_CODEC; continue; }
        out_len[i] = (size_t)res[2 * k + 1];
        if (out_len[i] > cap[i]) { status[i] = RPGPU_E_OVERFLOW; continue; }
        if (out_len[i]) std::memcpy(out[i], h + o_out + items[k].dst, out_len[i]);
        status[i] = RPGPU_OK;
    }
    return RPGPU_OK;
}

// compressor::compress for lz4 / snappy (rp_compress.hip)
size_t rpgpu_compress_bound(int codec, size_t n, size_t frag) {
    if (codec == RPGPU_CODEC_LZ4) return 15 + ((n + 65535) / 65536) * (4 + 65536) + 4;
    if (codec == RPGPU_CODEC_SNAPPY) {
        if (frag == 0 || frag > n) frag = n ? n : 1;
        const size_t nf = n ? (n + frag - 1) / frag : 0;
        return 16 + nf * (4 + 32 + frag + frag / 6);  // snappy::MaxCompressedLength per fragment
    }
    // deflateBound / ZSTD_compressBound, generously (per-fragment flushes add
    // a few bytes each)
    if (codec == RPGPU_CODEC_GZIP || codec == RPGPU_CODEC_ZSTD) {
        const size_t nf = frag ? (n + frag - 1) / frag : 1;
        return n + n / 64 + 1024 + nf * 16;
    }
    return 0;
}

int rpgpu_compress_batch(rpgpu_ctx* c, uint32_t n, const int* codecs, const void* const* in, const size_t* in_len,
                         const size_t* frag, void* const* out, const size_t* cap, size_t* out_len, int* status) {
    // ctx may be NULL when every payload is gzip / zstd (host work only)
    if (n && (!codecs || !in || !in_len || !out || !cap || !out_len || !status)) return RPGPU_E_INVALID;
    std::vector<uint32_t> dev;
    std::vector<CompPayload> pays;
    std::vector<CompBlock> blocks;
    // staged input pieces: (host bytes, length, staged offset); every snappy
    // fragment (each a RawCompress of its own) starts 16-byte aligned, as
    // the block kernels' dword reads assume
    struct Stage { const uint8_t* src; uint64_t n, off; };
    std::vector<Stage> stage;
    // gzip payloads the device takes (rpgpu_set_device_gzip): one k_deflate
    // stream each, its output slot among the frames'
    std::vector<uint32_t> dfl_dev;
    std::vector<DeflateItem> dfl;
    uint64_t in_total = 0, out_total = 0;
    for (uint32_t i = 0; i < n; i++) {
        out_len[i] = 0;
        const int codec = codecs[i];
        if (codec < 0 || codec > RPGPU_CODEC_ZSTD || (!in[i] && in_len[i])) { status[i] = RPGPU_E_INVALID; continue; }
        if (codec == RPGPU_CODEC_NONE) { status[i] = RPGPU_E_CODEC; continue; }
        if (codec == RPGPU_CODEC_GZIP && c && c->device_gzip && df::takes(in_len[i])) {
            DeflateItem it;
            it.src = in_total;
            it.n = in_len[i];
            it.frag = frag ? frag[i] : 0;
            it.out = out_total;
            stage.push_back({(const uint8_t*)in[i], it.n, in_total});
            in_total += align_up(it.n + 8, 16);
            out_total += align_up(df::bound(it.n), 16);
            dfl.push_back(it);
            dfl_dev.push_back(i);
            status[i] = RPGPU_E_CODEC;
            continue;
        }
        if (codec == RPGPU_CODEC_GZIP || codec == RPGPU_CODEC_ZSTD) {
            // the CPU fallback: the reference's loops over zlib / libzstd
            const int r = host_compress(codec, (const uint8_t*)in[i], in_len[i], frag ? frag[i] : 0, (uint8_t*)out[i],
                                        cap[i], &out_len[i]);
            status[i] = r == 0 ? RPGPU_OK
                        : r == kHostCodecOverflow ? RPGPU_E_OVERFLOW
                        : r == kHostCodecMissing  ? RPGPU_E_UNSUPPORTED
                                                  : RPGPU_E_CODEC;
            continue;
        }
        // 32-bit frame fields (CompBlock::frag_len, the snappy length varint
        // and BE32 chunk length) hold lengths below 4 GiB only
        if (!c || in_len[i] >= (1ull << 32)) { status[i] = RPGPU_E_INVALID; continue; }
        const uint64_t len = in_len[i];
        uint64_t fr = (codec == RPGPU_CODEC_SNAPPY && frag && frag[i]) ? frag[i] : len;
        if (fr == 0) fr = 1;
        // snappy_java_compressor::compress writes int32_t(omax) per fragment
        // (compression/internal/snappy_java_compressor.cc:58-75): a fragment
        // whose bound does not fit int32 cannot be framed
        if (codec == RPGPU_CODEC_SNAPPY && 32 + std::min<uint64_t>(fr, len) + std::min<uint64_t>(fr, len) / 6 > 0x7FFFFFFFull) {
            status[i] = RPGPU_E_INVALID;
            continue;
        }
        CompPayload p;
        p.n = len;
        p.out = out_total;
        p.first = (uint32_t)blocks.size();
        p.codec = (uint32_t)codec;
        p.pad = 0;
        const uint8_t* src = (const uint8_t*)in[i];
        for (uint64_t f = 0; f < len; f += (codec == RPGPU_CODEC_LZ4 ? len : fr)) {
            // lz4: the frame's 64 KiB blocks whatever the fragmentation;
            // snappy: each fragment is a RawCompress of its own
            const uint64_t flen = codec == RPGPU_CODEC_LZ4 ? len : std::min<uint64_t>(fr, len - f);
            const uint32_t nbk = (uint32_t)((flen + 65535) / 65536);
            for (uint32_t k = 0; k < nbk; k++) {
                CompBlock b;
                b.src = in_total + (uint64_t)k * 65536;
                b.n = (uint32_t)std::min<uint64_t>(65536, flen - (uint64_t)k * 65536);
                b.codec = (uint32_t)codec;
                b.frag_len = k == 0 ? (uint32_t)flen : 0;
                b.frag_blocks = k == 0 ? nbk : 0;
                blocks.push_back(b);
            }
            stage.push_back({src + f, flen, in_total});
            in_total += align_up(flen + 8, 16);
        }
        p.nblocks = (uint32_t)blocks.size() - p.first;
        pays.push_back(p);
        dev.push_back(i);
        out_total += align_up(rpgpu_compress_bound(codec, len, fr), 16);
        status[i] = RPGPU_E_CODEC;
    }
    if (pays.empty() && dfl.empty()) return RPGPU_OK;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const uint32_t np = (uint32_t)pays.size(), nb = (uint32_t)blocks.size(), nd = (uint32_t)dfl.size();
    // device: [inputs][blocks][payloads][deflate items] | [out_len: frames,
    // then gzip streams][sizes][outputs][scratch]; host (pinned): the first
    // part, then out_len + outputs coming back
    const size_t o_blk = align_up(in_total + 16, 256), o_pay = align_up(o_blk + (size_t)nb * sizeof(CompBlock), 256);
    const size_t o_dfi = align_up(o_pay + (size_t)np * sizeof(CompPayload), 256);
    const size_t o_len = align_up(o_dfi + (size_t)nd * sizeof(DeflateItem), 256);
    const size_t o_sz = align_up(o_len + (size_t)(np + nd) * 8, 256), o_out = align_up(o_sz + (size_t)nb * 4, 256);
    const size_t o_scr = align_up(o_out + out_total, 256), total = o_scr + (size_t)nb * kCompSlot;
    if (int rc = grow(c, c->bd, total, s, "compress staging")) return rc;
    if (int rc = grow(c, c->bh, o_scr, s, "compress pinned staging")) return rc;
    uint8_t* h = c->bh.as<uint8_t>();
    uint8_t* d = c->bd.as<uint8_t>();
    std::memset(h, 0, o_blk);
    for (const Stage& st : stage)
        if (st.n) std::memcpy(h + st.off, st.src, st.n);
    std::memcpy(h + o_blk, blocks.data(), nb * sizeof(CompBlock));
    std::memcpy(h + o_pay, pays.data(), np * sizeof(CompPayload));
    if (nd) std::memcpy(h + o_dfi, dfl.data(), nd * sizeof(DeflateItem));
    const uint32_t streams = std::min(nd, kDeflateStreams);
    if (nd)
        if (int rc = grow(c, c->dfw, deflate_work_bytes(streams), s, "gzip work areas")) return rc;
    const bool dtimed = nd && c->timing;
    c->dev_live = false;
    if (dtimed)
        for (int k = 0; k < 2; k++)
            if (!c->dev[k]) HIPCHK(c, hipEventCreate(&c->dev[k]));
    HIPCHK(c, hipMemcpyAsync(d, h, o_len, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_compress(d, (const CompBlock*)(d + o_blk), nb, (const CompPayload*)(d + o_pay), np, d + o_scr,
                              (uint32_t*)(d + o_sz), d + o_out, (uint64_t*)(d + o_len), s));
    if (dtimed) HIPCHK(c, hipEventRecord(c->dev[0], s));
    if (nd)
        HIPCHK(c, launch_deflate(d, (const DeflateItem*)(d + o_dfi), nd, d + o_out, (uint64_t*)(d + o_len) + np,
                                 c->dfw.as<uint8_t>(), streams, s));
    if (dtimed) {
        HIPCHK(c, hipEventRecord(c->dev[1], s));
        c->dev_live = true;
    }
    HIPCHK(c, hipMemcpyAsync(h + o_len, d + o_len, (size_t)(np + nd) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(h + o_out, d + o_out, out_total, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint64_t* lens = (const uint64_t*)(h + o_len);
    for (uint32_t k = 0; k < np; k++) {
        const uint32_t i = dev[k];
        out_len[i] = (size_t)lens[k];
        if (out_len[i] > cap[i]) { status[i] = RPGPU_E_OVERFLOW; continue; }
        std::memcpy(out[i], h + o_out + pays[k].out, out_len[i]);
        status[i] = RPGPU_OK;
    }
    for (uint32_t k = 0; k < nd; k++) {
        const uint32_t i = dfl_dev[k];
        out_len[i] = (size_t)lens[np + k];
        if (out_len[i] > cap[i]) { status[i] = RPGPU_E_OVERFLOW; continue; }
        std::memcpy(out[i], h + o_out + dfl[k].out, out_len[i]);
        status[i] = RPGPU_OK;
    }
    c->gzip_dev_payloads += nd;
    return RPGPU_OK;
}

// ---------------------------------------------------------------------------
// Host segment path (log_replayer over files, storage/log_replayer.cc:95-114):
// host-resident segments are grouped into staging groups of at most
// kHostGroupBytes (a larger segment is a group of its own), copied H2D with
// hipMemcpyAsync on the context's copy stream into one of two device slots,
// and validated by the same pipeline as rpgpu_submit on the compute stream;
// while group g validates, group g + 1 is being copied and group g - 1's
// per-batch results come back.  Outputs are the caller's host arrays; the
// record index and decoded bytes stay on the device (the verdict bits,
// records_parsed and the decoded crcs are in the batch results).  A group
// whose device outputs overflowed is re-run with the capacities the device
// reported, so the host sees the same results as one big rpgpu_submit.
// ---------------------------------------------------------------------------
}  // extern "C"

namespace {
constexpr uint64_t kHostGroupBytes = 256ull << 20;

// staging-group size: rpgpu_host_job.group_kib, 0 = kHostGroupBytes (tests
// use small groups to exercise the double buffering on small inputs)
uint64_t host_group_bytes(const rpgpu_host_job* job) {
    return job->group_kib ? (uint64_t)job->group_kib << 10 : kHostGroupBytes;
}

// a slot's staging for n elements of T (its capacity is count<T>())
template <class T>
int slot_grow(rpgpu_ctx* c, Buf& b, uint64_t n) {
    return grow(c, b, (size_t)std::max<uint64_t>(n, 1) * sizeof(T), c->stream, "rpgpu_validate_host: device staging");
}
template <class T>
uint64_t count(const Buf& b) { return b.bytes / sizeof(T); }

struct HostGroup {
    uint32_t seg0, nseg;
    uint64_t bytes;
};

// issue group g on slot h: H2D on the copy stream, then the pipeline on the
// compute stream (after the copy), then the totals back to pinned memory
int host_issue(rpgpu_ctx* c, rpgpu_ctx::HostSlot& h, const rpgpu_host_job* job, const HostGroup& g) {
    const uint64_t padded = align_up(g.bytes + 64, 256);
    if (int rc = slot_grow<uint8_t>(c, h.d_data, padded)) return rc;
    if (int rc = slot_grow<uint64_t>(c, h.d_offs, (uint64_t)g.nseg + 1)) return rc;
    if (int rc = slot_grow<rpgpu_segment_summary>(c, h.d_sums, (uint64_t)g.nseg)) return rc;
    // first-try capacities: every batch at least a header, every record at
    // least 7 bytes (length, attributes, three deltas/lengths, header count),
    // decode up to 4x; a group that overflows is re-run
    const uint64_t bneed = g.bytes / RPGPU_HEADER_SIZE + 1;
    if (int rc = slot_grow<rpgpu_batch_result>(c, h.d_batches, bneed)) return rc;
    if (job->flags & RPGPU_JOB_PARSE)
        if (int rc = slot_grow<rpgpu_record_index>(c, h.d_records, g.bytes / 7 + 1)) return rc;
    if (job->flags & RPGPU_JOB_DECODE)
        if (int rc = slot_grow<uint8_t>(c, h.d_decoded, 4 * g.bytes + 4096)) return rc;
    h.h_offs.assign(g.nseg + 1, 0);
    for (uint32_t i = 0; i < g.nseg; i++) h.h_offs[i + 1] = h.h_offs[i] + job->seg_sizes[g.seg0 + i];
    for (uint32_t i = 0; i < g.nseg; i++)
        if (job->seg_sizes[g.seg0 + i])
            HIPCHK(c, hipMemcpyAsync(h.d_data.as<uint8_t>() + h.h_offs[i], job->segments[g.seg0 + i],
                                     job->seg_sizes[g.seg0 + i], hipMemcpyHostToDevice, c->copy));
    HIPCHK(c, hipMemcpyAsync(h.d_offs.p, h.h_offs.data(), (g.nseg + 1) * 8, hipMemcpyHostToDevice, c->copy));
    HIPCHK(c, hipEventRecord(h.h2d, c->copy));
    HIPCHK(c, hipStreamWaitEvent(c->stream, h.h2d, 0));
    const uint64_t bcap = count<rpgpu_batch_result>(h.d_batches);
    rpgpu_job j{};
    j.d_data = h.d_data.as<uint8_t>();
    j.d_seg_offsets = h.d_offs.as<uint64_t>();
    j.h_seg_offsets = h.h_offs.data();
    j.n_segments = g.nseg;
    j.layout = job->layout;
    j.flags = job->flags;
    j.d_batches = h.d_batches.as<rpgpu_batch_result>();
    j.batch_capacity = bcap;
    j.d_records = h.d_records.as<rpgpu_record_index>();
    j.record_capacity = (job->flags & RPGPU_JOB_PARSE) ? count<rpgpu_record_index>(h.d_records) : 0;
    j.d_decoded = h.d_decoded.as<uint8_t>();
    j.decoded_capacity = (job->flags & RPGPU_JOB_DECODE) ? h.d_decoded.bytes : 0;
    j.d_summaries = h.d_sums.as<rpgpu_segment_summary>();
    j.d_totals = h.d_tot.as<rpgpu_job_totals>();
    if (int rc = rpgpu_submit(c, &j, c->stream)) return rc;
    if (job->index_step && job->layout == RPGPU_LAYOUT_DISK) {
        // segment_index::maybe_track over the group's crc-good prefixes
        // (storage/log_replayer.cc:62-74), base offsets from the caller
        if (int rc = slot_grow<rpgpu_index_state>(c, h.d_ist, (uint64_t)g.nseg)) return rc;
        if (int rc = slot_grow<uint32_t>(c, h.d_ro, bcap)) return rc;
        if (int rc = slot_grow<uint32_t>(c, h.d_rt, bcap)) return rc;
        if (int rc = slot_grow<uint64_t>(c, h.d_ps, bcap)) return rc;
        h.h_ist.assign(g.nseg, rpgpu_index_state{});
        for (uint32_t i = 0; i < g.nseg; i++) h.h_ist[i].base_offset = job->index_states[g.seg0 + i].base_offset;
        HIPCHK(c, hipMemcpyAsync(h.d_ist.p, h.h_ist.data(), g.nseg * sizeof(rpgpu_index_state), hipMemcpyHostToDevice,
                                 c->stream));
        if (int rc = rpgpu_segment_index(c, j.d_batches, bcap, j.d_summaries, g.nseg, job->index_step,
                                         h.d_ist.as<rpgpu_index_state>(), h.d_ro.as<uint32_t>(), h.d_rt.as<uint32_t>(),
                                         h.d_ps.as<uint64_t>(), c->stream))
            return rc;
    }
    HIPCHK(c, hipMemcpyAsync(h.h_tot.p, h.d_tot.p, sizeof(rpgpu_job_totals), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(h.done, c->stream));
    return RPGPU_OK;
}
}  // namespace

extern "C" {

int rpgpu_validate_host(rpgpu_ctx* c, const rpgpu_host_job* job) {
    if (!c || !job || (job->n_segments && (!job->segments || !job->seg_sizes)) || !job->totals ||
        (job->n_segments && !job->summaries) || (job->batch_capacity && !job->batches) ||
        (job->record_capacity && !job->records) || (job->decoded_capacity && !job->decoded) ||
        (job->index_step && (!job->index_states || (job->batch_capacity && (!job->rel_offset || !job->rel_time ||
                                                                             !job->position)))))
        return fail(c, RPGPU_E_INVALID, "rpgpu_validate_host: missing argument");
    if (job->index_step >= (1ull << 62)) return fail(c, RPGPU_E_INVALID, "rpgpu_validate_host: index step out of range");
    if (job->layout != RPGPU_LAYOUT_DISK && job->layout != RPGPU_LAYOUT_WIRE)
        return fail(c, RPGPU_E_INVALID, "rpgpu_validate_host: unknown layout");
    hipSetDevice(c->device);
    std::memset(job->totals, 0, sizeof(rpgpu_job_totals));
    if (job->n_segments == 0) return RPGPU_OK;
    if (!c->copy) HIPCHK(c, hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
    for (auto& h : c->hs) {
        if (!h.h2d) HIPCHK(c, hipEventCreateWithFlags(&h.h2d, hipEventDisableTiming));
        if (!h.done) HIPCHK(c, hipEventCreateWithFlags(&h.done, hipEventDisableTiming));
        if (int rc = slot_grow<rpgpu_job_totals>(c, h.h_tot, 1)) return rc;
        if (int rc = slot_grow<rpgpu_job_totals>(c, h.d_tot, 1)) return rc;
    }
    std::vector<HostGroup> groups;
    const uint64_t gbytes = host_group_bytes(job);
    for (uint32_t i = 0; i < job->n_segments; i++) {
        const uint64_t sz = job->seg_sizes[i];
        if (!job->segments[i] && sz) return fail(c, RPGPU_E_INVALID, "rpgpu_validate_host: null segment");
        if (groups.empty() || groups.back().bytes + sz > gbytes) groups.push_back({i, 0, 0});
        groups.back().nseg++;
        groups.back().bytes += sz;
    }
    rpgpu_job_totals& T = *job->totals;
    uint64_t out_b = 0;
    // collect group gi (slot h): its totals, re-run on overflow, then the
    // batch results and summaries into the caller's arrays
    auto finish = [&](size_t gi) -> int {
        auto& h = c->hs[gi & 1];
        const HostGroup& g = groups[gi];
        HIPCHK(c, hipEventSynchronize(h.done));
        const rpgpu_job_totals* h_tot = h.h_tot.as<rpgpu_job_totals>();
        for (int tries = 0; h_tot->overflow && tries < 2; tries++) {
            const rpgpu_job_totals t = *h_tot;
            if (int rc = slot_grow<rpgpu_batch_result>(c, h.d_batches, t.batch_capacity_needed)) return rc;
            if (job->flags & RPGPU_JOB_PARSE)
                if (int rc = slot_grow<rpgpu_record_index>(c, h.d_records, t.record_capacity_needed)) return rc;
            if (job->flags & RPGPU_JOB_DECODE)
                if (int rc = slot_grow<uint8_t>(c, h.d_decoded, t.decoded_capacity_needed)) return rc;
            if (int rc = host_issue(c, h, job, g)) return rc;
            HIPCHK(c, hipEventSynchronize(h.done));
        }
        const rpgpu_job_totals t = *h_tot;
        const uint64_t nb = t.n_batches;
        const uint64_t room = job->batch_capacity > out_b ? job->batch_capacity - out_b : 0;
        const uint64_t take = std::min(nb, room);
        // this group's positions in the job: its records and decoded bytes
        // follow the earlier groups' (the index slots and arena bytes one
        // rpgpu_submit over every segment would have reserved before them)
        const uint64_t rec_base = T.n_records, dec_base = T.decoded_bytes;
        const uint64_t nrec = (job->flags & RPGPU_JOB_PARSE) ? t.n_records : 0;
        const uint64_t ndec = (job->flags & RPGPU_JOB_DECODE) ? t.decoded_bytes : 0;
        const uint64_t rroom = job->record_capacity > rec_base ? job->record_capacity - rec_base : 0;
        const uint64_t droom = job->decoded_capacity > dec_base ? job->decoded_capacity - dec_base : 0;
        const uint64_t rtake = job->records ? std::min(nrec, rroom) : 0;
        const uint64_t dtake = job->decoded ? std::min(ndec, droom) : 0;
        const bool ix = job->index_step && job->layout == RPGPU_LAYOUT_DISK;
        // results back on the copy stream: the compute stream already holds
        // the next group's pipeline, which must not be waited for here
        if (take) {
            HIPCHK(c, hipMemcpyAsync(job->batches + out_b, h.d_batches.p, take * sizeof(rpgpu_batch_result),
                                     hipMemcpyDeviceToHost, c->copy));
            if (ix) {
                HIPCHK(c, hipMemcpyAsync(job->rel_offset + out_b, h.d_ro.p, take * 4, hipMemcpyDeviceToHost, c->copy));
                HIPCHK(c, hipMemcpyAsync(job->rel_time + out_b, h.d_rt.p, take * 4, hipMemcpyDeviceToHost, c->copy));
                HIPCHK(c, hipMemcpyAsync(job->position + out_b, h.d_ps.p, take * 8, hipMemcpyDeviceToHost, c->copy));
            }
        }
        if (rtake)
            HIPCHK(c, hipMemcpyAsync(job->records + rec_base, h.d_records.p, rtake * sizeof(rpgpu_record_index),
                                     hipMemcpyDeviceToHost, c->copy));
        if (dtake) HIPCHK(c, hipMemcpyAsync(job->decoded + dec_base, h.d_decoded.p, dtake, hipMemcpyDeviceToHost, c->copy));
        HIPCHK(c, hipMemcpyAsync(job->summaries + g.seg0, h.d_sums.p, g.nseg * sizeof(rpgpu_segment_summary),
                                 hipMemcpyDeviceToHost, c->copy));
        if (ix)
            HIPCHK(c, hipMemcpyAsync(job->index_states + g.seg0, h.d_ist.p, g.nseg * sizeof(rpgpu_index_state),
                                     hipMemcpyDeviceToHost, c->copy));
        HIPCHK(c, hipStreamSynchronize(c->copy));
        // group-relative -> job-wide ordinals and positions
        for (uint64_t i = 0; i < take; i++) {
            rpgpu_batch_result& r = job->batches[out_b + i];
            r.segment += g.seg0;
            r.index_base += rec_base;
            r.decoded_off += dec_base;
        }
        for (uint64_t i = 0; i < rtake; i++) job->records[rec_base + i].batch += (uint32_t)out_b;
        for (uint32_t i = 0; i < g.nseg; i++) job->summaries[g.seg0 + i].first_batch += out_b;
        if (ix)
            for (uint32_t i = 0; i < g.nseg; i++) job->index_states[g.seg0 + i].first_entry += out_b;
        if (nrec > rtake && job->records) T.overflow |= 2u;
        if (ndec > dtake && job->decoded) T.overflow |= 4u;
        T.n_batches += nb;
        T.n_records += t.n_records;
        T.decoded_bytes += t.decoded_bytes;
        T.n_rewalks += t.n_rewalks;
        T.record_capacity_needed += t.record_capacity_needed;
        T.decoded_capacity_needed += t.decoded_capacity_needed;
        T.overflow |= t.overflow;
        if (nb > room) T.overflow |= 1u;
        out_b += nb;
        return RPGPU_OK;
    };
    // issue(g) before finish(g - 1): group g's copy and pipeline are queued
    // while g - 1's results come back; issue(g + 1) reuses g - 1's slot
    for (size_t gi = 0; gi < groups.size(); gi++) {
        if (int rc = host_issue(c, c->hs[gi & 1], job, groups[gi])) return rc;
        if (gi) if (int rc = finish(gi - 1)) return rc;
    }
    if (int rc = finish(groups.size() - 1)) return rc;
    T.batch_capacity_needed = T.n_batches;
    return RPGPU_OK;
}

uint64_t rpgpu_uncompress_bound(int codec, const void* in, size_t n) {
    if (!in || n == 0 || (codec != RPGPU_CODEC_LZ4 && codec != RPGPU_CODEC_SNAPPY)) return 0;
    return decode_capacity_dev(codec, (const uint8_t*)in, n);
}

int rpgpu_stamp_host(rpgpu_ctx* c, uint8_t* buf, size_t len, const uint64_t* pos, const uint32_t* payload_len,
                     uint32_t n, int64_t next_offset, uint32_t flags) {
    if (!c) return RPGPU_E_INVALID;
    if (n == 0) return RPGPU_OK;
    if (!buf || !pos || ((flags & RPGPU_STAMP_CRC) && !payload_len))
        return fail(c, RPGPU_E_INVALID, "rpgpu_stamp_host: missing argument");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    // device: [batches + 16][pos][plen]; host (pinned): the same
    const size_t o_pos = align_up(len + 16, 256), o_len = align_up(o_pos + (size_t)n * 8, 256);
    const size_t total = align_up(o_len + (size_t)n * 4, 256);
    if (int rc = grow(c, c->std_, total, s, "stamp staging")) return rc;
    if (int rc = grow(c, c->sth, total, s, "stamp pinned staging")) return rc;
    uint8_t* h = c->sth.as<uint8_t>();
    uint8_t* d = c->std_.as<uint8_t>();
    std::memcpy(h, buf, len);
    std::memset(h + len, 0, 16);
    std::memcpy(h + o_pos, pos, (size_t)n * 8);
    if (payload_len) std::memcpy(h + o_len, payload_len, (size_t)n * 4);
    HIPCHK(c, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, s));
    if (int rc = rpgpu_stamp(c, d, (const uint64_t*)(d + o_pos), payload_len ? (const uint32_t*)(d + o_len) : nullptr, n,
                             next_offset, flags, s))
        return rc;
    HIPCHK(c, hipMemcpyAsync(h, d, len, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(buf, h, len);
    return RPGPU_OK;
}

}  // extern "C"
