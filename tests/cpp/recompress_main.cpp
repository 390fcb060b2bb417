// Driver of storage::internal::compact_segment with recompress_options
// (include/rpgpu_redpanda.h):
//   recompress_test <segment file> <output file> [codec [min_batch_bytes [snappy_frag]]]
// (codec: an rpgpu_codec value, or -1 for every batch's source codec) writes
// the on-disk compacted segment to the output file and prints
//   kept <offset>...      the surviving record offsets
//   batches <out_pos>:<payload_len>:<codec>:<flags>...   per output batch
//   stats <records_in> <records_kept> <batches_in> <batches_out> <batches_rewritten>
//   recompress <batches_compressed> <batches_host> <bytes_out of the device call>
//   index <base_offset> <max_offset> <base_timestamp> <max_timestamp> <entries>
//   entry <relative_offset> <relative_time> <position>     per index entry
// or `error <what>` (exit status 2) where compact_segment throws.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <iterator>
#include <vector>

#include "rpgpu_redpanda.h"

int main(int argc, char** argv) {
    if (argc < 3 || argc > 6) {
        std::fprintf(stderr, "usage: %s <segment file> <output file> [codec [min_batch_bytes [snappy_frag]]]\n", argv[0]);
        return 1;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 1;
    }
    const std::vector<char> seg((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    storage::internal::recompress_options opt;
    if (argc > 3 && std::atoi(argv[3]) >= 0) opt.codec = (uint32_t)std::atoi(argv[3]);
    if (argc > 4) opt.min_batch_bytes = std::strtoull(argv[4], nullptr, 10);
    if (argc > 5) opt.snappy_frag = std::strtoull(argv[5], nullptr, 10);
    try {
        const auto r = storage::internal::compact_segment(reinterpret_cast<const uint8_t*>(seg.data()), seg.size(), opt);
        std::ofstream out(argv[2], std::ios::binary);
        out.write(reinterpret_cast<const char*>(r.bytes.data()), (std::streamsize)r.bytes.size());
        if (!out) {
            std::fprintf(stderr, "cannot write %s\n", argv[2]);
            return 1;
        }
        std::printf("kept");
        for (int64_t o : r.kept_offsets) std::printf(" %lld", (long long)o);
        std::printf("\nbatches");
        for (const auto& b : r.batches)
            std::printf(" %llu:%u:%u:%u", (unsigned long long)b.out_pos, b.payload_len, b.codec, b.flags);
        std::printf("\nstats %llu %llu %llu %llu %llu\n", (unsigned long long)r.stats.records_in,
                    (unsigned long long)r.stats.records_kept, (unsigned long long)r.stats.batches_in,
                    (unsigned long long)r.stats.batches_out, (unsigned long long)r.stats.batches_rewritten);
        std::printf("recompress %llu %llu %llu\n", (unsigned long long)r.recompress.batches_compressed,
                    (unsigned long long)r.recompress.batches_host, (unsigned long long)r.recompress.bytes_out);
        const auto& x = r.index;
        std::printf("index %lld %lld %lld %lld %zu\n", (long long)x.base_offset, (long long)x.max_offset,
                    (long long)x.base_timestamp, (long long)x.max_timestamp, x.relative_offset_index.size());
        for (size_t i = 0; i < x.relative_offset_index.size(); i++)
            std::printf("entry %u %u %llu\n", x.relative_offset_index[i], x.relative_time_index[i],
                        (unsigned long long)x.position_index[i]);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
