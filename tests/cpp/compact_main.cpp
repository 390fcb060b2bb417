// Driver of storage::internal::compact_segment (include/rpgpu_redpanda.h):
//   compact_test <segment file> <output file>
// writes the compacted segment to the output file and prints
//   kept <offset>...      the surviving record offsets
//   codecs <codec>...     per output batch, its codec before compaction
//   stats <records_in> <records_kept> <batches_in> <batches_out> <batches_rewritten> <bytes_out>
// or `error <what>` (exit status 2) where compact_segment throws.
#include <cstdio>
#include <exception>
#include <fstream>
#include <iterator>
#include <vector>

#include "rpgpu_redpanda.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <segment file> <output file>\n", argv[0]);
        return 1;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 1;
    }
    const std::vector<char> seg((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    try {
        const auto r = storage::internal::compact_segment(reinterpret_cast<const uint8_t*>(seg.data()), seg.size());
        std::ofstream out(argv[2], std::ios::binary);
        out.write(reinterpret_cast<const char*>(r.bytes.data()), (std::streamsize)r.bytes.size());
        if (!out) {
            std::fprintf(stderr, "cannot write %s\n", argv[2]);
            return 1;
        }
        std::printf("kept");
        for (int64_t o : r.kept_offsets) std::printf(" %lld", (long long)o);
        std::printf("\ncodecs");
        for (auto c : r.codecs) std::printf(" %d", (int)c);
        std::printf("\nstats %llu %llu %llu %llu %llu %llu\n", (unsigned long long)r.stats.records_in,
                    (unsigned long long)r.stats.records_kept, (unsigned long long)r.stats.batches_in,
                    (unsigned long long)r.stats.batches_out, (unsigned long long)r.stats.batches_rewritten,
                    (unsigned long long)r.stats.bytes_out);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
