// Driver of kafka::read_from_partitions and storage::timequery
// (include/rpgpu_redpanda.h):
//   fetch_test <request file> <output file> [--index]
//   fetch_test <request file> --timequery <time> <max offset>
// The request file holds, little-endian: u32 n, then per partition its
// rpgpu_fetch_request (40 bytes), u32 segments, and per segment u64 length and
// the segment's bytes.  The first form writes the partitions' record sets back
// to back to the output file and prints, per partition,
//   part <record_count> <base_offset> <last_offset> <next_offset> <over_budget> <bytes>
// or `error <what>` (exit status 2) where read_from_partitions throws.  The
// second runs storage::timequery over the first partition's segments and
// prints `timequery <offset> <time>` or `timequery none`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "rpgpu_redpanda.h"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <request file> <output file> [--index] | <request file> --timequery <time> <max>\n",
                     argv[0]);
        return 1;
    }
    const bool tq = std::string(argv[2]) == "--timequery";
    if (tq && argc < 5) {
        std::fprintf(stderr, "--timequery needs <time> <max offset>\n");
        return 1;
    }
    const bool use_index = !tq && argc > 3 && std::string(argv[3]) == "--index";
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 1;
    }
    const std::vector<char> req((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    auto take = [&](void* dst, size_t n) {
        if (req.size() - pos < n) return false;
        std::memcpy(dst, req.data() + pos, n);
        pos += n;
        return true;
    };
    auto short_file = [] {
        std::fprintf(stderr, "short request file\n");
        return 1;
    };
    uint32_t n = 0;
    if (!take(&n, 4)) return short_file();
    std::vector<std::vector<rpgpu::iobuf>> parts;
    std::vector<storage::log_reader_config> configs;
    for (uint32_t i = 0; i < n; i++) {
        rpgpu_fetch_request q;
        uint32_t nseg = 0;
        if (!take(&q, sizeof q) || !take(&nseg, 4)) return short_file();
        storage::log_reader_config g(q.start_offset, q.max_offset, 0, (size_t)q.max_bytes, storage::io_priority_class{},
                                     (q.flags & RPGPU_FETCH_TYPE_FILTER) ? std::optional<int8_t>(q.type_filter) : std::nullopt,
                                     (q.flags & RPGPU_FETCH_FIRST_TIMESTAMP) ? std::optional<int64_t>(q.first_timestamp)
                                                                              : std::nullopt,
                                     std::nullopt);
        g.strict_max_bytes = (q.flags & RPGPU_FETCH_STRICT_MAX_BYTES) != 0;
        configs.push_back(g);
        parts.emplace_back();
        for (uint32_t s = 0; s < nseg; s++) {
            uint64_t len = 0;
            if (!take(&len, 8) || req.size() - pos < len) return short_file();
            parts.back().emplace_back(reinterpret_cast<const uint8_t*>(req.data()) + pos, (size_t)len);
            pos += (size_t)len;
        }
    }
    try {
        if (tq) {
            const auto r = storage::timequery(parts.empty() ? std::vector<rpgpu::iobuf>{} : parts[0],
                                              std::strtoll(argv[3], nullptr, 10), std::strtoll(argv[4], nullptr, 10));
            if (r) std::printf("timequery %lld %lld\n", (long long)r->offset, (long long)r->time);
            else std::printf("timequery none\n");
            return 0;
        }
        const auto res = kafka::read_from_partitions(parts, configs, use_index);
        std::ofstream out(argv[2], std::ios::binary);
        for (const auto& p : res) {
            out.write(reinterpret_cast<const char*>(p.data.data()), (std::streamsize)p.data.size_bytes());
            std::printf("part %u %lld %lld %lld %d %zu\n", p.record_count, (long long)p.base_offset, (long long)p.last_offset,
                        (long long)p.next_offset, p.over_budget ? 1 : 0, p.data.size_bytes());
        }
        if (!out) {
            std::fprintf(stderr, "cannot write %s\n", argv[2]);
            return 1;
        }
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
