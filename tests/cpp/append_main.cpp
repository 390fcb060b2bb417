// Driver of kafka::produce_append (include/rpgpu_redpanda.h):
//   append_test <request file> <output file> [--all]
// The request file holds, little-endian: u32 n, then per record set
// i64 next_offset, i64 append_time (INT64_MIN: create time), u64 length and
// the set's bytes.  Writes the partitions' log bytes back to back to the
// output file and prints, per partition,
//   set <error_code> <status> <base_offset> <last_offset> <log bytes>
// or `error <what>` (exit status 2) where produce_append throws.
// --all: every batch of a set instead of the produce rule's first one.
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "rpgpu_redpanda.h"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <request file> <output file> [--all]\n", argv[0]);
        return 1;
    }
    const bool all = argc > 3 && std::string(argv[3]) == "--all";
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
    uint32_t n = 0;
    if (!take(&n, 4)) {
        std::fprintf(stderr, "short request file\n");
        return 1;
    }
    std::vector<rpgpu::iobuf> sets;
    std::vector<int64_t> next, times;
    for (uint32_t i = 0; i < n; i++) {
        int64_t nx = 0, at = 0;
        uint64_t len = 0;
        if (!take(&nx, 8) || !take(&at, 8) || !take(&len, 8) || req.size() - pos < len) {
            std::fprintf(stderr, "short request file\n");
            return 1;
        }
        sets.emplace_back(reinterpret_cast<const uint8_t*>(req.data()) + pos, (size_t)len);
        pos += (size_t)len;
        next.push_back(nx);
        times.push_back(at);
    }
    try {
        const auto res = kafka::produce_append(sets, next, times, rpgpu::engine::local(), all);
        std::ofstream out(argv[2], std::ios::binary);
        for (const auto& p : res) {
            out.write(reinterpret_cast<const char*>(p.log_bytes.data()), (std::streamsize)p.log_bytes.size());
            std::printf("set %d %d %lld %lld %zu\n", (int)p.error, (int)p.status, (long long)p.base_offset,
                        (long long)p.last_offset, p.log_bytes.size());
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
