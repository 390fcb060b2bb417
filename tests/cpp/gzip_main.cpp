// Driver of storage::internal::compact_segment with
// recompress_options::device_gzip (include/rpgpu_redpanda.h):
//   gzip_test <segment file> <output file> <device_gzip: 0 | 1>
// writes the on-disk compacted segment to the output file and prints
//   batches <out_pos>:<payload_len>:<codec>:<flags>...   per output batch
//   recompress <batches_compressed> <batches_host> <bytes_out of the device call>
//   device_payloads <gzip payloads rpgpu_compress_batch deflated on the device>
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
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <segment file> <output file> <device_gzip: 0 | 1>\n", argv[0]);
        return 1;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 1;
    }
    const std::vector<char> seg((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    storage::internal::recompress_options opt;
    opt.device_gzip = std::atoi(argv[3]) != 0;
    try {
        const auto r = storage::internal::compact_segment(reinterpret_cast<const uint8_t*>(seg.data()), seg.size(), opt);
        std::ofstream out(argv[2], std::ios::binary);
        out.write(reinterpret_cast<const char*>(r.bytes.data()), (std::streamsize)r.bytes.size());
        if (!out) {
            std::fprintf(stderr, "cannot write %s\n", argv[2]);
            return 1;
        }
        std::printf("batches");
        for (const auto& b : r.batches)
            std::printf(" %llu:%u:%u:%u", (unsigned long long)b.out_pos, b.payload_len, b.codec, b.flags);
        std::printf("\nrecompress %llu %llu %llu\n", (unsigned long long)r.recompress.batches_compressed,
                    (unsigned long long)r.recompress.batches_host, (unsigned long long)r.recompress.bytes_out);
        // a host pass with the switch on would show here: compress_batch takes the same context
        uint64_t dev = 0;
        rpgpu_gzip_device_payloads(rpgpu::engine::local().ctx(), &dev);
        std::printf("device_payloads %llu\n", (unsigned long long)dev);
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
