// Stand-alone run of rp_deflate_core.h for the sanitizers (TEST
// INFRASTRUCTURE ONLY): built with -fsanitize=address,undefined, it reads
// payload files, runs the core over each at several fragment sizes into an
// exactly deflateBound-sized heap buffer with an exactly kWorkBytes-sized
// work area, and prints length and a checksum per stream.
//   deflate_core_main FILE...
// The files are the named cases of tests/gzip_compress_corpus.py, written out
// by the caller ("gzip compression design", has the command).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../redpanda_amd/csrc/rp_deflate_core.h"

int main(int argc, char** argv) {
    static const uint64_t frags[] = {0, 1000, 4096, 65280, 65530};
    uint64_t streams = 0;
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> data;
        uint8_t chunk[65536];
        for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) data.insert(data.end(), chunk, chunk + k);
        fclose(f);
        // exact-size heap copies: an access past either end is reported
        uint8_t* src = (uint8_t*)malloc(data.size() ? data.size() : 1);
        for (size_t i = 0; i < data.size(); i++) src[i] = data[i];
        for (uint64_t frag : frags) {
            const uint64_t cap = rp::df::bound(data.size());
            uint8_t* out = (uint8_t*)malloc(cap);
            rp::df::Work* w = (rp::df::Work*)malloc(rp::df::kWorkBytes);
            const uint64_t n = rp::df::gzip(src, data.size(), frag, out, w);
            if (n > cap) { fprintf(stderr, "%s: %llu > bound %llu\n", argv[a], (unsigned long long)n, (unsigned long long)cap); return 1; }
            uint32_t sum = 0;
            for (uint64_t i = 0; i < n; i++) sum = sum * 31 + out[i];
            printf("%s frag %llu: %llu bytes, sum %08x\n", argv[a], (unsigned long long)frag, (unsigned long long)n, sum);
            free(w);
            free(out);
            streams++;
        }
        free(src);
    }
    printf("%llu streams ok\n", (unsigned long long)streams);
    return 0;
}
