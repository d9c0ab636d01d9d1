// ecc::RawFileReader on a recording in chunks of a given size: raw_reader_probe <in.raw> <chunk_words>
// <out.bin>.  Writes the decoded events as n (int64), xy[n] (u32), t[n] (i64), p[n] (u8) and prints
// the event count of every chunk.  Built by tests/test_gpu_evt21.py against lib/libecc.so.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ecc.hpp"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    try {
        ecc::Context &ctx = ecc::Context::default_context();
        ecc::RawFileReader rd(ctx, argv[1], std::atoll(argv[2]));
        std::vector<uint32_t> xy;
        std::vector<int64_t> t;
        std::vector<uint8_t> p;
        const uint32_t *dx;
        const int64_t *dt;
        const uint8_t *dp;
        for (int64_t n; (n = rd.next(&dx, &dt, &dp)) > 0;) {
            const size_t o = xy.size();
            xy.resize(o + n); t.resize(o + n); p.resize(o + n);
            if (ecc_memcpy_d2h(xy.data() + o, dx, (size_t)n * 4, ctx.stream()) ||
                ecc_memcpy_d2h(t.data() + o, dt, (size_t)n * 8, ctx.stream()) ||
                ecc_memcpy_d2h(p.data() + o, dp, (size_t)n, ctx.stream()))
                return 3;
            ctx.sync();
            std::printf("%lld\n", (long long)n);
        }
        FILE *f = std::fopen(argv[3], "wb");
        if (!f) return 4;
        const int64_t n = (int64_t)xy.size();
        std::fwrite(&n, 8, 1, f);
        std::fwrite(xy.data(), 4, xy.size(), f);
        std::fwrite(t.data(), 8, t.size(), f);
        std::fwrite(p.data(), 1, p.size(), f);
        std::fclose(f);
    } catch (const ecc::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
