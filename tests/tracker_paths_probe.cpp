// Stand-alone reader of csrc/tracker_paths.hpp (its own main, only that header, no HIP and no
// libecc).  Commands:
//   consts                 name=value lines of every switch point
//   floor_div a b [a b …]  one quotient per line
//   bucket cx cy [cx cy …] one bucket per line
//   grid MD_BITS […]       "grid_ok cell reach_bits" per max_distance (a float bit pattern, hex)
//   lanes T GRID […]       "L lists_ok" of tracker_kernel per (T, use_grid)
//   fast T C […]           "lane_shift chunk" of tracker_fast_kernel per (T, C)
//   span                   the 3-cell property, swept (see below): "OK checked=N"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tracker_paths.hpp"

using namespace trk_paths;

static float from_bits(const char *s) {
    const uint32_t b = (uint32_t)std::strtoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

// The cells tracker_kernel's grid visitor walks on one axis for a prediction coordinate p
// (grid_cell_lo / grid_cell_hi are the kernel's own).
static int cells_spanned(float p, float reach, int cell) {
    return grid_cell_hi(p, reach, cell) - grid_cell_lo(p, reach, cell) + 1;
}

// Every max_distance of the sweep, every prediction coordinate around every cell border near a few
// bases (the int16 ends, the origin, a negative and a positive far base): at most 3 cells, and the
// cell of every integer coordinate q with |q - p| < max_distance is among them.
static int span_sweep() {
    unsigned long long checked = 0;
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    const float bases[] = {0.f, -32768.f, 32767.f, -100000.f, 250000.f, -7.f};
    for (int k = 0; k < 60000; ++k) {
        float md;
        if (k <= 4000) md = (float)k * 0.25f;                                 // 0 .. 1000 in quarters
        else if (k <= 8000) md = std::nextafterf((float)(k - 4000), k & 1 ? 0.f : 1.0e9f);  // beside integers
        else if (k == 8001) md = std::nextafterf(1.0e5f, 0.f);
        else {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            md = (float)((lcg >> 11) * (1.0 / 9007199254740992.0) * 1.0e5);
            if (!(md < 1.0e5f)) md = 99999.f;
        }
        if (!grid_ok(md)) { std::printf("FAIL grid_ok md=%a\n", md); return 1; }
        const float reach = grid_reach(md);
        const int cell = grid_cell(md);
        if (cell < 2) { std::printf("FAIL cell md=%a cell=%d\n", md, cell); return 1; }
        for (float base : bases) {
            const float border = (float)(floor_div((int)base, cell) * cell);
            for (int side = -1; side <= 1; ++side)
                for (int j = -6; j <= 6; ++j) {
                    // predictions whose box ends sit on and beside a cell border
                    const float p = border + (float)side * reach + (float)j * 0.25f;
                    ++checked;
                    const int n = cells_spanned(p, reach, cell);
                    if (n < 1 || n > 3) { std::printf("FAIL span md=%a p=%a cells=%d\n", md, p, n); return 1; }
                    // an integer q with |q - p| < max_distance lies in a walked cell
                    const int q0 = (int)ceilf(p - md), q1 = (int)floorf(p + md);
                    if (q0 <= q1 && (floor_div(q0, cell) < grid_cell_lo(p, reach, cell) ||
                                     floor_div(q1, cell) > grid_cell_hi(p, reach, cell))) {
                        std::printf("FAIL reach md=%a p=%a\n", md, p);
                        return 1;
                    }
                }
        }
    }
    std::printf("OK checked=%llu\n", checked);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const char *c = argv[1];
    if (!std::strcmp(c, "consts")) {
        std::printf("kFT=%d\nkFThreads=%d\nkFList=%d\nkFTailTracks=%d\nkFLaneShiftT=%d\nkFChunkNarrow=%d\nkFChunkWide=%d\n",
                    kFT, kFThreads, kFList, kFTailTracks, kFLaneShiftT, kFChunkNarrow, kFChunkWide);
        std::printf("kNT=%d\nkBuckets=%d\nkBrute=%d\nkLaneList=%d\nkTailCap=%d\nkTailTracks=%d\nkLanesMax=%d\nkGroupWave=%d\n",
                    kNT, kBuckets, kBrute, kLaneList, kTailCap, kTailTracks, kLanesMax, kGroupWave);
        return 0;
    }
    if (!std::strcmp(c, "span")) return span_sweep();
    const bool pairs = !std::strcmp(c, "floor_div") || !std::strcmp(c, "bucket") || !std::strcmp(c, "lanes") ||
                       !std::strcmp(c, "fast");
    if (pairs) {
        if ((argc - 2) % 2) return 2;
        for (int k = 2; k + 1 < argc; k += 2) {
            const int a = std::atoi(argv[k]), b = std::atoi(argv[k + 1]);
            if (c[0] == 'f' && c[1] == 'l') {
                if (b <= 0) return 2;
                std::printf("%d\n", floor_div(a, b));
            } else if (c[0] == 'b') {
                std::printf("%d\n", cell_bucket(a, b));
            } else if (c[0] == 'l') {
                const int L = general_lanes(a, b != 0);
                std::printf("%d %d\n", L, lists_ok(a, L) ? 1 : 0);
            } else {
                const int sh = fast_lane_shift(a);
                std::printf("%d %d\n", sh, fast_chunk_narrow(b, 1 << sh) ? kFChunkNarrow : kFChunkWide);
            }
        }
        return 0;
    }
    if (!std::strcmp(c, "grid")) {
        for (int k = 2; k < argc; ++k) {
            const float md = from_bits(argv[k]);
            std::printf("%d %d %08x\n", grid_ok(md) ? 1 : 0, grid_cell(md), bits_of(grid_reach(md)));
        }
        return 0;
    }
    return 2;
}
