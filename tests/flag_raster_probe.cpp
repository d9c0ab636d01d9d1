// Stand-alone check of csrc/flag_raster.hpp (its own main, only that header and the two it
// includes, no HIP and no libecc): the flag pass's raster corner bitmap.
//   * the lookup: for every pair (x, y) in [0, 65535]^2 and each sensor size given on the command
//     line (default: 346x260, 33x29, 64x28, 1280x720, 65536x9) flag_raster_index stays at or below
//     W * H - 1, hence inside the flag_raster_words(W, H) words of the bitmap, (65535, 65535)
//     included, and on the sensor it is y * W + x;
//   * the staging map: for every tile and every lp < 196, the pixel that flag_stage_word and
//     flag_stage_pixel compute from (word index tile * 7 + lp / 32, bit lp % 32) is the tile's
//     origin plus (lp % 14, lp / 14), with `set` exactly where that pixel is on the sensor (tiles
//     cut by the right and bottom edges set nothing past them); bits 4..31 of a tile's seventh
//     word (lp >= 196) set nothing; every on-sensor pixel is reached exactly once.
// The host form of ECC_UMUL24 multiplies the operands' low 24 bits, as v_mul_u32_u24 does, so a
// product that would lose bits on the device loses them here.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "flag_raster.hpp"

struct Sensor {
    uint32_t W, H;
};

static std::atomic<uint64_t> g_bad{0}, g_on{0}, g_staged{0};

static void fail(const char *what, uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t got, uint32_t want) {
    if (g_bad.fetch_add(1) < 10)
        std::printf("FAIL %s: sensor %ux%u, (x, y) = (%u, %u): got %u, want %u\n", what, W, H, x, y, got, want);
}

static void rows(const Sensor s, uint32_t y0, uint32_t y1) {
    const uint32_t last_bit = s.W * s.H - 1, words = flag_raster_words(s.W, s.H);
    uint64_t on = 0;
    for (uint32_t y = y0; y < y1; ++y)
        for (uint32_t x = 0; x < 65536; ++x) {
            const uint32_t i = flag_raster_index(x, y, s.W, last_bit);
            if (i > last_bit || (i >> 5) >= words) fail("index out of the bitmap", s.W, s.H, x, y, i, last_bit);
            if (x < s.W && y < s.H) {
                ++on;
                if (i != y * s.W + x) fail("index", s.W, s.H, x, y, i, y * s.W + x);
            }
        }
    g_on += on;
}

static void staging(const Sensor s) {
    const uint32_t tiles_x = (s.W + 13) / 14, tiles_y = (s.H + 13) / 14;
    const MagicDiv md = magic_div31(tiles_x);
    std::vector<uint8_t> hit((size_t)s.W * s.H, 0);
    uint64_t staged = 0;
    for (uint32_t tile = 0; tile < tiles_x * tiles_y; ++tile)
        for (uint32_t lp = 0; lp < 224; ++lp) {
            const uint32_t i = tile * 7 + lp / 32, b = lp % 32;
            const FlagStageWord sw = flag_stage_word(i, tiles_x, md.mul, md.sh);
            const FlagStagePixel px = flag_stage_pixel(sw, b, s.W, s.H);
            if (lp >= 196) {
                if (px.set) fail("padding bit sets a pixel", s.W, s.H, tile, lp, px.set, 0);
                continue;
            }
            const uint32_t x = (tile % tiles_x) * 14 + lp % 14, y = (tile / tiles_x) * 14 + lp / 14;
            if (px.x != x) fail("stage x (tile, lp)", s.W, s.H, tile, lp, px.x, x);
            if (px.y != y) fail("stage y (tile, lp)", s.W, s.H, tile, lp, px.y, y);
            const uint32_t inside = (x < s.W && y < s.H) ? 1u : 0u;
            if (px.set != inside) fail("stage set (tile, lp)", s.W, s.H, tile, lp, px.set, inside);
            if (px.set && inside) {
                // the bit staged for the pixel is the bit an event at the pixel reads
                const uint32_t idx = ECC_UMUL24(px.y, s.W) + px.x;
                if (idx != flag_raster_index(x, y, s.W, s.W * s.H - 1)) fail("stage bit", s.W, s.H, x, y, idx, y * s.W + x);
                if (hit[(size_t)y * s.W + x]++) fail("pixel staged twice", s.W, s.H, x, y, 2, 1);
                ++staged;
            }
        }
    g_staged += staged;
}

int main(int argc, char **argv) {
    std::vector<Sensor> sensors;
    for (int i = 1; i + 1 < argc; i += 2) sensors.push_back({(uint32_t)std::atoi(argv[i]), (uint32_t)std::atoi(argv[i + 1])});
    if (sensors.empty()) sensors = {{346, 260}, {33, 29}, {64, 28}, {1280, 720}, {65536, 9}};
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    uint64_t expect_on = 0;
    for (const Sensor s : sensors) {
        if (s.W < 1 || s.W > 65536 || s.H < 1 || s.H > 65536 || ((s.W + 13) / 14) * ((s.H + 13) / 14) > 8191) {
            std::printf("FAIL sensor %ux%u: outside the corner detector's range (at most 8191 tiles)\n", s.W, s.H);
            return 1;
        }
        if (flag_raster_words(s.W, s.H) > ((s.W + 13) / 14) * ((s.H + 13) / 14) * 7) {
            std::printf("FAIL sensor %ux%u: the raster bitmap is larger than the tile segments\n", s.W, s.H);
            return 1;
        }
        expect_on += (uint64_t)s.W * s.H;
        staging(s);
        std::vector<std::thread> th;
        for (unsigned i = 0; i < nt; ++i)
            th.emplace_back(rows, s, (uint32_t)(65536ull * i / nt), (uint32_t)(65536ull * (i + 1) / nt));
        for (auto &t : th) t.join();
    }
    const bool ok = g_bad == 0 && g_on == expect_on && g_staged == expect_on;
    std::printf("%s sensors=%zu on_sensor=%llu staged=%llu bad=%llu\n", ok ? "OK" : "FAILED", sensors.size(),
                (unsigned long long)g_on.load(), (unsigned long long)g_staged.load(), (unsigned long long)g_bad.load());
    return ok ? 0 : 1;
}
