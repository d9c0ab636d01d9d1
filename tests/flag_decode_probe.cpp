// Stand-alone check of csrc/flag_decode.hpp (its own main, only that header, no HIP and no libecc):
// the flag pass's map from an event to (word of the slice's result segments, bit), built from
// 24-bit multiplies and shifts, against the plain / 14, % 14 form.
//   * flag_div14(v) == v / 14 for every v in [0, 65535];
//   * for every pair (x, y) in [0, 65535]^2 and each sensor size given on the command line
//     (default: 346x260, 33x29, 1280x720, 65536x9): the word index is at most
//     n_tiles * 7 - 1 and the bit below 32, (65535, 65535) included; flag_on_sensor is x < W && y < H;
//     and on the sensor the word and the bit are those of
//     ((y / 14) * tiles_x + x / 14) * 7 + lp / 32 and lp % 32, lp = (y % 14) * 14 + x % 14.
// The host form of ECC_UMUL24 multiplies the operands' low 24 bits, as v_mul_u32_u24 does, so a
// product that would lose bits on the device loses them here.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "flag_decode.hpp"

struct Sensor {
    uint32_t W, H;
};

static std::atomic<uint64_t> g_bad{0}, g_on{0};

static void fail(const char *what, uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t got, uint32_t want) {
    if (g_bad.fetch_add(1) < 10)
        std::printf("FAIL %s: sensor %ux%u, (x, y) = (%u, %u): got %u, want %u\n", what, W, H, x, y, got, want);
}

static void rows(const Sensor s, uint32_t y0, uint32_t y1) {
    const uint32_t tiles_x = (s.W + 13) / 14, tiles_y = (s.H + 13) / 14;
    const uint32_t last_word = tiles_x * tiles_y * 7 - 1;
    uint64_t on = 0;
    for (uint32_t y = y0; y < y1; ++y)
        for (uint32_t x = 0; x < 65536; ++x) {
            const FlagSlot sl = flag_slot(x, y, tiles_x, last_word);
            if (sl.word > last_word) fail("word out of bounds", s.W, s.H, x, y, sl.word, last_word);
            if (sl.bit > 31) fail("bit out of range", s.W, s.H, x, y, sl.bit, 31);
            const uint32_t inside = (x < s.W && y < s.H) ? 1u : 0u;
            if (flag_on_sensor(x, y, s.W, s.H) != inside) fail("on_sensor", s.W, s.H, x, y, !inside, inside);
            if (!inside) continue;
            ++on;
            const uint32_t lp = (y % 14) * 14 + x % 14;
            const uint32_t word = ((y / 14) * tiles_x + x / 14) * 7 + lp / 32;
            if (sl.word != word) fail("word", s.W, s.H, x, y, sl.word, word);
            if (sl.bit != lp % 32) fail("bit", s.W, s.H, x, y, sl.bit, lp % 32);
        }
    g_on += on;
}

int main(int argc, char **argv) {
    std::vector<Sensor> sensors;
    for (int i = 1; i + 1 < argc; i += 2) sensors.push_back({(uint32_t)std::atoi(argv[i]), (uint32_t)std::atoi(argv[i + 1])});
    if (sensors.empty()) sensors = {{346, 260}, {33, 29}, {1280, 720}, {65536, 9}};
    for (uint32_t v = 0; v < 65536; ++v)
        if (flag_div14(v) != v / 14) fail("div14", 0, 0, v, 0, flag_div14(v), v / 14);
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    uint64_t expect_on = 0;
    for (const Sensor s : sensors) {
        if (s.W < 1 || s.W > 65536 || s.H < 1 || s.H > 65536 || ((s.W + 13) / 14) * ((s.H + 13) / 14) > 8191) {
            std::printf("FAIL sensor %ux%u: outside the corner detector's range (at most 8191 tiles)\n", s.W, s.H);
            return 1;
        }
        expect_on += (uint64_t)s.W * s.H;
        std::vector<std::thread> th;
        for (unsigned i = 0; i < nt; ++i)
            th.emplace_back(rows, s, (uint32_t)(65536ull * i / nt), (uint32_t)(65536ull * (i + 1) / nt));
        for (auto &t : th) t.join();
    }
    const bool ok = g_bad == 0 && g_on == expect_on;
    std::printf("%s sensors=%zu on_sensor=%llu bad=%llu\n", ok ? "OK" : "FAILED", sensors.size(),
                (unsigned long long)g_on.load(), (unsigned long long)g_bad.load());
    return ok ? 0 : 1;
}
