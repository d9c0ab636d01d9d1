// Stand-alone check of the compact value list's index arithmetic in csrc/arc_select.hpp (its own
// main, only that header, no HIP and no libecc): arc_below_mask, arc_value_byte and
// arc_value_byte_below, the byte of arc_kernel's value array that an event of slice j reads at a
// window pixel whose record is (mask, offset in bytes).
//   * arc_below_mask(j) has exactly bits 0 .. j, for every j in 0 .. 31 (j = 31: all ones);
//   * for every j in 0 .. 31, every mask of a set that holds the empty, the full, all single-bit,
//     all "bits 0 .. b" and "bits b .. 31" masks and 4096 random ones, and every word offset of
//     0, 1, the largest the kernel can produce (cap - 1, cap = kValCap + kWinPix given as argv[1])
//     and the largest a pixel with that mask can have (cap - 1 - popcount(mask): its run ends at
//     the array's last word): the byte is 4 * (off_words + popcount(mask & bits 0 .. j)), formed
//     here in 64 bits, and both entry points agree;
//   * wherever the record is one the kernel can write (off_words + popcount(mask) < cap: the pixel's
//     B_g slot and its values lie inside the array), the word read lies inside the array too; the
//     count of such lookups that read the array's LAST word is printed, and must not be zero.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "arc_select.hpp"

int main(int argc, char **argv) {
    const uint64_t cap = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4096 + 484;  // words of vals[]
    if (cap < 64 || cap > (1u << 20)) {
        std::printf("FAIL cap %llu\n", (unsigned long long)cap);
        return 1;
    }
    uint64_t bad = 0, checked = 0, inside = 0, last_word = 0;
    auto fail = [&](const char *what, uint32_t mask, int j, uint64_t off, uint64_t got, uint64_t want) {
        if (bad++ < 10)
            std::printf("FAIL %s: mask %08x, j %d, off_words %llu: got %llu, want %llu\n", what, mask, j,
                        (unsigned long long)off, (unsigned long long)got, (unsigned long long)want);
    };
    for (int j = 0; j < 32; ++j) {
        const uint64_t want = (1ull << (j + 1)) - 1ull;
        if (arc_below_mask(j) != (uint32_t)want) fail("below_mask", 0, j, 0, arc_below_mask(j), want);
    }
    std::vector<uint32_t> masks = {0u, 0xffffffffu};
    for (int b = 0; b < 32; ++b) {
        masks.push_back(1u << b);
        masks.push_back((uint32_t)((1ull << (b + 1)) - 1ull));
        masks.push_back(0xffffffffu << b);
    }
    std::mt19937 rng(12345);
    for (int i = 0; i < 4096; ++i) masks.push_back((uint32_t)rng() & (i % 3 ? 0xffffffffu : (uint32_t)rng()));
    for (const uint32_t mask : masks) {
        const uint64_t p = (uint64_t)__builtin_popcount(mask);
        const uint64_t offs[4] = {0, 1, cap - 1, cap - 1 - p};
        for (const uint64_t off : offs)
            for (int j = 0; j < 32; ++j) {
                const uint32_t below = (uint32_t)((1ull << (j + 1)) - 1ull);
                const uint64_t want = 4ull * (off + (uint64_t)__builtin_popcount(mask & below));
                const uint64_t got = arc_value_byte(mask, j, (uint32_t)(4 * off));
                ++checked;
                if (got != want) fail("value_byte", mask, j, off, got, want);
                if (arc_value_byte_below(mask, below, (uint32_t)(4 * off)) != got) fail("value_byte_below", mask, j, off, 0, got);
                if (off + p < cap) {  // a record the kernel can write
                    ++inside;
                    if (got + 4 > 4 * cap) fail("outside the array", mask, j, off, got, 4 * cap - 4);
                    if (got + 4 == 4 * cap) ++last_word;
                }
            }
    }
    const bool ok = bad == 0 && last_word > 0;
    std::printf("%s cap=%llu checked=%llu inside=%llu last_word=%llu bad=%llu\n", ok ? "OK" : "FAILED",
                (unsigned long long)cap, (unsigned long long)checked, (unsigned long long)inside,
                (unsigned long long)last_word, (unsigned long long)bad);
    return ok ? 0 : 1;
}
