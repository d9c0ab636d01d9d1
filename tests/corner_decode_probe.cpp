// Stand-alone check of csrc/corner_decode.hpp (its own main, only that header, no HIP and no
// libecc): magic_quot(v, magic_div31(d)) == v / d for 0 <= v < 2^31.
//   * every divisor 1 .. 8192 (the corner kernels divide by tile counts up to 8191) and a few
//     large ones, at the dividends where a multiply-high quotient can first go wrong: the last
//     value of a quotient step (k d - 1), the first of the next (k d) and its neighbours, for the
//     lowest and highest quotients and 64 spread over the range, and 2^31 - 1 itself;
//   * every dividend below 2^31 for the tile count of a 1600 x 900 sensor (7475).
#include <cstdint>
#include <cstdio>

#include "corner_decode.hpp"

static uint64_t g_checked = 0;

static bool check(uint32_t v, uint32_t d, const MagicDiv &m) {
    ++g_checked;
    if (magic_quot(v, m.mul, m.sh) == v / d) return true;
    std::printf("FAIL v=%u d=%u mul=%u sh=%u got=%u want=%u\n", v, d, m.mul, m.sh, magic_quot(v, m.mul, m.sh), v / d);
    return false;
}

static bool check_divisor(uint32_t d) {
    const MagicDiv m = magic_div31(d);
    if (m.sh < 31 || m.sh > 62) {
        std::printf("FAIL d=%u sh=%u\n", d, m.sh);
        return false;
    }
    const uint64_t top = (1ull << 31) - 1;
    const uint64_t qmax = top / d;
    bool ok = check((uint32_t)top, d, m) && check(0u, d, m);
    uint64_t x = 0x9e3779b97f4a7c15ull ^ d;
    for (int i = 0; i < 64 + 6 && ok; ++i) {
        uint64_t k;
        if (i < 3) k = (uint64_t)i;
        else if (i < 6) k = qmax - (uint64_t)(i - 3);
        else {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift
            k = x % (qmax + 1);
        }
        for (int64_t o = -2; o <= 2 && ok; ++o) {
            const int64_t v = (int64_t)(k * d) + o;
            if (v >= 0 && (uint64_t)v <= top) ok = check((uint32_t)v, d, m);
        }
    }
    return ok;
}

int main() {
    bool ok = true;
    for (uint32_t d = 1; d <= 8192 && ok; ++d) ok = check_divisor(d);
    const uint32_t large[] = {8193, 65535, 65536, 65537, 1000003, (1u << 30) - 1, 1u << 30, (1u << 30) + 1, (1u << 31) - 1};
    for (uint32_t d : large)
        if (ok) ok = check_divisor(d);
    if (ok) {
        const uint32_t d = 7475;
        const MagicDiv m = magic_div31(d);
        uint32_t q = 0, r = 0;  // v / d and v % d, carried along
        for (uint32_t v = 0; v < (1u << 31); ++v) {
            if (magic_quot(v, m.mul, m.sh) != q) {
                std::printf("FAIL sweep v=%u d=%u\n", v, d);
                ok = false;
                break;
            }
            if (++r == d) r = 0, ++q;
        }
        g_checked += 1ull << 31;
    }
    std::printf("%s checked=%llu\n", ok ? "OK" : "FAILED", (unsigned long long)g_checked);
    return ok ? 0 : 1;
}
