// Stand-alone check of csrc/nms_cell.hpp (its own main, only that header and corner_decode.hpp, no
// HIP and no libecc):
//   * the cell of a coordinate: magic_quot(v, magic_div31(cs)) == v / cs for every 16-bit v and every
//     cell size 1 .. 63 (boxes up to 63), and for a few large cell sizes;
//   * the unguarded probe: an empty cell is further than nms_reach(half) from every coordinate pair a
//     sensor of up to 32767 x 32767 can hold, for every half; and the cut reach decides two centres
//     inside such a sensor as 2 * half does; the one-compare form (nms_key, nms_span) says the same.
#include <cstdint>
#include <cstdio>

#include "nms_cell.hpp"

int main() {
    unsigned long long checked = 0;
    const uint32_t large[] = {64, 255, 256, 257, 32767, 65535, 65536, 65537, (1u << 31) - 1};
    for (uint32_t i = 1; i <= 63 + sizeof(large) / sizeof(large[0]); ++i) {
        const uint32_t cs = i <= 63 ? i : large[i - 64];
        const MagicDiv m = magic_div31(cs);
        for (uint32_t v = 0; v < 65536; ++v, ++checked)
            if (magic_quot(v, m.mul, m.sh) != v / cs) {
                std::printf("FAIL cell v=%u cs=%u got=%u want=%u\n", v, cs, magic_quot(v, m.mul, m.sh), v / cs);
                return 1;
            }
    }
    // the distance is a maximum over the axes, so the axis extremes (0 and 32766) decide for an empty
    // cell; the values between them are there for the pairs of centres
    const int halves[] = {0, 1, 7, 15, 31, 16383, 16384, 1 << 20, (1 << 30) - 1};
    const uint32_t ends[] = {0u, 1u, 2u, 14u, 15u, 16u, 29u, 30u, 31u, 62u, 63u, 16383u, 32765u, 32766u};
    for (int half : halves) {
        const int reach = nms_reach(half);
        if (reach > kReachMax || (2 * half <= kReachMax && reach != 2 * half)) {
            std::printf("FAIL reach half=%d reach=%d\n", half, reach);
            return 1;
        }
        for (uint32_t x : ends)
            for (uint32_t y : ends) {
                const uint32_t v = x | y << 16;
                ++checked;
                const NmsKey key = nms_key(v, reach);
                if (nms_cell_dist(kNoCentre, v) <= reach || nms_cell_dist(v, kNoCentre) <= reach ||
                    nms_span(key, kNoCentre) <= 2u * (uint32_t)reach) {
                    std::printf("FAIL empty cell reached: half=%d x=%u y=%u\n", half, x, y);
                    return 1;
                }
                for (uint32_t x2 : ends)
                    for (uint32_t y2 : ends) {
                        const int d = nms_cell_dist(v, x2 | y2 << 16);
                        ++checked;
                        if ((d <= reach) != ((long long)d <= 2ll * half) ||
                            (nms_span(key, x2 | y2 << 16) <= 2u * (uint32_t)reach) != (d <= reach)) {
                            std::printf("FAIL cut reach: half=%d d=%d\n", half, d);
                            return 1;
                        }
                    }
            }
    }
    for (uint32_t x = 0; x < 32767; ++x, ++checked)  // every coordinate on one axis, the other at its nearest
        if (nms_cell_dist(kNoCentre, x | 32766u << 16) < 32769 || nms_cell_dist(kNoCentre, 32766u | x << 16) < 32769 ||
            nms_span(nms_key(x | 32766u << 16, kReachMax), kNoCentre) <= 2u * kReachMax ||
            nms_span(nms_key(32766u | x << 16, kReachMax), kNoCentre) <= 2u * kReachMax) {
            std::printf("FAIL empty cell distance x=%u\n", x);
            return 1;
        }
    std::printf("OK checked=%llu\n", checked);
    return 0;
}
