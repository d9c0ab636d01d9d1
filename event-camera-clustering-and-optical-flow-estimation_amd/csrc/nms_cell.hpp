// The greedy NMS pass's cell arithmetic, in plain C++ so that the host can check it
// (tests/nms_cell_probe.cpp): the cell of a coordinate by multiply-high (corner_decode.hpp), and the
// probe of a grid cell without a test for "empty".
#pragma once
#include <cstdint>

#include "corner_decode.hpp"

constexpr uint32_t kNoCentre = 0xffffffffu;  // an empty grid cell
// An empty cell unpacks to (65535, 65535): at least 32769 from every coordinate of a sensor of at
// most 32767 pixels a side, while two centres inside the sensor are at most 32766 apart.  A reach
// cut at 32767 therefore decides every pair of centres as the uncut one does and never reaches an
// empty cell.
constexpr int kReachMax = 32767;

ECC_DECODE_HD int nms_reach(int half) { return 2 * half < kReachMax ? 2 * half : kReachMax; }

// "Within reach r on both axes" as one unsigned compare: |x - cx| <= r iff 0 <= x + r - cx <= 2 r,
// and a negative difference wraps to more than any 2 r, so with the candidate's (x + r, y + r) at hand
//     max(x + r - cx, y + r - cy) <= 2 r        (uint32)
// is two subtracts, a maximum and a compare per centre.  For an empty cell (cx = 65535) the first
// difference is negative for every x + r <= 65534, which x <= 32766 and r <= kReachMax give.
struct NmsKey {
    uint32_t xr, yr;
};
ECC_DECODE_HD NmsKey nms_key(uint32_t v, int reach) {
    return NmsKey{(v & 0xffffu) + (uint32_t)reach, (v >> 16) + (uint32_t)reach};
}
ECC_DECODE_HD uint32_t nms_span(NmsKey k, uint32_t centre) {
    const uint32_t a = k.xr - (centre & 0xffffu), b = k.yr - (centre >> 16);
    return a > b ? a : b;
}

// Chebyshev distance of two packed centres (x | y << 16).
ECC_DECODE_HD int nms_cell_dist(uint32_t a, uint32_t b) {
    const int dx = (int)(a & 0xffffu) - (int)(b & 0xffffu), dy = (int)(a >> 16) - (int)(b >> 16);
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    return ax > ay ? ax : ay;
}
