// The flag pass's map from an event to its corner bit: the word of the slice's result segments
// (tile * kSegWords + pixel-in-tile / 32) and the bit in it, for ANY packed u16 pair, from 24-bit
// multiplies and shifts only (a runtime y / 14 * tiles_x is a 64-bit mad plus a 32-bit multiply,
// both quarter rate).  The word index is clamped to the segments' last word, so a lookup never
// leaves its array; whether the event is on the sensor is a separate mask (flag_on_sensor), applied
// to the bit afterwards.  Plain C++: compiles for the host too (tests/flag_decode_probe.cpp checks
// it there against the / 14, % 14 form over every u16 pair).
#pragma once
#include <cstdint>

#include "corner_decode.hpp"

// low 32 bits of the product of the operands' low 24 bits (v_mul_u32_u24); the host form computes
// the same value, so the probe sees what the kernel sees
#if defined(__HIP_DEVICE_COMPILE__)
#define ECC_UMUL24(a, b) __umul24((a), (b))
#define ECC_DECODE_OPAQUE(v) asm("" : "+v"(v))  // no instruction: the value, unknown to the optimiser
#else
#define ECC_UMUL24(a, b) ((uint32_t)(((a) & 0xffffffu) * ((b) & 0xffffffu)))
#define ECC_DECODE_OPAQUE(v) ((void)0)
#endif

constexpr uint32_t kFlagTile = 14;      // corner::kTile
constexpr uint32_t kFlagSegWords = 7;   // corner::kSegWords: ceil(196 / 32)

// floor(v / 14) for v < 2^16: v / 14 = (v >> 1) / 7, and for u < 2^15 floor(u / 7) =
// (u * 37450) >> 18, since 37450 * 7 = 2^18 + 6 and 6 <= 2^(18 - 15) (Granlund & Montgomery 1994,
// Thm 4.2 with N = 15); u * 37450 < 2^31.
ECC_DECODE_HD uint32_t flag_div14(uint32_t v) { return ECC_UMUL24(v >> 1, 37450u) >> 18; }

struct FlagSlot {
    uint32_t word;  // index into the slice's [n_tiles][kSegWords] words, <= last_word
    uint32_t bit;   // bit of that word, 0..31
};

// x, y in [0, 65535]; tiles_x <= 8191 (corner::kMaxTiles); last_word = n_tiles * kSegWords - 1.
// The pixel in the tile is (y - 14 ty) * 14 + (x - 14 tx) = (14 y + x) - (196 ty + 14 tx): every
// factor is below 2^16 by its own bit width, so each product is one 24-bit multiply-add (a
// product of a difference is not: the compiler cannot bound it and takes the 64-bit mad).  On the
// sensor (x < W, y < H) the index is the pixel's own word (tile < n_tiles, so no clamp acts);
// off it the index stays below 2^30 and the clamp alone keeps it inside.
ECC_DECODE_HD FlagSlot flag_slot(uint32_t x, uint32_t y, uint32_t tiles_x, uint32_t last_word) {
    const uint32_t tx = flag_div14(x), ty = flag_div14(y);
    const uint32_t lp = (ECC_UMUL24(y, kFlagTile) + x) - (ECC_UMUL24(ty, kFlagTile * kFlagTile) + ECC_UMUL24(tx, kFlagTile));
    // (ty * tiles_x + tx) * 7 + lp / 32, the row's 7 * tiles_x words a uniform factor below 2^16.
    // The column's part is kept from the optimiser's view: it would factor the 7 back out, and
    // (ty * tiles_x + tx) * 7 is no 24-bit product.
    uint32_t col = ECC_UMUL24(tx, kFlagSegWords) + (lp >> 5);
    ECC_DECODE_OPAQUE(col);
    const uint32_t w = ECC_UMUL24(ty, (tiles_x & 0x1fffu) * kFlagSegWords) + col;
    return FlagSlot{w < last_word ? w : last_word, lp & 31u};
}

// 1 on the sensor, else 0 (W, H >= 1)
ECC_DECODE_HD uint32_t flag_on_sensor(uint32_t x, uint32_t y, uint32_t W, uint32_t H) {
    return (x < W && y < H) ? 1u : 0u;
}
