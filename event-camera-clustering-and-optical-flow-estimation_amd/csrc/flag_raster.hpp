// The flag pass's raster corner bitmap: one bit per sensor pixel of a slice, bit y * W + x, built
// in LDS from the slice's [n_tiles][kFlagSegWords] result words (flag_decode.hpp's layout, which
// the arc kernels write).  An event's flag depends on (slice, x, y) alone, so with the bits in
// raster order its lookup is one 24-bit multiply-add, a clamp, a shift and a mask; the map from a
// result word's set bit to its pixel runs once per corner pixel of the slice, not once per event.
// Plain C++: compiles for the host too (tests/flag_raster_probe.cpp checks both maps there).
#pragma once
#include <cstdint>

#include "flag_decode.hpp"

// Words of the raster bitmap: ceil(W * H / 32).  Never more than the tile segments' n_tiles * 7
// (W * H <= 196 n_tiles bits against 224 n_tiles).
ECC_DECODE_HD uint32_t flag_raster_words(uint32_t W, uint32_t H) { return (W * H + 31u) >> 5; }

// Bit of the raster bitmap an event reads, for ANY packed u16 pair: y * W + x on the sensor
// (x < W, y < H: below W * H, so no clamp acts); off it some bit at or below last_bit = W * H - 1
// (the product may wrap: W < 2^24, y < 2^16), which flag_on_sensor masks afterwards.
ECC_DECODE_HD uint32_t flag_raster_index(uint32_t x, uint32_t y, uint32_t W, uint32_t last_bit) {
    const uint32_t i = ECC_UMUL24(y, W) + x;
    return i < last_bit ? i : last_bit;
}

// Staging: word i of the slice's [n_tiles][kFlagSegWords] run belongs to tile i / 7 and holds the
// tile pixels lp0 .. lp0 + 31, lp0 = 32 * (i % 7); the tile's origin from tile = ty * tiles_x + tx
// by CornerGeom's divisor (tx_mul, tx_sh: magic_div31(tiles_x)).
struct FlagStageWord {
    uint32_t x0, y0;  // the tile's first pixel
    uint32_t lp0;     // tile pixel of the word's bit 0
};
ECC_DECODE_HD FlagStageWord flag_stage_word(uint32_t i, uint32_t tiles_x, uint32_t tx_mul, uint32_t tx_sh) {
    const uint32_t tile = i / kFlagSegWords;
    const uint32_t ty = magic_quot(tile, tx_mul, tx_sh), tx = tile - ty * tiles_x;
    return FlagStageWord{tx * kFlagTile, ty * kFlagTile, 32u * (i - tile * kFlagSegWords)};
}

// Bit b of that word is tile pixel lp = lp0 + b, pixel (x0 + lp % 14, y0 + lp / 14).  `set` is 0
// for the padding bits of a tile's last word (lp >= 196) and for pixels of an edge tile past the
// sensor (x >= W or y >= H): they set nothing in the raster.
struct FlagStagePixel {
    uint32_t x, y, set;
};
ECC_DECODE_HD FlagStagePixel flag_stage_pixel(const FlagStageWord &sw, uint32_t b, uint32_t W, uint32_t H) {
    const uint32_t lp = sw.lp0 + b;  // < 224
    // floor(lp / 14) for lp < 2^8: 4682 * 14 = 2^16 + 12 and 12 <= 2^(16 - 8) (flag_div14's theorem)
    const uint32_t ly = ECC_UMUL24(lp, 4682u) >> 16;
    const uint32_t x = sw.x0 + (lp - ly * kFlagTile), y = sw.y0 + ly;
    return FlagStagePixel{x, y, (lp < kFlagTile * kFlagTile && x < W && y < H) ? 1u : 0u};
}
