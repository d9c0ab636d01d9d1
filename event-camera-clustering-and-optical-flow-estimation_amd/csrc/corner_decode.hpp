// Division by a launch constant as a multiply-high: the corner kernels turn an item number into
// (group, tile) and a tile into (row, column) once per wave, and a runtime integer division
// compiles to a float-reciprocal sequence with correction steps.  Plain C++: compiles for the
// host too (tests/corner_decode_probe.cpp checks it there).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECC_DECODE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ECC_DECODE_HD inline
#endif

// floor(v / d) for 0 <= v < 2^31 as (v * mul) >> sh, with l = ceil(log2 d), sh = 31 + l and
// mul = ceil(2^sh / d): 2^sh <= mul * d <= 2^sh + 2^l, which is exact for every 31-bit v
// (Granlund & Montgomery 1994, Thm 4.2 with N = 31), and mul < 2^32 for every d below 2^31.
struct MagicDiv {
    uint32_t mul, sh;
};

inline MagicDiv magic_div31(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    const uint32_t sh = 31 + l;
    return MagicDiv{(uint32_t)(((1ull << sh) + d - 1) / d), sh};
}

ECC_DECODE_HD uint32_t magic_quot(uint32_t v, uint32_t mul, uint32_t sh) {
    return (uint32_t)(((uint64_t)v * mul) >> sh);
}
