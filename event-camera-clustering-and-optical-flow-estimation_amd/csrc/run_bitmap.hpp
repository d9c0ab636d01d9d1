// The pixel bitmap of a distinct-pixel window (eps.hip's and dbscan.hip's row-run kernels): an
// occupancy bitmap over the window's bounding box, one bit per pixel, 32 pixels a word, rows of
// WW = (Wb >> 5) + 1 words (x == Wb, the end of a run that reaches the right edge, still has a
// word), each word paired with the number of points in the words before it, row-major.  A pixel's
// raster rank is one word read and a popcount; the points of row y in [xl, xh) number
// prefix(y, xh) - prefix(y, xl).  Rows outside the box read a zero word the caller keeps.
// The arithmetic is host-compilable (no HIP include; tests/run_bitmap_probe.cpp checks it against
// brute force); the workgroup steps that build the bitmap follow under __HIPCC__.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include "ecc_internal.hpp"
#define ECC_RUNBM_FN __host__ __device__ __forceinline__
#define ECC_RUNBM_UNROLL(n) _Pragma(#n)
#else
#define ECC_RUNBM_FN inline
#define ECC_RUNBM_UNROLL(n)
#endif

namespace ecc {
namespace runbm {

#if defined(__HIPCC__)
typedef uint2 Word;  // x: occupancy bits, y: points in the words before this one
#else
struct Word { uint32_t x, y; };
#endif

// floor(sqrt(r2i - a^2)), exact; a * a <= r2i.
ECC_RUNBM_FN uint32_t half_width(uint32_t r2i, int a) {
    const uint32_t v = r2i - (uint32_t)(a * a);
    uint32_t h = (uint32_t)__builtin_sqrtf((float)v);
    while (h * h > v) --h;
    while ((h + 1) * (h + 1) <= v) ++h;
    return h;
}

// The bounding box of m points with coordinates in [xmn, xmx] x [ymn, ymx] (m == 0: one pixel).
struct Box {
    int xmn, ymn, Wb, H, WW;
    ECC_RUNBM_FN Box(int m, int x0, int y0, int xmx, int ymx)
        : xmn(x0), ymn(y0), Wb(m ? xmx - x0 + 1 : 1), H(m ? ymx - y0 + 1 : 1), WW((Wb >> 5) + 1) {}
    ECC_RUNBM_FN int64_t words() const { return (int64_t)H * WW; }
};

// Word and bit of the box pixel (x, y): 0 <= x <= Wb, 0 <= y < H.
ECC_RUNBM_FN int word_of(const Box &b, int x, int y) { return y * b.WW + (x >> 5); }
ECC_RUNBM_FN uint32_t bit_of(int x) { return 1u << (x & 31); }

// Points before pixel (x, y) in raster order: the rank of a set pixel.
ECC_RUNBM_FN int rank_at(const Word *wd, const Box &b, int x, int y) {
    const Word q = wd[word_of(b, x, y)];
    return (int)q.y + __builtin_popcount(q.x & (bit_of(x) - 1u));
}

// Points (x', y') of the box with (x' - x)^2 + (y' - y)^2 <= r2i (the same integer test as the
// candidate walks), for hwt[a] = half_width(r2i, a) and amax = min(floor(eps), H - 1) (rows
// further away hold nothing): per row the chord [xl, xh) clipped to the box, as a prefix
// difference (two reads); wd[zero_word] = {0, 0} stands for the rows outside the box.
ECC_RUNBM_FN int chord_count(const Word *wd, int zero_word, const Box &b, const uint16_t *hwt, int x, int y,
                             int amax) {
    int cnt = 0;
    ECC_RUNBM_UNROLL(unroll 4)  // four rows' word loads in flight; no loop-carried state
    for (int a = 0; a <= amax; ++a) {
        const int hw = hwt[a];
        const int xl = x - hw > 0 ? x - hw : 0, xh = x + hw + 1 < b.Wb ? x + hw + 1 : b.Wb;
        const uint32_t ml = bit_of(xl) - 1u, mh = bit_of(xh) - 1u;
        const int cl = xl >> 5, ch = xh >> 5;
        ECC_RUNBM_UNROLL(unroll)
        for (int sgn = 0; sgn < 2; ++sgn) {
            if (sgn && a == 0) break;
            const int yy = sgn ? y - a : y + a;
            const bool ok = (unsigned)yy < (unsigned)b.H;
            const int rb = yy * b.WW;
            const Word lo = wd[ok ? rb + cl : zero_word], hi = wd[ok ? rb + ch : zero_word];
            cnt += (int)(hi.y - lo.y) + __builtin_popcount(hi.x & mh) - __builtin_popcount(lo.x & ml);
        }
    }
    return cnt;
}

#if defined(__HIPCC__)
// The workgroup's steps (nt threads).  tid, lane and wave are arguments: a kernel short of
// registers passes values it re-derives per phase (dbscan.hip's opaque_lane).

// hwt[a] = half_width(r2i, a) for a <= e_int, a < cap.
__device__ __forceinline__ void fill_half_widths(uint16_t *hwt, int cap, int e_int, uint32_t r2i, int tid, int nt) {
    for (int a = tid; a < cap && a <= e_int; a += nt) hwt[a] = (uint16_t)half_width(r2i, a);
}

// The box of the workgroup's m points from each lane's own min / max (0x7fffffff / -1 where it
// holds none), exchanged through box[wave][4] (kW waves).  One barrier.
template <int kW>
__device__ __forceinline__ Box block_box(int (*box)[4], int m, int xmn, int ymn, int xmx, int ymx, int lane, int wave) {
    xmn = wave_min_i32(xmn); ymn = wave_min_i32(ymn);  // DPP
    xmx = wave_max_i32(xmx); ymx = wave_max_i32(ymx);
    if (lane == 0) {
        box[wave][0] = xmn; box[wave][1] = ymn;
        box[wave][2] = xmx; box[wave][3] = ymx;
    }
    __syncthreads();
    xmn = box[0][0]; ymn = box[0][1]; xmx = box[0][2]; ymx = box[0][3];
#pragma unroll
    for (int w = 1; w < kW; ++w) {
        xmn = min(xmn, box[w][0]); ymn = min(ymn, box[w][1]);
        xmx = max(xmx, box[w][2]); ymx = max(ymx, box[w][3]);
    }
    return Box(m, xmn, ymn, xmx, ymx);
}

// Sets the box pixel (x, y); true when it was set already (the window repeats a pixel).
__device__ __forceinline__ bool set_pixel(Word *wd, const Box &b, int x, int y) {
    const uint32_t bit = bit_of(x);
    return atomicOr(&wd[word_of(b, x, y)].x, bit) & bit;
}

// wd[w].y = set bits of wd[0 .. w) for w < words: thread t takes words [t * per, t * per + per).
// One barrier inside (the waves' totals through wsum[nt / 64]); the caller adds one after.
__device__ __forceinline__ void prefix_words(Word *wd, int words, int *wsum, int tid, int lane, int wave, int nt) {
    const int per = (words + nt - 1) / nt;
    const int w0 = tid * per, w1 = min(w0 + per, words);
    int loc = 0;
    for (int w = w0; w < w1; ++w) loc += __popc(wd[w].x);
    const int inc = wave_incl_scan(loc);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = inc - loc;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    for (int w = w0; w < w1; ++w) {
        wd[w].y = (uint32_t)off;
        off += __popc(wd[w].x);
    }
}
#endif

}  // namespace runbm
}  // namespace ecc
