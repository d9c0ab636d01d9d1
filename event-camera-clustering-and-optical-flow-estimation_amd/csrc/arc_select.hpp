// The arc test's sorting and selection helpers, its maps to clamped keys and the index arithmetic
// of arc_kernel's compact value lists, shared by arc_kernel and arc_dense_kernel.  Plain C++:
// compiles for the host too (tests/arc_select_probe.cpp runs every 0/1 input through the networks
// there, checks arc_keys against arc_streak's count form and the clamps over the int64 edges;
// tests/arc_lookup_probe.cpp runs the index arithmetic over every slice and the edge offsets).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECC_SEL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ECC_SEL_HD inline
#endif

#ifndef ECC_ARC_BATCHER
#define ECC_ARC_BATCHER 0  // 1: circle 4 by the Batcher sort of 32 (twelve zero pads) instead of its selection network
#endif

// Count form of the reference's arc loop: with cnt[j] = #{k : v[k] > v[j]}, the top-s set is
// {j : cnt[j] < s}; an arc of length s exists iff that set has s members (strictly separated from
// the rest) and they are contiguous on the circle.
template <int N, int SMIN, int SMAX>
ECC_SEL_HD bool arc_streak(const int64_t (&v)[N]) {
    int cnt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) cnt[j] = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int k = j + 1; k < N; ++k) {
            cnt[j] += (v[k] > v[j]) ? 1 : 0;
            cnt[k] += (v[j] > v[k]) ? 1 : 0;
        }
    }
    constexpr uint32_t full = (N == 32) ? 0xffffffffu : ((1u << N) - 1u);
    bool ok = false;
#pragma unroll
    for (int s = SMIN; s <= SMAX; ++s) {
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) m |= (cnt[j] < s ? 1u : 0u) << j;
        const uint32_t rot = ((m << 1) | (m >> (N - 1))) & full;  // bit j <- bit j-1
        const uint32_t starts = m & ~rot;
        ok |= (__builtin_popcount(m) == s) && (__builtin_popcount(starts) == 1);
    }
    return ok;
}

// Batcher odd-even merge sort, descending; with compile-time padding and only the top outputs
// used, dead compare-exchanges fold away.
template <int N>
ECC_SEL_HD void sort_desc(uint32_t (&k)[N]) {
#pragma unroll
    for (int p = 1; p < N; p += p) {
#pragma unroll
        for (int kk = p; kk > 0; kk /= 2) {
#pragma unroll
            for (int j = kk % p; j + kk < N; j += kk + kk) {
#pragma unroll
                for (int i = 0; i < kk; ++i) {
                    if (i + j + kk < N && (i + j) / (p + p) == (i + j + kk) / (p + p)) {
                        const uint32_t a = k[i + j], b = k[i + j + kk];
                        k[i + j] = a > b ? a : b;
                        k[i + j + kk] = a > b ? b : a;
                    }
                }
            }
        }
    }
}

// ---- selection network: the sorted top 9 of 20 (circle 4), nothing else ------------------------
// Leaves are sorted triples (three instructions with max3 / med3 / min3, where two compare-
// exchanges give only a sorted pair) and pairs; the runs are merged by Batcher's odd-even merge
// for unequal lengths, shortest two first, each result cut to its top K, and every compare-
// exchange output that cannot reach the top K is dropped (mx: only the maximum is kept).  The
// comparator lists were generated and checked on all 0/1 inputs (a network of max / min / med
// operations sorts every input iff it sorts every 0/1 input); tests/arc_select_probe.cpp repeats
// that check on the code below.  Circle 3 keeps the pruned Batcher sort of 16: the same
// construction gave 91 operations against its 96, one instruction less in the compiled loop
// (the compiler folds the Batcher form into max3 too) and no measurable time; circle 4's network
// is 137 against 159, 18 instructions less per trip, arc_kernel 149.2 -> 147.2 us.
namespace arc_net {
ECC_SEL_HD uint32_t mx2(uint32_t a, uint32_t b) { return a > b ? a : b; }
ECC_SEL_HD uint32_t mn2(uint32_t a, uint32_t b) { return a > b ? b : a; }
ECC_SEL_HD void ce(uint32_t &a, uint32_t &b) {  // a <- max, b <- min
    const uint32_t h = mx2(a, b), l = mn2(a, b);
    a = h, b = l;
}
ECC_SEL_HD void mx(uint32_t &a, uint32_t b) { a = mx2(a, b); }
ECC_SEL_HD void s3(uint32_t &a, uint32_t &b, uint32_t &c) {  // a >= b >= c: v_max3 / v_med3 / v_min3
    const uint32_t h = mx2(mx2(a, b), c), l = mn2(mn2(a, b), c);
    const uint32_t m = mn2(mx2(a, b), mx2(mn2(a, b), c));
    a = h, b = m, c = l;
}
}  // namespace arc_net

// sorted top 9 of 20: 137 operations (the Batcher sort of 32 with twelve zero pads: 159)
ECC_SEL_HD void top9_of_20(uint32_t (&k)[20], uint32_t (&o)[9]) {
    using namespace arc_net;
    ce(k[0], k[1]); ce(k[2], k[3]); s3(k[4], k[5], k[6]); s3(k[7], k[8], k[9]); s3(k[10], k[11], k[12]);
    s3(k[13], k[14], k[15]); ce(k[16], k[17]); ce(k[18], k[19]); ce(k[16], k[18]); ce(k[17], k[19]);
    ce(k[17], k[18]); ce(k[0], k[2]); ce(k[1], k[3]); ce(k[1], k[2]); ce(k[4], k[7]); ce(k[6], k[9]);
    ce(k[6], k[7]); ce(k[5], k[8]); ce(k[5], k[6]); ce(k[8], k[7]); ce(k[10], k[13]); ce(k[12], k[15]);
    ce(k[12], k[13]); ce(k[11], k[14]); ce(k[11], k[12]); ce(k[14], k[13]); ce(k[0], k[16]); ce(k[2], k[18]);
    ce(k[2], k[16]); ce(k[1], k[17]); ce(k[3], k[19]); ce(k[3], k[17]); ce(k[1], k[2]); ce(k[3], k[16]);
    ce(k[17], k[18]); ce(k[10], k[4]); mx(k[13], k[7]); ce(k[13], k[4]); ce(k[12], k[6]); ce(k[12], k[13]);
    ce(k[6], k[4]); ce(k[11], k[5]); mx(k[15], k[9]); ce(k[15], k[5]); ce(k[14], k[8]); ce(k[14], k[15]);
    mx(k[8], k[5]); ce(k[11], k[12]); ce(k[14], k[13]); ce(k[15], k[6]); ce(k[8], k[4]); ce(k[0], k[10]);
    mx(k[4], k[10]); mx(k[16], k[13]); ce(k[16], k[4]); ce(k[2], k[12]); mx(k[18], k[6]); mx(k[18], k[12]);
    ce(k[2], k[16]); ce(k[18], k[4]); ce(k[1], k[11]); mx(k[17], k[15]); ce(k[17], k[11]); ce(k[3], k[14]);
    mx(k[19], k[8]); mx(k[19], k[14]); ce(k[3], k[17]); mx(k[19], k[11]); ce(k[1], k[2]); ce(k[3], k[16]);
    ce(k[17], k[18]); ce(k[19], k[4]);
    o[0] = k[0], o[1] = k[1], o[2] = k[2], o[3] = k[3], o[4] = k[16], o[5] = k[17], o[6] = k[18], o[7] = k[19],
    o[8] = k[4];
}

// The sorted top K of k[0, N) into o: circle 4 by its network unless kBatcher, everything else by
// the Batcher sort padded to 16 or 32.
template <int N, int K, bool kBatcher>
ECC_SEL_HD void arc_top(uint32_t (&k)[N], uint32_t (&o)[K]) {
    if constexpr (!kBatcher && N == 20 && K == 9) {
        top9_of_20(k, o);
    } else {
        constexpr int NP = N <= 16 ? 16 : 32;
        uint32_t p[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) p[i] = i < N ? k[i] : 0u;
        sort_desc<NP>(p);
#pragma unroll
        for (int i = 0; i < K; ++i) o[i] = p[i];
    }
}

// ---- fast arc test on 32-bit keys ------------------------------------------------------------
// Values are mapped to v' = clamp(v - L, 0, 2^27 - 1) with L = t_last(group) - (2^27 - 1) and
// keyed as (v' << IB) | position.  Clamping merges the values <= L into ties at 0.  This cannot
// change the outcome when at least SMAX+1 values are unclamped: a witness k (the largest value
// outside the arc) has <= SMAX values above it, so it and its arc are unclamped and compare as
// before, while a clamped k' has every unclamped value (> SMAX of them) above it in both
// forms.  Otherwise (or when some value exceeds t_last) the exact int64 test runs.
// 1 = arc found, 0 = none, -1 = undecidable on clamped keys (fewer than SMAX+1 unclamped and
// the clamped values not all equal).
template <int N, int IB, int SMIN, int SMAX, bool kBatcher = (ECC_ARC_BATCHER != 0)>
ECC_SEL_HD int arc_keys(uint32_t (&keys)[N], bool ties_exact) {
    uint32_t k[SMAX + 1];
    arc_top<N, SMAX + 1, kBatcher>(keys, k);
    if (!ties_exact && (k[SMAX] >> IB) == 0u) return -1;
    constexpr uint32_t full = (1u << N) - 1u;
    uint32_t m = 0;
    bool ok = false;
#pragma unroll
    for (int s = 1; s <= SMAX; ++s) {
        m |= 1u << (k[s - 1] & ((1u << IB) - 1u));  // IB = 5: the shift's own 5-bit mask, no AND
        if (s >= SMIN) {
            // (a >> IB) > (b >> IB)  <=>  a > (b | low IB bits): one OR, one compare
            const bool sep = k[s - 1] > (k[s] | ((1u << IB) - 1u));
            const uint32_t rot = ((m << 1) | (m >> (N - 1))) & full;
            ok |= sep && (__builtin_popcount(m & ~rot) == 1);
        }
    }
    return ok ? 1 : 0;
}

// ---- the compact value list's index arithmetic (arc_kernel) -----------------------------------
// slices 0 .. j (j <= 31: 2u << 31 is 0 in 32 bits, so j = 31 gives all ones without a select)
ECC_SEL_HD uint32_t arc_below_mask(int j) { return (2u << j) - 1u; }

// A window pixel keeps its clamped B_g slot followed by the values of the slices in `mask`,
// ascending j, from byte `off_bytes` of the value array (a multiple of 4).  The byte an event of
// slice j reads: the B_g slot when no slice <= j touched the pixel, else the value of the latest
// such slice.  The offset is kept in bytes so that the device forms the address with an AND, a
// population count and one shift-and-add (a word offset cost a second shift per lookup).
ECC_SEL_HD uint32_t arc_value_byte_below(uint32_t mask, uint32_t below, uint32_t off_bytes) {
    return ((uint32_t)__builtin_popcount(mask & below) << 2) + off_bytes;
}
ECC_SEL_HD uint32_t arc_value_byte(uint32_t mask, int j, uint32_t off_bytes) {
    return arc_value_byte_below(mask, arc_below_mask(j), off_bytes);
}

// ---- the maps from surface values to clamped keys ---------------------------------------------
// v' = clamp(v - L, 0, vmax) for a narrow group: L + vmax is the group's last timestamp (below
// 2^53 in magnitude, so L + vmax cannot overflow), L may be negative.  A value above the range
// cannot be keyed: it raises *exact_flag (the item takes the exact int64 tests) and maps to vmax.
// The range is checked BEFORE the subtraction: v - L leaves int64 for v near INT64_MAX under a
// negative L (the difference used to wrap, and a wrapped key raised no flag).
//
// arc_kernel's: `inside` says the lane's pixel is on the sensor.  A lane outside it carries
// INT64_MAX, which no test reads and which must not send the item away; a pixel of the surface
// that really holds INT64_MAX is the newest value of its circles and does.
ECC_SEL_HD uint32_t arc_clamp_value(int64_t v, int64_t L, uint32_t vmax, bool narrow, bool inside, int32_t *exact_flag) {
    if (!narrow || v <= L) return 0u;
    if (v > L + (int64_t)vmax) {
        if (inside) *exact_flag = 1;
        return vmax;
    }
    return (uint32_t)(v - L);
}

// arc_dense_kernel's (narrow groups, pixels on the sensor): a value at or below L that is not the
// window minimum vz also raises *mixed_flag (ties among the keys at 0 may then be artefacts).
ECC_SEL_HD uint32_t arc_clamp_rel(int64_t v, int64_t L, int64_t vz, uint32_t vmax, int32_t *exact_flag,
                                  int32_t *mixed_flag) {
    if (v <= L) {
        if (v != vz) *mixed_flag = 1;
        return 0u;
    }
    if (v > L + (int64_t)vmax) {
        *exact_flag = 1;
        return vmax;
    }
    return (uint32_t)(v - L);
}
