// Stand-alone check of csrc/arc_select.hpp (its own main, only that header, no HIP and no libecc),
// for circle 3's pruned Batcher sort, circle 4's selection network and the Batcher form it replaces:
//   * every 0/1 input: 2^16 through the sorted top 7 of 16, 2^20 through the sorted top 9 of 20
//     (output r must be 1 iff more than r inputs are 1);
//   * 10^5 random key sets with heavy ties per circle against std::sort;
//   * arc_keys against the count form (arc_streak) on the same kind of values, with clamped zeros:
//     the verdict where the keys decide, and the undecidable return exactly where fewer than
//     SMAX + 1 values are unclamped and ties are not exact;
//   * arc_clamp_value and arc_clamp_rel over the int64 edges against 128-bit arithmetic: L negative,
//     zero and positive up to the ends of the narrow groups' range (+-2^53), v from INT64_MIN to
//     INT64_MAX with L, L + 1, L + vmax and L + vmax + 1 in between, on and off the sensor.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>

#include "arc_select.hpp"

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 24);
}

template <int N, int K, bool kBatcher>
static bool zero_one() {
    for (uint32_t x = 0; x < (1u << N); ++x) {
        uint32_t k[N], o[K];
        for (int i = 0; i < N; ++i) k[i] = (x >> i) & 1u;
        arc_top<N, K, kBatcher>(k, o);
        const int ones = __builtin_popcount(x);
        for (int r = 0; r < K; ++r)
            if (o[r] != (ones > r ? 1u : 0u)) {
                std::printf("FAIL 0/1 N=%d batcher=%d x=%x r=%d\n", N, (int)kBatcher, x, r);
                return false;
            }
    }
    return true;
}

template <int N, int K, bool kBatcher>
static bool random_ties(int rounds) {
    for (int it = 0; it < rounds; ++it) {
        uint32_t k[N], s[N], o[K];
        const uint32_t range = 1u + rnd() % 6u;  // 1 .. 6 distinct values: heavy ties
        for (int i = 0; i < N; ++i) s[i] = k[i] = rnd() % range;
        std::sort(s, s + N, std::greater<uint32_t>());
        arc_top<N, K, kBatcher>(k, o);
        for (int r = 0; r < K; ++r)
            if (o[r] != s[r]) {
                std::printf("FAIL ties N=%d batcher=%d it=%d r=%d\n", N, (int)kBatcher, it, r);
                return false;
            }
    }
    return true;
}

// values with few levels (ties, clamped zeros) and, half the time, a planted arc of larger values
template <int N, int SMIN, int SMAX, bool kBatcher>
static bool keys_vs_count(int rounds, uint64_t *undecided) {
    for (int it = 0; it < rounds; ++it) {
        uint32_t v[N];
        const uint32_t levels = 1u + rnd() % 5u;
        for (int i = 0; i < N; ++i) v[i] = (rnd() % 3u == 0u) ? 0u : rnd() % levels;
        if (rnd() & 1u) {
            const int len = 1 + (int)(rnd() % (uint32_t)(SMAX + 2)), at = (int)(rnd() % (uint32_t)N);
            for (int j = 0; j < len; ++j) v[(at + j) % N] = levels + rnd() % 3u;
        }
        int64_t v64[N];
        uint32_t k[N];
        int unclamped = 0;
        for (int i = 0; i < N; ++i) {
            v64[i] = (int64_t)v[i];
            unclamped += v[i] != 0u;
        }
        const bool want = arc_streak<N, SMIN, SMAX>(v64);
        for (int ties_exact = 0; ties_exact < 2; ++ties_exact) {
            for (int i = 0; i < N; ++i) k[i] = (v[i] << 5) | (uint32_t)i;
            const int got = arc_keys<N, 5, SMIN, SMAX, kBatcher>(k, ties_exact != 0);
            const int expect = (!ties_exact && unclamped <= SMAX) ? -1 : (want ? 1 : 0);
            if (expect < 0) ++*undecided;
            if (got != expect) {
                std::printf("FAIL keys N=%d batcher=%d it=%d ties_exact=%d got=%d want=%d\n", N, (int)kBatcher, it,
                            ties_exact, got, expect);
                return false;
            }
        }
    }
    return true;
}

// clamp(v - L, 0, vmax) and its flags in arithmetic that cannot overflow
static bool clamp_edges() {
    constexpr uint32_t vmax = (1u << 27) - 1u;
    const int64_t two53 = (int64_t)1 << 53;
    // L = t_last - vmax for t_last from the bottom to the top of the narrow groups' range
    const int64_t Ls[] = {-two53 + 1 - (int64_t)vmax, -two53, -((int64_t)1 << 40), -(int64_t)vmax - 1, -(int64_t)vmax,
                          -(int64_t)vmax + 1, -5, -1, 0, 1, 1000, (int64_t)1 << 30, two53 - 1 - (int64_t)vmax};
    bool ok = true;
    for (const int64_t L : Ls) {
        const int64_t vs[] = {INT64_MIN, INT64_MIN + 1, L - 1, L, L + 1, L + 2, L + (int64_t)vmax - 1, L + (int64_t)vmax,
                              L + (int64_t)vmax + 1, L + (int64_t)vmax + 2, 0, -1, 1, (int64_t)1 << 62, -((int64_t)1 << 62),
                              INT64_MAX - (int64_t)vmax, INT64_MAX - 1, INT64_MAX};
        for (const int64_t v : vs) {
            const __int128 d = (__int128)v - (__int128)L;
            const uint32_t want = d <= 0 ? 0u : d > (__int128)vmax ? vmax : (uint32_t)d;
            const bool above = d > (__int128)vmax, low = d <= 0;
            for (int narrow = 0; narrow < 2; ++narrow)
                for (int inside = 0; inside < 2; ++inside) {
                    int32_t ex = 0;
                    const uint32_t got = arc_clamp_value(v, L, vmax, narrow != 0, inside != 0, &ex);
                    const bool good = narrow ? got == want && ex == (above && inside ? 1 : 0) : got == 0u && ex == 0;
                    if (!good) {
                        std::printf("arc_clamp_value(v=%lld, L=%lld, narrow=%d, inside=%d) = %u, flag %d\n", (long long)v,
                                    (long long)L, narrow, inside, got, ex);
                        ok = false;
                    }
                }
            for (const int64_t vz : {v, INT64_MIN, L}) {
                int32_t ex = 0, mixed = 0;
                const uint32_t got = arc_clamp_rel(v, L, vz, vmax, &ex, &mixed);
                if (got != want || ex != (above ? 1 : 0) || mixed != (low && v != vz ? 1 : 0)) {
                    std::printf("arc_clamp_rel(v=%lld, L=%lld, vz=%lld) = %u, flags %d %d\n", (long long)v, (long long)L,
                                (long long)vz, got, ex, mixed);
                    ok = false;
                }
            }
        }
    }
    return ok;
}

int main() {
    uint64_t und = 0;
    bool ok = zero_one<16, 7, false>() && zero_one<20, 9, false>() &&
              zero_one<20, 9, true>();
    ok = ok && random_ties<16, 7, false>(100000) &&
         random_ties<20, 9, false>(100000) && random_ties<20, 9, true>(100000);
    ok = ok && keys_vs_count<16, 3, 6, false>(100000, &und) &&
         keys_vs_count<20, 4, 8, false>(100000, &und) && keys_vs_count<20, 4, 8, true>(100000, &und);
    ok = ok && clamp_edges();
    std::printf("%s undecided=%llu\n", ok ? "OK" : "FAILED", (unsigned long long)und);
    return ok && und > 0 ? 0 : 1;
}
