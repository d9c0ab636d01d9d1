// k-means: what the three families (kmeans_xy16.hip, kmeans_f32.hip, kmeans_refcompat.hip) share:
// the constants and the state word, the segment view, the assignment helpers, the one-wave
// update kernel, the hosts' argument check and the dispatch on the compiled K.  Everything has
// internal linkage.
#pragma once

#include "ecc_internal.hpp"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 64;
constexpr int kMaxGrid = 2048;
constexpr int kMaxGridPts = 4096;  // label-image point passes
constexpr int kFastMaxK = 32;
constexpr int kImgSide = 2048;  // label image side (see kmeans_step_kernel)
constexpr int kFlushBatches = 2;  // packed u64 slot fields stay exact for < 512 points

struct KmState {
    int32_t done;
    int32_t iters;
};

// assign_to_centers (KM/assign_to_centers.cl:10-27): the FIRST centre whose fp32 distance
// sqrtf(dx*dx + dy*dy) is strictly below the running best (initially the threshold).  The
// sqrt is only evaluated when d2 drops below the pruning bound pb (a centre with d2 >= pb has
// sqrt >= the current best, so it can never be strictly closer) — about ln(k)+1 square roots
// per point instead of k, with exactly the reference's selection.
__device__ __forceinline__ uint32_t assign_point(float px, float py, const float2 *__restrict__ c,
                                                 int k, float thr) {
    uint32_t best = 255u;
    float best_s = thr, pb = __builtin_inff();
    for (int i = 0; i < k; ++i) {
        const float2 ci = c[i];
        const float dx = __fsub_rn(ci.x, px), dy = __fsub_rn(ci.y, py);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
        if (d2 < pb) {
            pb = d2;
            const float s = ecc::sqrt_rn(d2);
            if (s < best_s) { best_s = s; best = (uint32_t)i; }
        }
    }
    return best;
}

// Segment geometry: segment s holds count(s) points at base s*stride.  A caller's count is
// clamped to [0, stride] (ecc::seg_points), so a segment never runs into the next one; the dense
// form (counts == null) is one array of n_dense points re-cut into full segments and a remainder.
struct Segs {
    const int32_t *counts;  // nullable
    int64_t n_segs, stride, n_dense;
    __device__ __forceinline__ int64_t count(int64_t s) const {
        if (counts) return ecc::seg_points(counts, stride, s);
        const int64_t r = n_dense - s * stride;
        return r < stride ? r : stride;
    }
};

// ---- fast path for k <= 32: compile-time K, centroids in scalar registers -----------------
// Exact argmin without a square root per centre: sqrt_rn is monotone, so the reference's
// choice (first centre with the smallest sqrt_rn(d2), if below thr) is the first index of the
// smallest d2 — unless an EARLIER centre has a larger d2 that rounds to the same square root.
// That needs d2_i / d2_min <= ((1 + 2^-24) / (1 - 2^-24))^2 < 1 + 2^-22; the single pass
// keeps m_prev = min d2 over the indices before the winner and takes the exact
// sqrt-per-centre loop (assign_point's rule) only when m_prev <= m * (1 + 2^-20).
template <int K>
__device__ __forceinline__ uint32_t assign_fast(float px, float py, const float (&cx)[K],
                                                const float (&cy)[K], float thr) {
    float m = __builtin_inff(), m_prev = __builtin_inff();
    int ia = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float dx = __fsub_rn(cx[i], px), dy = __fsub_rn(cy[i], py);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
        const bool lt = d2 < m;
        m_prev = lt ? m : m_prev;
        ia = lt ? i : ia;
        m = lt ? d2 : m;
    }
    if (__builtin_expect(m_prev <= __fmul_rn(m, 1.0f + 0x1p-20f), 0)) {
        uint32_t best = 255u;
        float best_s = thr;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float dx = __fsub_rn(cx[i], px), dy = __fsub_rn(cy[i], py);
            const float s = ecc::sqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            if (s < best_s) { best_s = s; best = (uint32_t)i; }
        }
        return best;
    }
    return ecc::sqrt_rn(m) < thr ? (uint32_t)ia : 255u;
}

// The f32 engine's screen on the packed fp32 ALU (v_pk_add/mul/fma_f32), two centres per op.
// d2' = fma(dx, dx, dy*dy) (dx, dy exact as the reference's) is within 2 ulps of the reference's
// d2 = dx*dx + dy*dy; keys (bits(d2') & ~31) | i order the centres by 32-ulp bucket, then index,
// and one v_min + one v_med3 per centre keep the smallest two keys.  When the second-best key
// lies two or more buckets above the best (>= 33 ulps, i.e. > 2^-19 relative, beyond both the
// d2' error and assign_fast's 2^-20 square-root tie band), the best index is the reference's
// unique choice: the first centre with the smallest sqrt_rn(d2).  Its exact d2 then meets the
// threshold as d2 < thr2 (thr2 = the first float whose correctly rounded sqrt is >= thr, found
// by bisection on the host: sqrt_rn is monotone).  Closer calls, inf and NaN take assign_fast.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// median of three: with a <= b the two smallest of {a, b, c} are min(a, c) and med3(a, b, c).
// The min/max idiom is not matched to v_med3_u32 for register operands, hence the asm.
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// One point against the centres two at a time: the packed operands are a centre PAIR (two
// consecutive scalar registers, no copies) and the point broadcast, so the screen costs
// 2 packed + 3 scalar (v_and_or, v_min, v_med3) instructions per centre and point.
template <int K>
__device__ __forceinline__ void screen_point(float px, float py, const float (&cx)[K], const float (&cy)[K],
                                             uint32_t &k1, uint32_t &k2) {
    const f32x2 pxx = {px, px}, pyy = {py, py};
    k1 = 0xffffffffu;
    k2 = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < K; i += 2) {
        const f32x2 dx = (f32x2){cx[i], cx[i + 1]} - pxx, dy = (f32x2){cy[i], cy[i + 1]} - pyy;
        const f32x2 d2 = __builtin_elementwise_fma(dx, dx, dy * dy);
        const uint32_t ka = (__float_as_uint(d2.x) & ~31u) | (uint32_t)i;
        const uint32_t kb = (__float_as_uint(d2.y) & ~31u) | (uint32_t)(i + 1);
        k2 = umed3(k1, k2, ka);
        k1 = min(k1, ka);
        k2 = umed3(k1, k2, kb);
        k1 = min(k1, kb);
    }
}

template <int K>
__device__ __forceinline__ uint32_t finish_point(float px, float py, uint32_t k1, uint32_t k2,
                                                 const float (&cx)[K], const float (&cy)[K],
                                                 const float2 *__restrict__ s_c, float thr, float thr2) {
    constexpr uint32_t kInfBucket = 0x7F800000u >> 5;
    if (__builtin_expect((k1 >> 5) < kInfBucket && (k2 >> 5) > (k1 >> 5) + 1u, 1)) {
        const float2 c = s_c[k1 & 31u];
        const float dx = __fsub_rn(c.x, px), dy = __fsub_rn(c.y, py);
        return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < thr2 ? (k1 & 31u) : 255u;
    }
    return assign_fast<K>(px, py, cx, cy, thr);
}

template <int K>
__device__ __forceinline__ void assign_pair(float2 p0, float2 p1, const float (&cx)[K], const float (&cy)[K],
                                            const float2 *__restrict__ s_c, float thr, float thr2, uint32_t &l0,
                                            uint32_t &l1) {
    // the two points' screens interleaved centre pair by centre pair: two independent min/med3
    // chains per step (one point's chain alone leaves the VALU waiting on its own results)
    uint32_t a1 = 0xffffffffu, a2 = 0xffffffffu, b1 = 0xffffffffu, b2 = 0xffffffffu;
    {
        const f32x2 pxa = {p0.x, p0.x}, pya = {p0.y, p0.y}, pxb = {p1.x, p1.x}, pyb = {p1.y, p1.y};
#pragma unroll
        for (int i = 0; i < K; i += 2) {
            const f32x2 ccx = {cx[i], cx[i + 1]}, ccy = {cy[i], cy[i + 1]};
            const f32x2 dxa = ccx - pxa, dya = ccy - pya, dxb = ccx - pxb, dyb = ccy - pyb;
            const f32x2 da = __builtin_elementwise_fma(dxa, dxa, dya * dya);
            const f32x2 db = __builtin_elementwise_fma(dxb, dxb, dyb * dyb);
            const uint32_t ka0 = (__float_as_uint(da.x) & ~31u) | (uint32_t)i;
            const uint32_t kb0 = (__float_as_uint(db.x) & ~31u) | (uint32_t)i;
            const uint32_t ka1 = (__float_as_uint(da.y) & ~31u) | (uint32_t)(i + 1);
            const uint32_t kb1 = (__float_as_uint(db.y) & ~31u) | (uint32_t)(i + 1);
            a2 = umed3(a1, a2, ka0);
            b2 = umed3(b1, b2, kb0);
            a1 = min(a1, ka0);
            b1 = min(b1, kb0);
            a2 = umed3(a1, a2, ka1);
            b2 = umed3(b1, b2, kb1);
            a1 = min(a1, ka1);
            b1 = min(b1, kb1);
        }
    }
    l0 = finish_point<K>(p0.x, p0.y, a1, a2, cx, cy, s_c, thr, thr2);
    l1 = finish_point<K>(p1.x, p1.y, b1, b2, cx, cy, s_c, thr, thr2);
}

// assign_fast's arithmetic, step for step, with the centres read from LDS inside a rolled loop
// (the asm barrier keeps the compiler from hoisting them into registers).  Used by the
// label-image passes for points outside the image only; tests/test_gpu_parity.py covers both
// the outside points and the near-tie rule.
template <int K>
__device__ __forceinline__ uint32_t assign_lds(float px, float py, const float *s_cx, const float *s_cy, float thr) {
    float m = __builtin_inff(), m_prev = __builtin_inff();
    int ia = 0;
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
        asm volatile("" ::: "memory");
        const float dx = __fsub_rn(s_cx[i], px), dy = __fsub_rn(s_cy[i], py);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
        const bool lt = d2 < m;
        m_prev = lt ? m : m_prev;
        ia = lt ? i : ia;
        m = lt ? d2 : m;
    }
    if (m_prev <= __fmul_rn(m, 1.0f + 0x1p-20f)) {
        uint32_t best = 255u;
        float best_s = thr;
#pragma unroll 1
        for (int i = 0; i < K; ++i) {
            asm volatile("" ::: "memory");
            const float dx = __fsub_rn(s_cx[i], px), dy = __fsub_rn(s_cy[i], py);
            const float s = ecc::sqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            if (s < best_s) { best_s = s; best = (uint32_t)i; }
        }
        return best;
    }
    return ecc::sqrt_rn(m) < thr ? (uint32_t)ia : 255u;
}

__device__ __forceinline__ uint64_t lanes_below_mask(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

__device__ __forceinline__ float uniform_f32(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// Replicated accumulators: the per-WG flush goes to replica blockIdx % n_copies, which spreads
// the same-address global atomics; the update kernel sums the replicas.
constexpr int kAccStride = 3 * kMaxK;
constexpr int kAccCopies = 16;  // replicas: 256 pixel-pass WGs -> 16 atomics per address

// Host: the smallest float s >= 0 with sqrtf(s) >= thr (sqrtf correctly rounded, like sqrt_rn;
// monotone), so that sqrt_rn(d2) < thr <=> d2 < thr2.  Bisection over the bit patterns.
inline float sqrt_threshold(float thr) {
    if (!(thr > 0.f)) return 0.f;           // nothing is below (NaN threshold: nothing either)
    if (std::isinf(thr)) return __builtin_inff();
    uint32_t lo = 0u, hi = 0x7F800000u;      // sqrt(+0) < thr; sqrt(+inf) = inf >= thr
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float f;
        std::memcpy(&f, &mid, 4);
        (std::sqrt(f) < thr ? lo : hi) = mid;
    }
    float r;
    std::memcpy(&r, &hi, 4);
    return r;
}

// Centroid update, one wave: c = (float)(sum / n) (fp64), shift = max |new - old|.
// Sums n_copies replicas of acc (stride kAccStride) and zeroes them.
template <typename AccT>
__global__ void __launch_bounds__(64)
kmeans_update_kernel(AccT *__restrict__ acc, int n_copies, float *__restrict__ cent, int k, float tol,
                     KmState *__restrict__ st) {
    if (st->done) return;
    const int lane = threadIdx.x;
    float shift = 0.f;
    if (lane < k) {
        AccT a[3] = {0, 0, 0};
        AccT v[kAccCopies][3];  // every replica's loads in flight together
#pragma unroll
        for (int r = 0; r < kAccCopies; ++r)
#pragma unroll
            for (int f = 0; f < 3; ++f) v[r][f] = r < n_copies ? acc[r * kAccStride + 3 * lane + f] : (AccT)0;
#pragma unroll
        for (int r = 0; r < kAccCopies; ++r)
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                a[f] += v[r][f];
                if (r < n_copies) acc[r * kAccStride + 3 * lane + f] = 0;
            }
        const double n_pts = (double)a[0];
        if (n_pts > 0.0) {
            const float nx = (float)((double)a[1] / n_pts);
            const float ny = (float)((double)a[2] / n_pts);
            shift = fmaxf(fabsf(nx - cent[2 * lane]), fabsf(ny - cent[2 * lane + 1]));
            cent[2 * lane] = nx;
            cent[2 * lane + 1] = ny;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) shift = fmaxf(shift, __shfl_xor(shift, o));
    if (lane == 0) {
        st->iters += 1;
        if (tol >= 0.f && shift <= tol) st->done = 1;
    }
}

int grid_for(int64_t units) {
    int64_t g = units < kMaxGrid ? units : kMaxGrid;
    return g < 1 ? 1 : (int)g;
}

// The fast kernels are compiled for K = 16 and K = 32 centres: f(integral_constant<int, K>) for
// the smaller K that holds k (k <= kFastMaxK).
template <class F>
void dispatch_k(int k, F &&f) {
    if (k <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 32>{});
}

inline int kmeans_check(const ecc_ctx *ctx, const ecc_kmeans_cfg *cfg, const float *centroids) {
    if (!ctx || !cfg || !centroids) return ECC_ERR_INVALID;
    if (cfg->k < 1 || cfg->k > kMaxK || cfg->max_iters < 0) return ECC_ERR_INVALID;
    return ECC_OK;
}

}  // namespace
