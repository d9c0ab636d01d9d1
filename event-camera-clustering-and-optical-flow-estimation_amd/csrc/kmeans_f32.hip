// k-means over float points (the reference's data layout, BASELINE config C3): the generic kernel,
// the vector and the two matrix-core engines, and the candidate table of the vector engine.
#include "kmeans_common.hpp"

#ifndef ECC_KM_LUT_WG_PER_CU
#define ECC_KM_LUT_WG_PER_CU 5
#endif
#ifndef ECC_KM_LAB_WG_PER_CU
#define ECC_KM_LAB_WG_PER_CU 6
#endif
#ifndef ECC_KM_LUT_UNROLL
#define ECC_KM_LUT_UNROLL 4
#endif
#ifndef ECC_KM_MFMA_BLOCKS
#define ECC_KM_MFMA_BLOCKS 1  // matrix engine: 64-pair blocks per trip
#endif
#ifndef ECC_KM_MFMA_WAVES
#define ECC_KM_MFMA_WAVES 4  // matrix engine 3: waves/SIMD the register budget is held to
#endif
#ifndef ECC_KM_ACC_SUB
#define ECC_KM_ACC_SUB 4
#endif

namespace {

// float-input variant (reference data layout: interleaved float x,y): fp64 LDS + global
// atomics (order-dependent only at the 1e-16 relative level).
template <bool kAccumulate>
__global__ void __launch_bounds__(kThreads)
kmeans_f32_kernel(const float *__restrict__ xy, int64_t n, const float *__restrict__ cent, int k,
                  float thr, double *__restrict__ acc, const KmState *__restrict__ st,
                  uint8_t *__restrict__ labels) {
    if (kAccumulate && st->done) return;
    __shared__ float2 c_lds[kMaxK];
    __shared__ double a_s[kMaxK * 3];
    const int tid = threadIdx.x;
    if (tid < k) c_lds[tid] = make_float2(cent[2 * tid], cent[2 * tid + 1]);
    if (kAccumulate)
        for (int i = tid; i < kMaxK * 3; i += kThreads) a_s[i] = 0.0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float2 p = reinterpret_cast<const float2 *>(xy)[i];
        const uint32_t lab = assign_point(p.x, p.y, c_lds, k, thr);
        if (labels) labels[i] = (uint8_t)lab;
        if (kAccumulate && lab != 255u) {
            atomicAdd(&a_s[3 * lab + 0], 1.0);
            atomicAdd(&a_s[3 * lab + 1], (double)p.x);
            atomicAdd(&a_s[3 * lab + 2], (double)p.y);
        }
    }
    if (kAccumulate) {
        __syncthreads();
        if (tid < 3 * k && a_s[tid] != 0.0) atomicAdd(&acc[tid], a_s[tid]);
    }
}

// ---- float points, k <= 32 (BASELINE config C3): two assignment engines, one accumulation ---------
// Vector engine: assign_fast<K> with the centres in scalar registers (exact, ~9 VALU per centre).
// Matrix engine: the distance part on the matrix cores.  v_mfma_f32_4x4x1f32 runs 16 blocks of
// 4x4x1; with block b = lanes 4b..4b+3, A_b[i] = -2 cx_{4g+i} (lane 4b+i) and B_b[j] = px of
// lane 4b+j, D_b[i][j] (lane 4b+j, register i) = C + A_b[i] B_b[j]: so two MFMAs per group g of
// four centres give every lane s_i = |c_i|^2 - 2 c_i.p for ITS OWN point (an fma chain, one
// rounding per step).  The argmin over s equals the argmin over d^2 = s + |p|^2 up to rounding:
// with E bounding the error of every s (E = 2^-21 (max|c|^2 + 2 max|cx| |px| + 2 max|cy| |py|),
// >= 4x the worst case of the three roundings), a gap between the best and second-best s above
// 2E + 2^-19 (|s_best| + |p|^2 + E) proves the best index is the unique d^2 minimum with no
// earlier centre inside assign_fast's square-root tie band; the winner's exact d^2 then decides
// the threshold.  Any closer call (and NaN input) takes the exact vector path.
// The argument assumes only that each of the three roundings of s is bounded — not the order in
// which the matrix core sums the products, nor how it treats subnormals: a relative bound does
// not hold for subnormal or flushed results, so E also carries an absolute term (kAbsRound)
// above three flushes to zero of a result below the smallest normal (3 x 2^-126).  Points whose
// gaps are that small (coordinates around 1e-19 and below) always take the exact path.
// Accumulation (both engines): per wave LDS slots, u32 count and fp64 sums (ds_add_f64: exact for
// integer-valued coordinates, 1e-16 relative otherwise); per workgroup one fp64 global atomic per
// (cluster, field) into one of n_copies replicas that the update kernel sums.
typedef float floatx4_t __attribute__((ext_vector_type(4)));
constexpr float kAbsRound = 0x1p-124f;  // > 3 x 2^-126: the absolute part of E (see above)

template <int K>
__device__ __forceinline__ uint32_t assign_mfma(float px, float py, const float (&ax)[K / 4], const float (&ay)[K / 4],
                                                const float (&c2)[K], float emul_c2, float emul_x, float emul_y,
                                                const float2 *__restrict__ s_c, const float (&cx)[K],
                                                const float (&cy)[K], float thr, float thr2) {
    floatx4_t d[K / 4];
#pragma unroll
    for (int g = 0; g < K / 4; ++g) {
        d[g] = floatx4_t{c2[4 * g], c2[4 * g + 1], c2[4 * g + 2], c2[4 * g + 3]};
        d[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(ax[g], px, d[g], 0, 0, 0);
        d[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(ay[g], py, d[g], 0, 0, 0);
    }
    float b = __builtin_inff(), b2 = __builtin_inff();
    int bi = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float v = d[i / 4][i % 4];
        const bool lt = v < b;
        b2 = lt ? b : fminf(b2, v);
        bi = lt ? i : bi;
        b = lt ? v : b;
    }
    const float E = 0x1p-21f * (emul_c2 + 2.0f * (emul_x * fabsf(px) + emul_y * fabsf(py))) + kAbsRound;
    const float P = px * px + py * py;
    const float margin = 2.0f * E + 0x1p-19f * (fabsf(b) + P + E);
    if (__builtin_expect(!(b2 - b > margin), 0)) return assign_fast<K>(px, py, cx, cy, thr);  // close call / NaN
    const float2 c = s_c[bi];
    const float dx = __fsub_rn(c.x, px), dy = __fsub_rn(c.y, py);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < thr2 ? (uint32_t)bi : 255u;  // sqrt_rn(d2) < thr
}

// Matrix engine, streaming form (k <= 16, 16-B aligned points): v_mfma_f32_32x32x2f32, a 32 x 32
// x 2 product per instruction (4x the work of the 4x4x1 form above at twice its cycles).  A = 32
// centre rows (k index 0: -2 cx, 1: -2 cy), row i holding centre (i & 3) | (i >> 3) << 2, so that
// D register r of EVERY lane is centre r (rows (r&3) + 8 (r>>2) + 4 (lane>>5)); B = 32 point
// columns (lanes 0-31: x, lanes 32-63: y of point lane & 31); C = |c_r|^2.  D is the same k-ordered
// fma chain as assign_mfma's two 4x4x1 steps, fma(-2cy, py, fma(-2cx, px, |c|^2)).  Both halves of
// the wave see the same 32 columns, so each pair of instructions (even and odd points of 32 pairs)
// leaves lanes 0-31 the even points' 16 values and lanes 32-63 the odd points'.
typedef float floatx16_t __attribute__((ext_vector_type(16)));

// The argmin of one point from its 16 MFMA values s_r = |c_r|^2 - 2 c_r.p: the smallest s, and the
// one index whose s lies below s + margin' (margin' = 1.0625 x assign_mfma's margin, which covers
// the rounding of the sum, so every other s exceeds the winner by more than the margin).  More
// than one such index (a close call, a tie), none (NaN input) or an infinite margin takes the exact
// vector path; so does a non-finite point.  Same proof as assign_mfma.
template <int K>
__device__ __forceinline__ uint32_t pick_mfma(const float (&v)[K], float px, float py, float emul_c2, float emul_x,
                                              float emul_y, const float2 *__restrict__ s_c, const float (&cx)[K],
                                              const float (&cy)[K], float thr, float thr2) {
    float b = v[0];
#pragma unroll
    for (int i = 1; i < K; ++i) b = fminf(b, v[i]);
    const float E = 0x1p-21f * (emul_c2 + 2.0f * (emul_x * fabsf(px) + emul_y * fabsf(py))) + kAbsRound;
    const float P = px * px + py * py;
    const float margin = 2.0f * E + 0x1p-19f * (fabsf(b) + P + E);
    const float lim = b + 1.0625f * margin;
    int cnt = 0, bi = 0;
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        const bool in = v[i] < lim;
        cnt += in ? 1 : 0;
        bi = in ? i : bi;
    }
    if (__builtin_expect(!(cnt == 1 && lim < __builtin_inff()), 0)) return assign_fast<K>(px, py, cx, cy, thr);
    const float2 c = s_c[bi];
    const float dx = __fsub_rn(c.x, px), dy = __fsub_rn(c.y, py);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < thr2 ? (uint32_t)bi : 255u;  // sqrt_rn(d2) < thr
}

constexpr int kF32Unroll = 4;  // 64-point blocks per wave per trip (loads in flight together)

template <int K, bool kMfma, bool kAccumulate>
__global__ void __launch_bounds__(kThreads)
kmeans_f32_fast_kernel(const float2 *__restrict__ xy, int64_t n, const float *__restrict__ cent, int k, float thr,
                       float thr2, double *__restrict__ acc, int n_copies, const KmState *__restrict__ st,
                       uint8_t *__restrict__ labels) {
    if (kAccumulate && st->done) return;
    __shared__ uint32_t s_n[kWaves][K];
    __shared__ double s_sx[kWaves][K], s_sy[kWaves][K];
    __shared__ float2 s_c[K];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float cx[K], cy[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        cx[i] = uniform_f32(i < k ? cent[2 * i] : __builtin_inff());
        cy[i] = uniform_f32(i < k ? cent[2 * i + 1] : __builtin_inff());
    }
    // matrix-engine operands: A rows (lane & 3 = row i of every 4x4 block), |c|^2 per register
    float ax[K / 4], ay[K / 4], c2[K];
    float em_c2 = 0.f, em_x = 0.f, em_y = 0.f;
    if constexpr (kMfma) {
#pragma unroll
        for (int g = 0; g < K / 4; ++g) {
            const int i = 4 * g + (lane & 3);
            const float vx = i < k ? cent[2 * i] : 0.f, vy = i < k ? cent[2 * i + 1] : 0.f;
            ax[g] = -2.0f * vx;
            ay[g] = -2.0f * vy;
        }
#pragma unroll
        for (int i = 0; i < K; ++i) {
            c2[i] = i < k ? __fadd_rn(__fmul_rn(cx[i], cx[i]), __fmul_rn(cy[i], cy[i])) : __builtin_inff();
            if (i < k) {
                em_c2 = fmaxf(em_c2, c2[i]);
                em_x = fmaxf(em_x, fabsf(cx[i]));
                em_y = fmaxf(em_y, fabsf(cy[i]));
            }
        }
    }
    if (tid < K) s_c[tid] = make_float2(tid < k ? cent[2 * tid] : __builtin_inff(), tid < k ? cent[2 * tid + 1] : __builtin_inff());
    if (kAccumulate && lane < K) {
        s_n[wave][lane] = 0u;
        s_sx[wave][lane] = 0.0;
        s_sy[wave][lane] = 0.0;
    }
    __syncthreads();
    const int64_t nblk = (n + 63) / 64;
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t b0 = (int64_t)blockIdx.x * kWaves + wave; b0 < nblk; b0 += stride * kF32Unroll) {
        float2 q[kF32Unroll];
#pragma unroll
        for (int u = 0; u < kF32Unroll; ++u) {  // clamped, unconditional: all loads in flight at once
            const int64_t p = (b0 + u * stride) * 64 + lane;
            q[u] = xy[p < n ? p : n - 1];
        }
#pragma unroll
        for (int u = 0; u < kF32Unroll; u += 2) {
            if (b0 + u * stride >= nblk) break;  // wave-uniform
            uint32_t lab[2];
            if constexpr (kMfma) {
                lab[0] = assign_mfma<K>(q[u].x, q[u].y, ax, ay, c2, em_c2, em_x, em_y, s_c, cx, cy, thr, thr2);
                lab[1] = assign_mfma<K>(q[u + 1].x, q[u + 1].y, ax, ay, c2, em_c2, em_x, em_y, s_c, cx, cy, thr, thr2);
            } else {
                assign_pair<K>(q[u], q[u + 1], cx, cy, s_c, thr, thr2, lab[0], lab[1]);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t blk = b0 + (u + h) * stride;
                if (blk >= nblk) break;  // wave-uniform
                const int64_t p = blk * 64 + lane;
                const uint32_t l = p < n ? lab[h] : 255u;
                if (labels && p < n) labels[p] = (uint8_t)l;
                if (kAccumulate && l < (uint32_t)K) {
                    atomicAdd(&s_n[wave][l], 1u);
                    atomicAdd(&s_sx[wave][l], (double)q[u + h].x);
                    atomicAdd(&s_sy[wave][l], (double)q[u + h].y);
                }
            }
        }
    }
    if (!kAccumulate) return;
    __syncthreads();
    if (tid < 3 * k) {
        const int f = tid / k, c = tid - f * k;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += f == 0 ? (double)s_n[w][c] : (f == 1 ? s_sx[w][c] : s_sy[w][c]);
        if (v != 0.0) atomicAdd(&acc[(int)(blockIdx.x % n_copies) * kAccStride + 3 * c + f], v);
    }
}

// ---- candidate table for the vector engine (k <= 32, 16-B aligned points) ---------------------
// Each Lloyd pass labels every point by the first centre of smallest sqrt_rn(d2); with k = 16
// that is ~105 VALU per point in the screen above, and the pass is VALU-bound (r03j counters:
// 84 M VALU wave-instructions for 50 M points, 71 % busy).  Here a 64 x 64 grid of square cells
// over the points' bounding box holds, per cell and pass, the centres that can win ANYWHERE in
// the cell (computed in fp64 by the update kernel right after the centres move):
//   candidate i  <=>  dmin2_i(cell) <= min_j dmax2_j(cell) * (1 + 2^-12) + 1e-30,
// the cell grown by cs * 2^-12 on each side (covers the fp32 cell-index rounding, < cs * 2^-16).
// A non-candidate's fp32 d2 then exceeds the winner's by more than 2^-13 relative, beyond the
// fp32 rounding of d2 (< 2^-21) and assign_fast's 2^-20 square-root tie band: it can neither win
// nor make the tie test fire, so testing the (at most 3) candidates in ascending index with
// assign_fast's own steps gives assign_fast's label.  A cell whose every point lies beyond the
// threshold (dmin2 > thr2 (1 + 2^-12) for all centres) names a NaN sentinel centre three times
// (d2 NaN: no tie, label 255); more than 3 candidates name an infinite one (d2 = inf: the tie
// test fires).  A point outside the grid (or NaN) and a tie-band hit take assign_fast's steps over
// all centres.  The bounding box comes from a 64 K-point sample (points outside it are only
// slower, never wrong).  An entry holds the three candidates' BYTE offsets into the kernels' LDS
// centre table (10 bits each), so the lookup needs no shifts.
constexpr int kLutSide = 64;
constexpr int kLutCells = kLutSide * kLutSide;
constexpr int kLutBlocks = kLutCells / kThreads;
constexpr int kBoxBlocks = 64, kBoxPerThread = 4;
constexpr int kLutInf = kFastMaxK, kLutNan = kFastMaxK + 1;  // sentinel slots of the centre table
// Candidate slots the assignment tests per point.  With pairwise domination (lut_entry) about 1 %
// of the cells near the centres keep 3 candidates: their points go through the wave's fallback
// queue, which is cheaper than a third distance for every point.
constexpr int kLutSlots = 2;
__host__ __device__ constexpr uint32_t lut_pack(uint32_t a, uint32_t b, uint32_t c) {
    return (a * 8u) | (b * 8u) << 10 | (c * 8u) << 20;
}
constexpr uint32_t kLutFull = lut_pack(kLutInf, kLutInf, kLutInf);
constexpr uint32_t kLutFar = lut_pack(kLutNan, kLutNan, kLutNan);

struct LutGeom {
    float x0, y0, inv_cs, fgx, fgy, cs;
    int32_t gx, gy, ok, pad[7];
};
static_assert(sizeof(LutGeom) == 64, "LutGeom is one 64-B record");

// float -> u32 with the same order (so u32 atomic max gives float max; max of ~u gives the min)
__device__ __forceinline__ uint32_t ordered_u32(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// box[4 b + 0..3] = workgroup b's max ord(x), max ~ord(x), max ord(y), max ~ord(y) over its finite
// sampled points (0 = none); kmeans_update_lut_kernel reduces the kBoxBlocks records.  (One u32
// atomic max per wave into a single record measured 15 us: 1024 same-address atomics.)
__global__ void __launch_bounds__(kThreads)
kmeans_bbox_sample_kernel(const float2 *__restrict__ xy, int64_t n, uint32_t *__restrict__ box) {
    constexpr int64_t kSamples = (int64_t)kBoxBlocks * kThreads * kBoxPerThread;
    __shared__ uint32_t s_r[kThreads / 64][4];
    const int64_t step = n > kSamples ? n / kSamples : 1;
    const int tid = threadIdx.x;
    float2 p[kBoxPerThread + 1];
#pragma unroll
    for (int u = 0; u < kBoxPerThread; ++u) {
        const int64_t j = (((int64_t)blockIdx.x * kThreads + tid) * kBoxPerThread + u) * step;
        p[u] = xy[j < n ? j : n - 1];
    }
    p[kBoxPerThread] = xy[n - 1];  // the last point too
    uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u <= kBoxPerThread; ++u) {
        if (__builtin_isfinite(p[u].x) && __builtin_isfinite(p[u].y)) {
            const uint32_t ox = ordered_u32(p[u].x), oy = ordered_u32(p[u].y);
            r[0] = max(r[0], ox);
            r[1] = max(r[1], ~ox);
            r[2] = max(r[2], oy);
            r[3] = max(r[3], ~oy);
        }
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r[f] = max(r[f], (uint32_t)__shfl_xor((int)r[f], o));
    }
    if ((tid & 63) == 0)
        for (int f = 0; f < 4; ++f) s_r[tid >> 6][f] = r[f];
    __syncthreads();
    if (tid < 4) {
        uint32_t v = 0u;
        for (int w = 0; w < kThreads / 64; ++w) v = max(v, s_r[w][tid]);
        box[4 * blockIdx.x + tid] = v;
    }
}

// The grid over the sampled box (deterministic: every launch derives the same record).
__device__ inline LutGeom lut_geometry(const uint32_t (&box)[4]) {
    LutGeom g{};
    g.ok = 0;
    if (box[0] == 0u) return g;
    const float xmax = from_ordered(box[0]), xmin = from_ordered(~box[1]);
    const float ymax = from_ordered(box[2]), ymin = from_ordered(~box[3]);
    const double mag = fmax(fmax(fabs((double)xmin), fabs((double)xmax)), fmax(fabs((double)ymin), fabs((double)ymax)));
    if (!(mag < 1e18)) return g;  // keeps every candidate's fp32 d2 finite
    const double w = (double)xmax - xmin, h = (double)ymax - ymin;
    double cs = fmax(w, h) / kLutSide * (1.0 + 0x1p-10);
    cs = fmax(cs, fmax(mag * 0x1p-20, 1e-12));
    g.cs = (float)cs;
    g.inv_cs = __fdiv_rn(1.0f, g.cs);
    g.gx = min(kLutSide, (int)(w / (double)g.cs) + 1);
    g.gy = min(kLutSide, (int)(h / (double)g.cs) + 1);
    g.x0 = xmin;
    g.y0 = ymin;
    g.fgx = (float)g.gx;
    g.fgy = (float)g.gy;
    g.ok = 1;
    return g;
}

// One cell's entry: the candidates (ascending, padded with the last) as lut_pack offsets,
// kLutFar when no point of the cell can be within the threshold, kLutFull past 3 candidates.
__device__ inline uint32_t lut_entry(int ix, int iy, const LutGeom &g, const float2 *__restrict__ s_c, int k,
                                     float thr2) {
    const double cs = g.cs, e = cs * 0x1p-12;
    const double x0 = (double)g.x0 + ix * cs - e, x1 = (double)g.x0 + (ix + 1) * cs + e;
    const double y0 = (double)g.y0 + iy * cs - e, y1 = (double)g.y0 + (iy + 1) * cs + e;
    auto dmin2 = [&](float2 c) {
        const double dx = fmax(fmax(x0 - c.x, c.x - x1), 0.0), dy = fmax(fmax(y0 - c.y, c.y - y1), 0.0);
        return dx * dx + dy * dy;
    };
    double best = __builtin_inf(), near = __builtin_inf();
    for (int i = 0; i < k; ++i) {
        const float2 c = s_c[i];
        const double dx = fmax(fabs(c.x - x0), fabs(c.x - x1)), dy = fmax(fabs(c.y - y0), fabs(c.y - y1));
        best = fmin(best, dx * dx + dy * dy);
        near = fmin(near, dmin2(c));
    }
    // every point beyond the threshold: 255 whatever the candidates (far from all centres, many
    // of them are nearly equidistant, so such cells would otherwise overflow)
    if (near > (double)thr2 * (1.0 + 0x1p-12) + 1e-30) return kLutFar;
    const double bound = best * (1.0 + 0x1p-12) + 1e-30;
    constexpr int kPre = 4;
    int pre[kPre] = {0, 0, 0, 0};
    int np = 0;
    for (int i = 0; i < k; ++i) {
        if (dmin2(s_c[i]) <= bound) {
            pre[np < kPre ? np : kPre - 1] = np < kPre ? i : pre[kPre - 1];
            ++np;
        }
    }
    if (np == 0 || np > kPre) return kLutFull;  // (none: non-finite centres) -> all centres
    // Pairwise domination (the bound above is per centre): i cannot win in the cell if some other
    // candidate j has d_i^2 > (1 + 2^-12) d_j^2 + 1e-30 at every point of it.  d_i^2 - (1+eps) d_j^2
    // is concave in the point (its quadratic part is -eps |p|^2), so its minimum over the cell is
    // at a corner: four evaluations decide.  A pruned centre then stays 2^-13 above the winner, as
    // the per-centre bound guarantees.  This leaves 1-2 candidates in nearly every cell (the bound
    // alone left 4+ near Voronoi vertices).  Fixed-size, fully unrolled (register arrays).
    double dc[kPre][4];
#pragma unroll
    for (int a = 0; a < kPre; ++a) {
        const float2 c = s_c[pre[a]];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double dx = c.x - ((q & 1) ? x1 : x0), dy = c.y - ((q & 2) ? y1 : y0);
            dc[a][q] = dx * dx + dy * dy;
        }
    }
    uint32_t keep = (1u << np) - 1u;
#pragma unroll
    for (int a = 0; a < kPre; ++a) {
#pragma unroll
        for (int b = 0; b < kPre; ++b) {
            if (a == b) continue;
            bool dom = a < np && b < np;
#pragma unroll
            for (int q = 0; q < 4; ++q) dom = dom && (dc[a][q] - (1.0 + 0x1p-12) * dc[b][q] > 1e-30);
            keep &= dom ? ~(1u << a) : ~0u;
        }
    }
    uint32_t cand[3] = {0u, 0u, 0u};
    int cnt = 0;
#pragma unroll
    for (int a = 0; a < kPre; ++a) {
        if (keep >> a & 1u) {
            if (cnt < 3) cand[cnt] = (uint32_t)pre[a];
            ++cnt;
        }
    }
    if (cnt == 0 || cnt > kLutSlots) return kLutFull;
    if (cnt < 2) cand[1] = cand[0];
    return lut_pack(cand[0], cand[1], cand[1]);
}

// Centroid update fused with the candidate table.  kLutBlocks workgroups each sum the replicas
// (the same fp64 arithmetic as kmeans_update_kernel), keep the new centres in LDS and build 256
// cells; workgroup 0 writes the centres and the state.  Accumulators ping-pong between two sets:
// this launch reads acc_rd and zeroes acc_zero (read by the previous update), so no workgroup
// zeroes what another still reads.  iter < 0: table for the current centres only (before pass 0;
// also writes the grid record).  st->done holds iter + 1 of the converging update, so workgroups
// of that same launch still build its table.
__global__ void __launch_bounds__(kThreads)
kmeans_update_lut_kernel(const double *__restrict__ acc_rd, double *__restrict__ acc_zero, int n_copies,
                         float *__restrict__ cent, int k, float tol, KmState *__restrict__ st, int iter,
                         const uint32_t *__restrict__ box, LutGeom *__restrict__ geom, uint32_t *__restrict__ lut,
                         float thr2) {
    if (iter >= 0) {
        const int d = __builtin_amdgcn_readfirstlane(st->done);
        if (d != 0 && d <= iter) return;
    }
    __shared__ float2 s_c[kFastMaxK];
    __shared__ LutGeom s_g;
    const int tid = threadIdx.x;
    if (tid >= 64 && tid < 128) {  // wave 1: the grid record (reduced from the samples before pass 0)
        if (iter < 0) {
            const int l = tid - 64;
            uint32_t r[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                r[f] = l < kBoxBlocks ? box[4 * l + f] : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) r[f] = max(r[f], (uint32_t)__shfl_xor((int)r[f], o));
            }
            if (l == 0) {
                s_g = lut_geometry(r);
                if (blockIdx.x == 0) *geom = s_g;
            }
        } else if (tid == 64) {
            s_g = *geom;
        }
    }
    if (iter >= 0) {
        const int z = blockIdx.x * kThreads + tid;
        if (z < n_copies * kAccStride) acc_zero[z] = 0.0;
    }
    if (tid < 64) {  // wave 0: centres (k <= 32 lanes) and, in workgroup 0, the state
        float shift = 0.f;
        if (tid < k) {
            const float ox = cent[2 * tid], oy = cent[2 * tid + 1];
            float nx = ox, ny = oy;
            if (iter >= 0) {
                double a[3] = {0.0, 0.0, 0.0}, v[kAccCopies][3];
#pragma unroll
                for (int r = 0; r < kAccCopies; ++r)
#pragma unroll
                    for (int f = 0; f < 3; ++f) v[r][f] = r < n_copies ? acc_rd[r * kAccStride + 3 * tid + f] : 0.0;
#pragma unroll
                for (int r = 0; r < kAccCopies; ++r)
#pragma unroll
                    for (int f = 0; f < 3; ++f) a[f] += v[r][f];
                if (a[0] > 0.0) {
                    nx = (float)(a[1] / a[0]);
                    ny = (float)(a[2] / a[0]);
                    shift = fmaxf(fabsf(nx - ox), fabsf(ny - oy));
                    if (blockIdx.x == 0) {
                        cent[2 * tid] = nx;
                        cent[2 * tid + 1] = ny;
                    }
                }
            }
            s_c[tid] = make_float2(nx, ny);
        }
        if (iter >= 0 && blockIdx.x == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) shift = fmaxf(shift, __shfl_xor(shift, o));
            if (tid == 0) {
                st->iters += 1;
                if (tol >= 0.f && shift <= tol) st->done = iter + 1;
            }
        }
    }
    __syncthreads();
    const LutGeom g = s_g;
    if (!g.ok) return;
    const int c = blockIdx.x * kThreads + tid;
    if (c < g.gx * g.gy) lut[c] = lut_entry(c % g.gx, c / g.gx, g, s_c, k, thr2);
}

// What the assignment kernels need of the grid record.
struct LutView {
    float x0, y0, inv_cs, fgx_m, fgy_m;  // fgx_m: the largest float below the column count
    int32_t gx4;                          // row stride of the table in bytes
};

// assign_fast's steps with the centres read from LDS (the table kernels keep no centres in
// registers; this is their rare fallback)
template <int K>
__device__ __forceinline__ uint32_t assign_lds2(float px, float py, const float2 *__restrict__ s_c, float thr) {
    float m = __builtin_inff(), m_prev = __builtin_inff();
    int ia = 0;
#pragma unroll 4
    for (int i = 0; i < K; ++i) {
        const float2 c = s_c[i];
        const float dx = __fsub_rn(c.x, px), dy = __fsub_rn(c.y, py);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
        const bool lt = d2 < m;
        m_prev = lt ? m : m_prev;
        ia = lt ? i : ia;
        m = lt ? d2 : m;
    }
    if (m_prev <= __fmul_rn(m, 1.0f + 0x1p-20f)) {
        uint32_t best = 255u;
        float best_s = thr;
        for (int i = 0; i < K; ++i) {
            const float2 c = s_c[i];
            const float dx = __fsub_rn(c.x, px), dy = __fsub_rn(c.y, py);
            const float sd = ecc::sqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            if (sd < best_s) { best_s = sd; best = (uint32_t)i; }
        }
        return best;
    }
    return ecc::sqrt_rn(m) < thr ? (uint32_t)ia : 255u;
}

// One point through the table: assign_fast's steps over the cell's kLutSlots candidates.  full =
// the caller must take the steps over all centres (outside the grid, > 3 candidates, or a
// tie-band hit).  ~33 VALU per point: med3 clamps the cell coordinates and tells inside from
// outside in one compare, the entry's byte offsets address the centre table directly, and the
// first candidate seeds the running minimum (a real candidate's d2 is finite; the sentinels' inf /
// NaN propagate as described above).
__device__ __forceinline__ uint32_t lut_point(float px, float py, const LutView &g, const uint32_t *__restrict__ s_lut,
                                              const float2 *__restrict__ s_c, float thr2, bool &full) {
    const float tx = __fmul_rn(__fsub_rn(px, g.x0), g.inv_cs), ty = __fmul_rn(__fsub_rn(py, g.y0), g.inv_cs);
    const float cxf = __builtin_amdgcn_fmed3f(tx, 0.f, g.fgx_m), cyf = __builtin_amdgcn_fmed3f(ty, 0.f, g.fgy_m);
    const bool inside = (cxf == tx) & (cyf == ty);  // false for NaN
    const uint32_t a = __umul24((uint32_t)(int)cyf, (uint32_t)g.gx4) + ((uint32_t)(int)cxf << 2);
    const uint32_t e = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s_lut) + a);
    const uint32_t o0 = e & 0x3ffu, o1 = (e >> 10) & 0x3ffu;
    const char *cb = reinterpret_cast<const char *>(s_c);
    const float2 c0 = *reinterpret_cast<const float2 *>(cb + o0);
    const float2 c1 = *reinterpret_cast<const float2 *>(cb + o1);
    auto d2 = [&](float2 c) {
        const float dx = __fsub_rn(c.x, px), dy = __fsub_rn(c.y, py);
        return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
    };
    float m = d2(c0), m_prev = __builtin_inff();
    uint32_t ia = o0;
    {
        const float d = d2(c1);
        const bool lt = d < m;
        m_prev = lt ? m : m_prev;
        ia = lt ? o1 : ia;
        m = lt ? d : m;
    }
    full = !inside | (m_prev <= __fmul_rn(m, 1.0f + 0x1p-20f));
    return m < thr2 ? ia >> 3 : 255u;
}

// Vector engine, streaming form: a lane takes two consecutive points per 16-B load (the pair the
// packed screen tests together), kPairUnroll such loads per trip, and the NEXT trip's loads are
// issued before this trip's tests, so a wave keeps 2 x kPairUnroll x 16 B in flight across its
// compute (the one-trip form waited on its loads every trip: bound by bytes in flight, ~2.2 TB/s).
// The pair's two labels go out as one 2-byte store.  Needs 16-B aligned points (and labels 2-B
// aligned); an odd last point is taken by lane 0 of workgroup 0.
constexpr int kPairUnroll = 4;

template <int K, bool kAccumulate, bool kLut, bool kMfma = false>
__global__ void __launch_bounds__(kThreads, kMfma ? ECC_KM_MFMA_WAVES : 1)
kmeans_f32_pair_kernel(const float4 *__restrict__ xy4, int64_t n, const float *__restrict__ cent, int k, float thr,
                       float thr2, double *__restrict__ acc, int n_copies, const KmState *__restrict__ st,
                       uint8_t *__restrict__ labels, const LutGeom *__restrict__ geom,
                       const uint32_t *__restrict__ lut) {
    if (kAccumulate && st->done) return;
    // accumulator slots per wave, kSub copies (lane % kSub) to spread same-address LDS atomics
    constexpr int kSub = ECC_KM_ACC_SUB;
    __shared__ uint32_t s_n[kWaves * kSub][K];
    __shared__ double s_sx[kWaves * kSub][K], s_sy[kWaves * kSub][K];
    __shared__ float2 s_c[kLut ? kFastMaxK + 2 : K];  // + the table's inf and NaN sentinels
    __shared__ __attribute__((aligned(16))) uint32_t s_lut[kLut ? kLutCells : 4];
    __shared__ float4 s_q[kWaves][kLut ? 128 : 1];  // fallback queues: < 64 + 64 entries
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // The grid record as scalars (a struct copy of the 64-B record went to the stack).  Without a
    // grid (non-finite or huge box) every point is outside: fgx = 0, one cell, assign_lds2.
    LutView g{};
    if constexpr (kLut) {
        const bool ok = geom->ok != 0;
        g.x0 = geom->x0;
        g.y0 = geom->y0;
        g.inv_cs = geom->inv_cs;
        if (!ok) g.inv_cs = __builtin_nanf("");  // no grid: every point is outside (NaN compares false)
        g.fgx_m = ok ? __uint_as_float(__float_as_uint(geom->fgx) - 1u) : 0.f;  // fgx >= 1
        g.fgy_m = ok ? __uint_as_float(__float_as_uint(geom->fgy) - 1u) : 0.f;
        g.gx4 = ok ? 4 * geom->gx : 4;
        if (tid == kLutInf) s_c[kLutInf] = make_float2(__builtin_inff(), __builtin_inff());
        if (tid == kLutNan) s_c[kLutNan] = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        // the table into LDS: all of a lane's 16-B loads in flight at once (a strided word loop
        // paid one L2 round trip per word, at the start of every workgroup)
        const __amdgpu_buffer_rsrc_t v = ecc::buffer_view(lut, ok ? (uint32_t)(geom->gx * geom->gy) * 4u : 0u);
        uint4 q[kLutCells / (4 * kThreads)];
#pragma unroll
        for (int u = 0; u < kLutCells / (4 * kThreads); ++u)
            q[u] = ecc::buffer_load_u128(v, (uint32_t)tid * 16u, (uint32_t)(u * kThreads * 16));
#pragma unroll
        for (int u = 0; u < kLutCells / (4 * kThreads); ++u)
            reinterpret_cast<uint4 *>(s_lut)[u * kThreads + tid] = q[u];
        if (!ok && tid == 0) s_lut[0] = kLutFull;
    }
    float cx[K], cy[K];  // the screen's centres in scalar registers (not with the table)
    if constexpr (!kLut) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            cx[i] = uniform_f32(i < k ? cent[2 * i] : __builtin_inff());
            cy[i] = uniform_f32(i < k ? cent[2 * i + 1] : __builtin_inff());
        }
    }
    // matrix-engine operands (kMfma): this lane's A element, |c_r|^2 as the C input, error scales
    float a_ev = 0.f, a_od = 0.f, em_c2 = 0.f, em_x = 0.f, em_y = 0.f;
    floatx16_t c2v{};
    if constexpr (kMfma) {
        static_assert(K == 16, "the 32x32x2 layout maps D register r to centre r < 16");
        const int i = lane & 31, c = (i & 3) | ((i >> 3) << 2);
        const float a_op = c < k ? -2.0f * cent[2 * c + (lane >> 5)] : 0.f;
        // rows (i & 4) == 0 are lanes 0-31's D rows, the others lanes 32-63's: the even points'
        // instruction fills the first, the odd points' (chained on its output) the second
        a_ev = (i & 4) ? 0.f : a_op;
        a_od = (i & 4) ? a_op : 0.f;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            c2v[r] = r < k ? __fadd_rn(__fmul_rn(cx[r], cx[r]), __fmul_rn(cy[r], cy[r])) : __builtin_inff();
            if (r < k) {
                em_c2 = fmaxf(em_c2, c2v[r]);
                em_x = fmaxf(em_x, fabsf(cx[r]));
                em_y = fmaxf(em_y, fabsf(cy[r]));
            }
        }
    }
    if (tid < K) s_c[tid] = make_float2(tid < k ? cent[2 * tid] : __builtin_inff(), tid < k ? cent[2 * tid + 1] : __builtin_inff());
    if (kAccumulate && lane < K) {
        for (int b = 0; b < kSub; ++b) {
            s_n[wave * kSub + b][lane] = 0u;
            s_sx[wave * kSub + b][lane] = 0.0;
            s_sy[wave * kSub + b][lane] = 0.0;
        }
    }
    const int slot = wave * kSub + lane % kSub;
    __syncthreads();
    auto account = [&](float2 q, uint32_t l) __attribute__((always_inline)) {
        if (kAccumulate && l < (uint32_t)K) {
            atomicAdd(&s_n[slot][l], 1u);
            atomicAdd(&s_sx[slot][l], (double)q.x);
            atomicAdd(&s_sy[slot][l], (double)q.y);
        }
    };
    const int64_t npair = n / 2;
    const int64_t nblk = (npair + 63) / 64;  // 64 pairs per wave block
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    // table path: loads per trip (8 measured slower than 4: 117 vs 110 us per accumulate pass)
    // matrix engine: each lane loads the pairs of lanes (lane & 31) and (lane & 31) + 32 of a block
    // (the two column sets of its two instruction pairs; the duplicate addresses coalesce)
    constexpr int kBlk = kMfma ? ECC_KM_MFMA_BLOCKS : (kLut ? ECC_KM_LUT_UNROLL : kPairUnroll);  // blocks per trip
    constexpr int kU = kMfma ? 2 * kBlk : kBlk;  // 16-B loads per lane per trip
    const int64_t span = stride * kBlk;
    // a trip's loads through a buffer view based at its first pair: unconditional (0 past the
    // last pair), one VGPR of lane offset for all of them, the u part in the scalar offset
    auto load = [&](int64_t b0, float4 (&q)[kU]) __attribute__((always_inline)) {
        const int64_t first = b0 * 64 < npair ? b0 * 64 : npair;
        const int64_t rem = (npair - first) * 16;
        const __amdgpu_buffer_rsrc_t v = ecc::buffer_view(xy4 + first, rem < 0xffffffffll ? (uint32_t)rem : 0xffffffffu);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t lo = kMfma ? (uint32_t)(lane & 31) * 16u + (uint32_t)(u & 1) * 512u : (uint32_t)lane * 16u;
            const uint4 w = ecc::buffer_load_u128(v, lo, (uint32_t)((kMfma ? u >> 1 : u) * stride * 64 * 16));
            q[u] = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
        }
    };
    // Fallback queue of this wave (table path): points the table cannot decide (outside the grid,
    // > kLutSlots candidates, a tie-band hit) are appended with their index and labelled 64 at a
    // time by assign_lds2 with every lane busy, instead of one divergent round per trip.  The
    // queue is wave-private LDS; a wave's LDS operations execute in order, so only the compiler
    // is fenced.  A queued point's byte label is stored after the trip's 2-byte store of its pair.
    uint32_t qn = 0;  // wave-uniform fill
    auto drain = [&](uint32_t cnt) __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t i = qn - cnt + (uint32_t)lane;
        if ((uint32_t)lane < cnt) {
            const float4 e = s_q[wave][i];
            const float2 q2 = make_float2(e.x, e.y);
            const uint32_t l = assign_lds2<K>(q2.x, q2.y, s_c, thr);
            const int64_t idx = (int64_t)__float_as_uint(e.z) | ((int64_t)__float_as_uint(e.w) << 32);
            if (labels) labels[idx] = (uint8_t)l;
            account(q2, l);
        }
        qn -= cnt;
        __builtin_amdgcn_wave_barrier();
    };
    auto enqueue = [&](float2 p0, float2 p1, int64_t pp, bool f0, bool f1) __attribute__((always_inline)) {
        if constexpr (kLut) {
            const uint64_t m0 = __ballot(f0), m1 = __ballot(f1);
            if ((m0 | m1) == 0ull) return;  // uniform
            const uint32_t n0 = (uint32_t)__popcll(m0);
            const uint64_t below = lanes_below_mask(lane);
            auto put = [&](uint32_t slot, float2 pt, int64_t idx) {
                s_q[wave][slot] = make_float4(pt.x, pt.y, __uint_as_float((uint32_t)idx),
                                              __uint_as_float((uint32_t)((uint64_t)idx >> 32)));
            };
            // one half at a time with a drain check between: the queue never holds 128 entries
            if (f0) put(qn + (uint32_t)__popcll(m0 & below), p0, 2 * pp);
            qn += n0;
            if (qn >= 64u) drain(64u);
            if (f1) put(qn + (uint32_t)__popcll(m1 & below), p1, 2 * pp + 1);
            qn += (uint32_t)__popcll(m1);
            if (qn >= 64u) drain(64u);
        }
    };
    auto test = [&](int64_t b0, const float4 (&q)[kU]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < kBlk; ++u) {
            const int64_t blk = b0 + u * stride;
            if (blk >= nblk) break;  // wave-uniform
            if constexpr (kMfma) {
                // set h = the pairs 32h..32h+31 of the block, in both halves of the wave
                const bool low = lane < 32;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int src = (lane & 31) + 32 * h;
                    const float4 qs = q[2 * u + h];
                    const float sx = qs.x, sy = qs.y, sz = qs.z, sw = qs.w;
                    // even points into lanes 0-31's rows (lanes 32-63 keep C), then the odd points
                    // into lanes 32-63's rows with the first result as C (lanes 0-31 add fma(0, b)
                    // terms: unchanged, or NaN for a non-finite odd point -> the exact path)
                    const floatx16_t de = __builtin_amdgcn_mfma_f32_32x32x2f32(a_ev, low ? sx : sy, c2v, 0, 0, 0);
                    const floatx16_t dd = __builtin_amdgcn_mfma_f32_32x32x2f32(a_od, low ? sz : sw, de, 0, 0, 0);
                    float v[K];
#pragma unroll
                    for (int r = 0; r < K; ++r) v[r] = dd[r];
                    const float px = low ? sx : sz, py = low ? sy : sw;  // lanes 0-31: even, 32-63: odd point
                    const uint32_t l = pick_mfma<K>(v, px, py, em_c2, em_x, em_y, s_c, cx, cy, thr, thr2);
                    const int64_t pq = blk * 64 + src;
                    if (pq < npair) {
                        if (labels) labels[2 * pq + (low ? 0 : 1)] = (uint8_t)l;
                        account(make_float2(px, py), l);
                    }
                }
                continue;
            }
            const int64_t pp = blk * 64 + lane;
            const float2 p0 = make_float2(q[u].x, q[u].y), p1 = make_float2(q[u].z, q[u].w);
            uint32_t l0, l1;
            bool f0 = false, f1 = false;
            if constexpr (kLut) {
                l0 = lut_point(p0.x, p0.y, g, s_lut, s_c, thr2, f0);
                l1 = lut_point(p1.x, p1.y, g, s_lut, s_c, thr2, f1);
                f0 = f0 && pp < npair;
                f1 = f1 && pp < npair;
            } else {
                assign_pair<K>(p0, p1, cx, cy, s_c, thr, thr2, l0, l1);
            }
            if (pp < npair) {
                if (labels) reinterpret_cast<uint16_t *>(labels)[pp] = (uint16_t)(l0 | l1 << 8);
                if (!f0) account(p0, l0);
                if (!f1) account(p1, l1);
            }
            // after the pair's store: a drain rewrites the queued points' bytes
            if constexpr (kLut) enqueue(p0, p1, pp, f0, f1);
        }
    };
    // Two buffers in ping-pong with unconditional (clamped) loads: no register copies between
    // trips and no branch around the loads, so the wait before each trip's tests covers only
    // that trip's own loads while the other buffer's are in flight.
    float4 qa[kU], qb[kU];
    int64_t b0 = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(wave);  // uniform: scalar descriptors
    if (npair > 0 && b0 < nblk) {
        load(b0, qa);
        for (;;) {
            load(b0 + span, qb);
            test(b0, qa);
            b0 += span;
            if (b0 >= nblk) break;  // wave-uniform
            load(b0 + span, qa);
            test(b0, qb);
            b0 += span;
            if (b0 >= nblk) break;
        }
    }
    if constexpr (kLut) {
        if (qn) drain(qn);
    }
    if ((n & 1) && blockIdx.x == 0 && tid == 0) {  // the odd last point
        const float2 q = reinterpret_cast<const float2 *>(xy4)[n - 1];
        uint32_t l;
        if constexpr (kLut) l = assign_lds2<K>(q.x, q.y, s_c, thr);
        else l = assign_fast<K>(q.x, q.y, cx, cy, thr);
        if (labels) labels[n - 1] = (uint8_t)l;
        account(q, l);
    }
    if (!kAccumulate) return;
    __syncthreads();
    if (tid < 3 * k) {
        const int f = tid / k, c = tid - f * k;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves * kSub; ++w) v += f == 0 ? (double)s_n[w][c] : (f == 1 ? s_sx[w][c] : s_sy[w][c]);
        if (v != 0.0) atomicAdd(&acc[(int)(blockIdx.x % n_copies) * kAccStride + 3 * c + f], v);
    }
}

template <bool kAccumulate>
bool launch_f32_fast(int k, int method, dim3 grid, hipStream_t s, const float *xy, int64_t n, const float *cent,
                     float thr, double *acc, int n_copies, const KmState *st, uint8_t *labels,
                     const LutGeom *geom = nullptr, const uint32_t *lut = nullptr) {
    const float thr2 = sqrt_threshold(thr);
    if (k > kFastMaxK) return false;
    const float2 *p = reinterpret_cast<const float2 *>(xy);
    const float4 *p4 = reinterpret_cast<const float4 *>(xy);
    using std::false_type;
    using std::true_type;
    auto fast = [&](auto K, auto mfma) {
        hipLaunchKernelGGL((kmeans_f32_fast_kernel<decltype(K)::value, decltype(mfma)::value, kAccumulate>), grid,
                           dim3(kThreads), 0, s, p, n, cent, k, thr, thr2, acc, n_copies, st, labels);
    };
    auto pair = [&](auto K, auto table, auto mfma) {
        hipLaunchKernelGGL((kmeans_f32_pair_kernel<decltype(K)::value, kAccumulate, decltype(table)::value,
                                                   decltype(mfma)::value>),
                           grid, dim3(kThreads), 0, s, p4, n, cent, k, thr, thr2, acc, n_copies, st, labels, geom, lut);
    };
    // 16-B loads of point pairs, 2-B stores of label pairs
    const bool pairs_ok = (reinterpret_cast<uintptr_t>(xy) & 15) == 0 && (reinterpret_cast<uintptr_t>(labels) & 1) == 0;
    if (method == 3 && k <= 16 && pairs_ok)  // matrix engine, 32x32x2 streaming form
        pair(std::integral_constant<int, 16>{}, false_type{}, true_type{});
    else if (method >= 2)  // matrix engine, 4x4x1 form (also engine 3's k > 16 / unaligned case)
        dispatch_k(k, [&](auto K) { fast(K, true_type{}); });
    else if (pairs_ok && geom)
        dispatch_k(k, [&](auto K) { pair(K, true_type{}, false_type{}); });
    else if (pairs_ok)
        dispatch_k(k, [&](auto K) { pair(K, false_type{}, false_type{}); });
    else
        dispatch_k(k, [&](auto K) { fast(K, false_type{}); });
    return true;
}

}  // namespace

static int kmeans_run_f32_impl(ecc_ctx *ctx, const float *xy, int64_t n_points, const ecc_kmeans_cfg *cfg,
                               int method, float *centroids, uint8_t *labels, int32_t *iters_out, ecc_stream_t stream) {
    int rc = kmeans_check(ctx, cfg, centroids);
    if (rc) return rc;
    if (n_points < 0 || (n_points > 0 && !xy) || method < 0 || method > 3) return ECC_ERR_INVALID;
    if (method != 0 && cfg->k > kFastMaxK) return ECC_ERR_INVALID;  // the engines take k <= 32
    if ((reinterpret_cast<uintptr_t>(xy) & 7) != 0) return ECC_ERR_INVALID;  // float2 loads
    const bool fast = cfg->k <= kFastMaxK;
    const int n_copies = fast ? kAccCopies : 1;
    const int eng = method == 0 ? 1 : method;  // auto = the vector engine (measured faster)
    // the vector engine's pair kernel (16-B aligned points) runs on the candidate table
    const bool use_lut = fast && eng == 1 && n_points > 0 && (reinterpret_cast<uintptr_t>(xy) & 15) == 0;
    const size_t acc_bytes = (size_t)n_copies * kAccStride * 8;
    // workspace: accumulator set 0 | set 1 (the table path ping-pongs) | state | box | grid | table
    const size_t st_off = 2 * acc_bytes, box_off = st_off + 64, geom_off = box_off + 16 * kBoxBlocks, lut_off = geom_off + 64;
    const size_t ws_bytes = lut_off + (size_t)kLutCells * 4;
    rc = ecc::ws_reserve(ctx, ws_bytes);
    if (rc) return rc;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    char *ws = reinterpret_cast<char *>(ctx->ws);
    auto *acc = reinterpret_cast<double *>(ws);
    auto *st = reinterpret_cast<KmState *>(ws + st_off);
    auto *box = reinterpret_cast<uint32_t *>(ws + box_off);
    auto *geom = reinterpret_cast<LutGeom *>(ws + geom_off);
    auto *lut = reinterpret_cast<uint32_t *>(ws + lut_off);
    ECC_CHECK_HIP(ctx, hipMemsetAsync(ctx->ws, 0, box_off, s), "memset(kmeans acc)");
    const char *name = eng == 3 ? "kmeans_f32_mfma32_kernel" : eng == 2 ? "kmeans_f32_mfma_kernel" : "kmeans_f32_vec_kernel";
    const int grid = fast ? (int)std::max<int64_t>(1, std::min<int64_t>((n_points + 255) / 256, 4096))
                          : grid_for((n_points + kThreads - 1) / kThreads);
    const float thr2 = sqrt_threshold(cfg->threshold);
    if (use_lut) {
        {
            ECC_TIMED(ctx, s, "kmeans_bbox_sample_kernel");
            hipLaunchKernelGGL(kmeans_bbox_sample_kernel, dim3(kBoxBlocks), dim3(kThreads), 0, s,
                               reinterpret_cast<const float2 *>(xy), n_points, box);
        }
        {
            ECC_TIMED(ctx, s, "kmeans_update_lut_kernel");
            hipLaunchKernelGGL(kmeans_update_lut_kernel, dim3(kLutBlocks), dim3(kThreads), 0, s, acc, acc, n_copies,
                               centroids, cfg->k, cfg->tol, st, -1, box, geom, lut, thr2);
        }
        // one round of resident workgroups, as many per CU as registers and LDS allow (a
        // latency-bound stream: the labels pass took 104 us at four per CU, 93 at five): the
        // accumulate pass 5 (k <= 16: 86 VGPRs, 30 KB) or 4 (k <= 32: 35 KB of slots and table),
        // the labels pass 6 (80 VGPRs, 25 KB)
        auto rgrid = [&](int per_cu) {
            return (int)std::max<int64_t>(1, std::min<int64_t>((n_points + 255) / 256, (int64_t)per_cu * ctx->n_cu));
        };
        const int lgrid = rgrid(cfg->k <= 16 ? ECC_KM_LUT_WG_PER_CU : 4);
        const int lgrid_lab = rgrid(ECC_KM_LAB_WG_PER_CU);
        for (int it = 0; it < cfg->max_iters; ++it) {
            double *acc_it = acc + (size_t)(it & 1) * n_copies * kAccStride;
            double *acc_next = acc + (size_t)((it + 1) & 1) * n_copies * kAccStride;
            {
                ECC_TIMED(ctx, s, name);
                launch_f32_fast<true>(cfg->k, eng, dim3(lgrid), s, xy, n_points, centroids, cfg->threshold, acc_it,
                                      n_copies, st, nullptr, geom, lut);
            }
            {
                ECC_TIMED(ctx, s, "kmeans_update_lut_kernel");
                hipLaunchKernelGGL(kmeans_update_lut_kernel, dim3(kLutBlocks), dim3(kThreads), 0, s, acc_it,
                                   acc_next, n_copies, centroids, cfg->k, cfg->tol, st, it, box, geom, lut, thr2);
            }
        }
        ECC_CHECK_LAUNCH(ctx, "kmeans_f32 iteration");
        if (labels) {
            {
                ECC_TIMED(ctx, s, "kmeans_f32_labels");
                const bool lab_ok = (reinterpret_cast<uintptr_t>(labels) & 1) == 0;
                launch_f32_fast<false>(cfg->k, eng, dim3(lab_ok ? lgrid_lab : grid), s, xy, n_points, centroids, cfg->threshold, nullptr,
                                       1, st, labels, lab_ok ? geom : nullptr, lut);
            }
            ECC_CHECK_LAUNCH(ctx, "kmeans_f32 labels");
        }
        if (iters_out)
            ECC_CHECK_HIP(ctx, hipMemcpyAsync(iters_out, &st->iters, 4, hipMemcpyDeviceToDevice, s), "copy iters");
        return ECC_OK;
    }
    for (int it = 0; it < cfg->max_iters && n_points > 0; ++it) {
        {
            ECC_TIMED(ctx, s, fast ? name : "kmeans_f32_kernel");
            if (!launch_f32_fast<true>(cfg->k, eng, dim3(grid), s, xy, n_points, centroids, cfg->threshold, acc,
                                       n_copies, st, nullptr))
                hipLaunchKernelGGL(kmeans_f32_kernel<true>, dim3(grid), dim3(kThreads), 0, s, xy, n_points,
                                   centroids, cfg->k, cfg->threshold, acc, st, (uint8_t *)nullptr);
        }
        {
            ECC_TIMED(ctx, s, "kmeans_update_kernel");
            hipLaunchKernelGGL(kmeans_update_kernel<double>, dim3(1), dim3(64), 0, s, acc, n_copies, centroids,
                               cfg->k, cfg->tol, st);
        }
    }
    ECC_CHECK_LAUNCH(ctx, "kmeans_f32 iteration");
    if (labels && n_points > 0) {
        {
            ECC_TIMED(ctx, s, "kmeans_f32_labels");
            if (!launch_f32_fast<false>(cfg->k, eng, dim3(grid), s, xy, n_points, centroids, cfg->threshold,
                                        nullptr, 1, st, labels))
                hipLaunchKernelGGL(kmeans_f32_kernel<false>, dim3(grid), dim3(kThreads), 0, s, xy, n_points,
                                   centroids, cfg->k, cfg->threshold, acc, st, labels);
        }
        ECC_CHECK_LAUNCH(ctx, "kmeans_f32 labels");
    }
    if (iters_out)
        ECC_CHECK_HIP(ctx, hipMemcpyAsync(iters_out, &st->iters, 4, hipMemcpyDeviceToDevice, s),
                      "copy iters");
    return ECC_OK;
}

ECC_API int ecc_kmeans_run_f32(ecc_ctx *ctx, const float *xy, int64_t n_points,
                               const ecc_kmeans_cfg *cfg, float *centroids, uint8_t *labels,
                               int32_t *iters_out, ecc_stream_t stream) {
    return kmeans_run_f32_impl(ctx, xy, n_points, cfg, 0, centroids, labels, iters_out, stream);
}

ECC_API int ecc_kmeans_run_f32_engine(ecc_ctx *ctx, const float *xy, int64_t n_points,
                                      const ecc_kmeans_cfg *cfg, int32_t engine, float *centroids,
                                      uint8_t *labels, int32_t *iters_out, ecc_stream_t stream) {
    return kmeans_run_f32_impl(ctx, xy, n_points, cfg, engine, centroids, labels, iters_out, stream);
}

ECC_API int ecc_kmeans_assign_f32(ecc_ctx *ctx, const float *xy, int64_t n_points,
                                  const float *centroids, int32_t k, float threshold,
                                  uint8_t *labels, ecc_stream_t stream) {
    if (!ctx || !centroids || !labels || k < 1 || k > kMaxK || n_points < 0) return ECC_ERR_INVALID;
    if (n_points == 0) return ECC_OK;
    if (!xy) return ECC_ERR_INVALID;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    const int grid = grid_for((n_points + kThreads - 1) / kThreads);
    {
        ECC_TIMED(ctx, ecc::as_stream(stream), "kmeans_f32_kernel");
        hipLaunchKernelGGL(kmeans_f32_kernel<false>, dim3(grid), dim3(kThreads), 0,
                           ecc::as_stream(stream), xy, n_points, centroids, k, threshold,
                           (double *)nullptr, (const KmState *)nullptr, labels);
    }
    ECC_CHECK_LAUNCH(ctx, "kmeans assign");
    return ECC_OK;
}
