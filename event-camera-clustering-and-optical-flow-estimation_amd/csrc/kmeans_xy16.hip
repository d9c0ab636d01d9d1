// k-means over 2-D event points.
//
// Reference: KM/assign_to_centers.cl — assign_to_centers (:1-34: nearest of 8 centres by
// length((cx-x, cy-y, 0)), strict `<` from threshold 50, uchar 255 = none),
// assign_data_cluster (:36-119: atomic scatter into 8 bins of 2048), reduction_scalar
// (:121-140: 1024-wide tree sums), and the host loop KM/assign_to_centers2.c:184-548
// (buffers re-created every pass, blocking reads, goto restart).
//
// MI355X design ("fixed" mode, Appendix A Q7-Q10):
//   * one fused kernel per iteration: 16-B loads of 4 packed-u16 points per lane, centroids in
//     LDS (broadcast reads), assignment, and per-wave LDS accumulators updated with 64-bit LDS
//     atomics — no scatter pass, no bins, no host round trip;
//   * partial sums are INTEGERS (pixel coordinates): count<<40 | sum_x and sum_y per cluster,
//     flushed with one 64-bit global atomic per (WG, cluster, field) — exact, so the result is
//     independent of reduction order and bit-identical to the fp64 oracle;
//   * a 1-wave update kernel computes c = (float)(sum/n) in fp64, the max shift, and a
//     device-side `done` flag that makes the remaining queued iterations no-ops (no host
//     sync per iteration).
// Assignment arithmetic (canonical, shared with oracle/oracle.cpp assign_one): fp32
// d2 = dx*dx + dy*dy (no FMA contraction), correctly rounded sqrt (ecc::sqrt_rn), the
// reference's first-minimum rule; sqrt only where d2 improves (see assign_point).
// Algorithmic bytes: 4 B/point/iteration (packed u16 xy) + 1 B/point for the final labels.
#include "kmeans_common.hpp"

namespace {

// The labels pointer's own offset, in bytes: packed 4-B label stores are taken where element index
// plus this is a multiple of 4, so labels needs no alignment at all.
__device__ __forceinline__ int64_t label_skew(const uint8_t *labels) {
    return (int64_t)(reinterpret_cast<uintptr_t>(labels) & 3);
}

template <bool kAccumulate>
__global__ void __launch_bounds__(kThreads)
kmeans_xy16_kernel(const uint32_t *__restrict__ xy, Segs segs, const float *__restrict__ cent,
                   int k, float thr, unsigned long long *__restrict__ acc,
                   const KmState *__restrict__ st, uint8_t *__restrict__ labels) {
    if (kAccumulate && st->done) return;
    __shared__ float2 c_lds[kMaxK];
    __shared__ unsigned long long a_xc[kWaves][kMaxK];
    __shared__ unsigned long long a_y[kWaves][kMaxK];
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid < k) c_lds[tid] = make_float2(cent[2 * tid], cent[2 * tid + 1]);
    if (kAccumulate) {
        for (int i = tid; i < kWaves * kMaxK; i += kThreads) {
            (&a_xc[0][0])[i] = 0ull;
            (&a_y[0][0])[i] = 0ull;
        }
    }
    __syncthreads();
    // vector forms by ADDRESS (element index + the pointer's own offset; both uniform per segment):
    // 16-B loads of xy, 4-B stores of labels.  Either pointer needs only its type's alignment.
    const int64_t xy_skew = (int64_t)(reinterpret_cast<uintptr_t>(xy) >> 2), lab_skew = label_skew(labels);
    for (int64_t s = blockIdx.x; s < segs.n_segs; s += gridDim.x) {
        const int64_t cnt = segs.count(s);
        const int64_t base = s * segs.stride;
        const bool vec_ok = ((base + xy_skew) & 3) == 0, st_ok = ((base + lab_skew) & 3) == 0;
        for (int64_t j = 4 * tid; j < cnt; j += 4 * kThreads) {
            uint32_t v[4];
            if (vec_ok && j + 3 < cnt) {
                const uint4 q = *reinterpret_cast<const uint4 *>(xy + base + j);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (j + e < cnt) ? xy[base + j + e] : 0u;
            }
            uint32_t lab[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = j + e < cnt;
                const int x = ecc::xy_x(v[e]), y = ecc::xy_y(v[e]);
                lab[e] = ok ? assign_point((float)x, (float)y, c_lds, k, thr) : 255u;
                if (kAccumulate && lab[e] != 255u) {
                    atomicAdd(&a_xc[wave][lab[e]], (1ull << 40) | (unsigned long long)x);
                    atomicAdd(&a_y[wave][lab[e]], (unsigned long long)y);
                }
            }
            if (labels) {
                if (j + 3 < cnt && st_ok) {
                    const uint32_t pk = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
                    *reinterpret_cast<uint32_t *>(labels + base + j) = pk;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (j + e < cnt) labels[base + j + e] = (uint8_t)lab[e];
                }
            }
        }
    }
    if (kAccumulate) {
        __syncthreads();
        if (tid < k) {
            unsigned long long xc = 0, ys = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) { xc += a_xc[w][tid]; ys += a_y[w][tid]; }
            const unsigned long long n_pts = xc >> 40;
            if (n_pts) {
                atomicAdd(&acc[3 * tid + 0], n_pts);
                atomicAdd(&acc[3 * tid + 1], xc & ((1ull << 40) - 1));
                atomicAdd(&acc[3 * tid + 2], ys);
            }
        }
    }
}

// One Lloyd pass (kAccumulate) or the final labelling.  Accumulation: every point adds
// (1 << 52) | (x << 26) | y to its cluster's u64 slot of its WAVE in LDS with one no-return
// ds_add_u64 (64 lanes spread over <= K addresses).  The packed fields are exact while a slot
// receives < 512 points of < 2^16 per coordinate, so each wave unpacks its slots into u64 lane
// totals (lane c = cluster c) every kFlushBatches = 2 batches of 256 points.  One global u64
// atomic per (WG, cluster, field) at the end, spread over n_copies accumulator replicas.
// (Fusing the update into the last-arriving workgroup was measured slower: the device-scope
// release every workgroup needs before arriving costs more than the separate 1-wave launch.)
template <int K, bool kAccumulate>
__global__ void __launch_bounds__(kThreads)
kmeans_fast_kernel(const uint32_t *__restrict__ xy, Segs segs, const float *__restrict__ cent, int k, float thr,
                   unsigned long long *acc, int n_copies, const KmState *st, uint8_t *__restrict__ labels) {
    if (kAccumulate && st->done) return;
    __shared__ unsigned long long slot[kWaves][K];
    __shared__ unsigned long long w_acc[3][K];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // the centroids live in scalar registers
    float cx[K], cy[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        cx[i] = uniform_f32(i < k ? cent[2 * i] : __builtin_inff());
        cy[i] = uniform_f32(i < k ? cent[2 * i + 1] : __builtin_inff());
    }
    if (kAccumulate) {
        for (int i = tid; i < 3 * K; i += kThreads) (&w_acc[0][0])[i] = 0ull;
        if (lane < K) slot[wave][lane] = 0ull;
        __syncthreads();
    }
    unsigned long long tn = 0, tx = 0, ty = 0;  // lane c: wave totals of cluster c
    int batches = 0;
    auto flush = [&]() {  // the wave's own slots: LDS ops of one wave complete in order
        if (lane < K) {
            const unsigned long long w = slot[wave][lane];
            slot[wave][lane] = 0ull;
            tn += w >> 52;
            tx += (w >> 26) & ((1ull << 26) - 1);
            ty += w & ((1ull << 26) - 1);
        }
    };
    const int64_t lab_skew = label_skew(labels);
    for (int64_t s = blockIdx.x; s < segs.n_segs; s += gridDim.x) {
        const int64_t cnt = segs.count(s);
        const int64_t base = s * segs.stride;
        const bool st_ok = ((base + lab_skew) & 3) == 0;  // 4-B label stores by address (uniform)
        // Two 4-point batches per lane per trip: both loads and all eight label gathers are in
        // flight before the first LDS add, halving the dependent load -> gather -> add rounds.
        // the segment through a buffer view rounded up to 16 B (up to 12 B past the last point: the
        // bytes include/ecc.h asks callers to keep readable; points past cnt are masked):
        // unconditional 16-B loads (4-B alignment suffices)
        const __amdgpu_buffer_rsrc_t vs = ecc::buffer_view(xy + base, (uint32_t)((cnt * 4 + 15) & ~15ll));
        for (int64_t j0 = 0; j0 < cnt; j0 += 8 * kThreads) {  // uniform trip count per WG
            uint32_t v[8], lab[8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint4 q = ecc::buffer_load_u128(vs, (uint32_t)tid * 16u, (uint32_t)(j0 + u * 4 * kThreads) * 4u);
                v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int64_t j = j0 + u * 4 * kThreads + 4 * tid;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t w = v[4 * u + e];
                    const uint32_t x = (uint32_t)ecc::xy_x(w), y = (uint32_t)ecc::xy_y(w);
                    uint32_t l;
                    if (j + e >= cnt) l = 255u;
                    else l = assign_fast<K>((float)x, (float)y, cx, cy, thr);
                    lab[4 * u + e] = l;
                }
            }
            if (kAccumulate) {
                // Runs of equal labels are summed in registers first: neighbouring events mostly share
                // a cluster, and LDS atomics from many lanes to one slot serialise.
                uint32_t cl = lab[0];
                unsigned long long run = 0ull;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned long long pk = (1ull << 52) | ((unsigned long long)ecc::xy_x(v[e]) << 26) |
                                                  (unsigned long long)ecc::xy_y(v[e]);
                    if (lab[e] != cl) {
                        if (cl < (uint32_t)K) atomicAdd(&slot[wave][cl], run);
                        cl = lab[e];
                        run = 0ull;
                    }
                    run += pk;
                }
                if (cl < (uint32_t)K) atomicAdd(&slot[wave][cl], run);
                batches += 2;
                if (batches >= kFlushBatches) {
                    flush();
                    batches = 0;
                }
            }
            if (labels) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int64_t j = j0 + u * 4 * kThreads + 4 * tid;
                    if (j + 3 < cnt && st_ok) {
                        const uint32_t pk = lab[4 * u] | (lab[4 * u + 1] << 8) | (lab[4 * u + 2] << 16) |
                                            (lab[4 * u + 3] << 24);
                        *reinterpret_cast<uint32_t *>(labels + base + j) = pk;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (j + e < cnt) labels[base + j + e] = (uint8_t)lab[4 * u + e];
                    }
                }
            }
        }
    }
    if (!kAccumulate) return;
    flush();
    if (lane < K && tn) {
        atomicAdd(&w_acc[0][lane], tn);
        atomicAdd(&w_acc[1][lane], tx);
        atomicAdd(&w_acc[2][lane], ty);
    }
    __syncthreads();
    if (tid < 3 * k) {
        const int f = tid / k, c = tid - f * k;
        const unsigned long long sum = w_acc[f][c];
        if (sum) atomicAdd(&acc[(int)(blockIdx.x % n_copies) * kAccStride + 3 * c + f], sum);
    }
}

// Final labels from the label image: one workgroup per segment, 16 points per lane, so a
// segment of up to 4096 points is ONE trip — its four 16-B loads, sixteen image gathers and four
// packed stores each in flight together (kmeans_fast_kernel's two-batch trips took two dependent
// load -> gather -> store rounds per bench segment of ~3150 points).  The loads are issued
// before the segment count arrives: a lane reads within the segment's stride (always readable),
// and only the stores are masked by the count.  Labels equal assign_fast's on the same points.
constexpr int kLabPer = 16;
template <int K>
__global__ void __launch_bounds__(kThreads)
kmeans_img_labels_kernel(const uint32_t *__restrict__ xy, Segs segs, const float *__restrict__ cent, int k,
                         float thr, const uint8_t *__restrict__ img, const uint32_t *__restrict__ img_wh,
                         uint8_t *__restrict__ labels) {
    __shared__ float s_cx[K], s_cy[K];
    const int tid = threadIdx.x;
    if (tid < K) {
        s_cx[tid] = tid < k ? cent[2 * tid] : __builtin_inff();
        s_cy[tid] = tid < k ? cent[2 * tid + 1] : __builtin_inff();
    }
    __syncthreads();
    const uint32_t img_w = img_wh[0], img_h = img_wh[1];
    const int64_t lab_skew = label_skew(labels);
    for (int64_t s = blockIdx.x; s < segs.n_segs; s += gridDim.x) {
        const int64_t base = s * segs.stride;
        const bool st_ok = ((base + lab_skew) & 3) == 0;  // 4-B label stores by address (uniform)
        // readable extent: the whole stride (the next segment starts after it), except in the
        // last segment, whose buffer may end at its count
        const int64_t cnt = segs.count(s);
        const int64_t lim = s + 1 < segs.n_segs ? segs.stride : cnt;
        const __amdgpu_buffer_rsrc_t vs = ecc::buffer_view(xy + base, (uint32_t)((lim * 4 + 15) & ~15ll));
        for (int64_t j0 = 0; j0 < cnt; j0 += kLabPer * kThreads) {
            uint32_t v[kLabPer], lab[kLabPer];
#pragma unroll
            for (int u = 0; u < kLabPer / 4; ++u) {  // unconditional 16-B loads (see kmeans_fast_kernel)
                const uint4 q = ecc::buffer_load_u128(vs, (uint32_t)tid * 16u, (uint32_t)(j0 + u * 4 * kThreads) * 4u);
                v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < kLabPer / 4; ++u) {
                const int64_t j = j0 + u * 4 * kThreads + 4 * tid;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t w = v[4 * u + e];
                    const uint32_t x = (uint32_t)ecc::xy_x(w), y = (uint32_t)ecc::xy_y(w);
                    uint32_t l = 255u;
                    if (j + e < cnt) {
                        if (__builtin_expect(x < img_w && y < img_h, 1)) l = img[y * kImgSide + x];
                        else l = assign_lds<K>((float)x, (float)y, s_cx, s_cy, thr);
                    }
                    lab[4 * u + e] = l;
                }
            }
#pragma unroll
            for (int u = 0; u < kLabPer / 4; ++u) {
                const int64_t j = j0 + u * 4 * kThreads + 4 * tid;
                if (j + 3 < cnt && st_ok) {
                    const uint32_t pk = lab[4 * u] | (lab[4 * u + 1] << 8) | (lab[4 * u + 2] << 16) |
                                        (lab[4 * u + 3] << 24);
                    *reinterpret_cast<uint32_t *>(labels + base + j) = pk;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (j + e < cnt) labels[base + j + e] = (uint8_t)lab[4 * u + e];
                }
            }
        }
    }
}

// The same labels with the label image staged in LDS (frames up to kLabLdsBytes, e.g. the
// 90 KB of 346x260): the image gathers of kmeans_img_labels_kernel hit a different cache line per
// lane, so its 7.7 M gathers were bound by the texture units' one-line-per-cycle tag lookups, not
// by HBM.  One 1024-lane workgroup per CU copies the image once from L2, then takes four segments
// per trip (256 lanes x 16 points each), loads issued before the counts arrive as above.
constexpr int kLabLdsThreads = 1024;
constexpr int kLabLdsBytes = 96 * 1024;
template <int K>
__global__ void __launch_bounds__(kLabLdsThreads)
kmeans_lds_labels_kernel(const uint32_t *__restrict__ xy, Segs segs, const float *__restrict__ cent, int k,
                         float thr, const uint8_t *__restrict__ img, const uint32_t *__restrict__ img_wh,
                         uint8_t *__restrict__ labels) {
    extern __shared__ uint8_t s_img[];  // [img_h][img_w], compact
    __shared__ float s_cx[K], s_cy[K];
    const int tid = threadIdx.x, sub = tid >> 8, t = tid & 255;
    if (tid < K) {
        s_cx[tid] = tid < k ? cent[2 * tid] : __builtin_inff();
        s_cy[tid] = tid < k ? cent[2 * tid + 1] : __builtin_inff();
    }
    const uint32_t img_w = img_wh[0], img_h = img_wh[1];
    // rows copied as words (row pitch img_w rounded up to 4), eight loads in flight per lane
    const uint32_t wq = (img_w + 3) >> 2, pitch = 4 * wq, n_words = wq * img_h;
    for (uint32_t i0 = 0; i0 < n_words; i0 += 8 * kLabLdsThreads) {
        uint32_t wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {  // clamped word: unconditional loads, all eight in flight
            const uint32_t i0u = i0 + u * kLabLdsThreads + tid, i = i0u < n_words ? i0u : n_words - 1, r = i / wq;
            wv[u] = *reinterpret_cast<const uint32_t *>(img + r * kImgSide + 4 * (i - r * wq));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t i = i0 + u * kLabLdsThreads + tid;
            if (i < n_words) reinterpret_cast<uint32_t *>(s_img)[i] = wv[u];
        }
    }
    __syncthreads();
    const int64_t lab_skew = label_skew(labels);
    for (int64_t s0 = 4 * (int64_t)blockIdx.x; s0 < segs.n_segs; s0 += 4 * (int64_t)gridDim.x) {
        const int64_t s = s0 + sub;
        if (s >= segs.n_segs) continue;  // no barrier below
        const int64_t base = s * segs.stride;
        const bool st_ok = ((base + lab_skew) & 3) == 0;  // 4-B label stores by address (per sub-group)
        const int64_t cnt = segs.count(s);
        const int64_t lim = s + 1 < segs.n_segs ? segs.stride : cnt;
        // the segment through a buffer view rounded up to 16 B (up to 12 B past the last point, which
        // include/ecc.h asks callers to keep readable; points past cnt are masked): one
        // unconditional 16-B load per quad
        const __amdgpu_buffer_rsrc_t vs = ecc::buffer_view(xy + base, (uint32_t)((lim * 4 + 15) & ~15ll));
        for (int64_t j0 = 0; j0 < cnt; j0 += kLabPer * 256) {
            uint32_t v[kLabPer], lab[kLabPer];
#pragma unroll
            for (int u = 0; u < kLabPer / 4; ++u) {  // (16-B buffer loads need only 4-B alignment)
                const uint4 q = ecc::buffer_load_u128(vs, (uint32_t)t * 16u, (uint32_t)(j0 + u * 4 * 256) * 4u);
                v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < kLabPer / 4; ++u) {
                const int64_t j = j0 + u * 4 * 256 + 4 * t;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t w = v[4 * u + e];
                    const uint32_t x = (uint32_t)ecc::xy_x(w), y = (uint32_t)ecc::xy_y(w);
                    uint32_t l = 255u;
                    if (j + e < cnt) {
                        if (__builtin_expect(x < img_w && y < img_h, 1)) l = s_img[y * pitch + x];
                        else l = assign_lds<K>((float)x, (float)y, s_cx, s_cy, thr);
                    }
                    lab[4 * u + e] = l;
                }
            }
#pragma unroll
            for (int u = 0; u < kLabPer / 4; ++u) {
                const int64_t j = j0 + u * 4 * 256 + 4 * t;
                if (j + 3 < cnt && st_ok) {
                    const uint32_t pk = lab[4 * u] | (lab[4 * u + 1] << 8) | (lab[4 * u + 2] << 16) |
                                        (lab[4 * u + 3] << 24);
                    *reinterpret_cast<uint32_t *>(labels + base + j) = pk;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (j + e < cnt) labels[base + j + e] = (uint8_t)lab[4 * u + e];
                }
            }
        }
    }
}

// ---- label image (k <= 32) -------------------------------------------------------------------
// The assignment depends on a point's (x, y) only, and event representatives sit on a sensor
// grid (the bench: 7.7 M points on 346x260 pixels, ~85 per pixel).  Each pass therefore first
// labels every pixel of the points' bounding box once (assign_fast, the same function), and the
// accumulation pass reads a point's label from that image instead of testing k centres.  Points
// outside the kImgSide x kImgSide area are assigned directly.

__global__ void __launch_bounds__(kThreads)
kmeans_extent_kernel(const uint32_t *__restrict__ xy, Segs segs, uint32_t *__restrict__ ext) {
    uint32_t mx = 0, my = 0;
    bool any = false;
    for (int64_t s = blockIdx.x; s < segs.n_segs; s += gridDim.x) {
        const int64_t cnt = segs.count(s), base = s * segs.stride;
        for (int64_t j = threadIdx.x; j < cnt; j += kThreads) {
            const uint32_t v = xy[base + j], x = v & 0xffffu, y = v >> 16;
            if (x < kImgSide && y < kImgSide) {
                mx = max(mx, x);
                my = max(my, y);
                any = true;
            }
        }
    }
    // per-WG maxima into ext[2 * blockIdx] (no atomics: same-address device atomics serialise)
    __shared__ uint32_t wmx[kThreads / 64], wmy[kThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        my = max(my, (uint32_t)__shfl_xor((int)my, o));
    }
    const bool wany = __any(any);
    if ((threadIdx.x & 63) == 0) {
        wmx[threadIdx.x >> 6] = wany ? mx + 1 : 0u;
        wmy[threadIdx.x >> 6] = wany ? my + 1 : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (int w = 0; w < kThreads / 64; ++w) { a = max(a, wmx[w]); b = max(b, wmy[w]); }
        ext[2 * blockIdx.x] = a;
        ext[2 * blockIdx.x + 1] = b;
    }
}

// Per-pixel point counts: the assignment depends on a point's pixel only, so a Lloyd pass can
// visit each occupied pixel once with its multiplicity n, adding (n, n*x, n*y) — the same
// integer sums as adding every point.  Counts are compact over the bounding box (w x h from the
// extent kernel): cnt[y * w + x].  No global atomics (they execute at the memory side): workgroup
// (chunk c, part m) counts the points of its part falling in pixel chunk c into LDS and stores
// the chunk densely into partial[m]; kmeans_count_sum_kernel adds the parts.  Part 0's
// workgroups of chunk 0 also list the points outside the kImgSide^2 image.
constexpr int kHistThreads = 1024;
#ifndef ECC_KM_HIST_CHUNK
#define ECC_KM_HIST_CHUNK 32768
#endif
constexpr int kHistChunk = ECC_KM_HIST_CHUNK;  // pixels per LDS chunk (128 KiB)
constexpr int64_t kHistBudget = 16 << 20;  // partial-count entries (64 MiB): parts used = budget / cells

__host__ __device__ inline int parts_used(int parts, int64_t cells) {
    const int64_t p = cells > 0 ? kHistBudget / cells : parts;
    return (int)(p < 1 ? 1 : (p < parts ? p : parts));
}
constexpr int kHistUnroll = 4;
constexpr int kHistSegs = 4;
#ifndef ECC_KM_PIX_GRID
#define ECC_KM_PIX_GRID 128
#endif
// pixel-pass workgroups: on the k-means chain alone 256 were fastest (64: 102 us per ten passes
// against 82), but that chain runs beside the corner chain and has slack; 128 (87 us) leaves the
// corner chain more room: two-stream step 0.636 -> 0.630 ms
constexpr int kPixGrid = ECC_KM_PIX_GRID;

__device__ __forceinline__ void reduce_extent(const uint32_t *__restrict__ ext, int n_ext, uint32_t *s_red,
                                              uint32_t &w, uint32_t &h) {
    uint32_t p = 0, q = 0;
    for (int i = threadIdx.x; i < n_ext; i += blockDim.x) { p = max(p, ext[2 * i]); q = max(q, ext[2 * i + 1]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        p = max(p, (uint32_t)__shfl_xor((int)p, o));
        q = max(q, (uint32_t)__shfl_xor((int)q, o));
    }
    if ((threadIdx.x & 63) == 0) {
        s_red[2 * (threadIdx.x >> 6)] = p;
        s_red[2 * (threadIdx.x >> 6) + 1] = q;
    }
    __syncthreads();
    w = 0;
    h = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { w = max(w, s_red[2 * i]); h = max(h, s_red[2 * i + 1]); }
}

// 1-D grid, XCD-aware: workgroup b runs on XCD b % 8; the kCountSlots chunk workgroups of one
// part (point range) share b % 8 and are dispatched back to back, so the second and third reads of
// the part's points hit that XCD's L2 instead of HBM.
// The slot count is the frame's chunk count when the caller gives the frame (3 at 346x260, so
// no workgroup of a fourth slot idles), else 4; parts fill the 256 CUs: 8 * (32 / slots).
constexpr int kCountSlots = 4;
#ifndef ECC_KM_COUNT_MUL
#define ECC_KM_COUNT_MUL 8
#endif
#ifndef ECC_KM_LAB_GRID
#define ECC_KM_LAB_GRID 256
#endif

__host__ __device__ inline int count_grid(int parts, int slots) { return 8 * ((parts + 7) / 8) * slots; }

inline void count_layout(int64_t n_segs, int64_t cells, int &parts, int &slots) {
    const int64_t ch = (cells + kHistChunk - 1) / kHistChunk;
    slots = cells > 0 ? (int)(ch < 1 ? 1 : (ch < kCountSlots ? ch : kCountSlots)) : kCountSlots;
    parts = (int)std::min<int64_t>(ECC_KM_COUNT_MUL * (32 / slots), std::max<int64_t>(n_segs, 1));
}

__global__ void __launch_bounds__(kHistThreads)
kmeans_count_kernel(const uint32_t *__restrict__ xy, Segs segs, const uint32_t *__restrict__ ext, int n_ext,
                    int parts, int slots, uint32_t *__restrict__ partial, uint32_t *__restrict__ wh,
                    uint32_t *__restrict__ outside, uint32_t *__restrict__ n_outside, uint32_t fixed_w,
                    uint32_t fixed_h, int32_t *__restrict__ err) {
    extern __shared__ uint32_t hist[];  // [kHistChunk]
    __shared__ uint32_t s_red[2 * kHistThreads / 64];
    const int xcd = (int)(blockIdx.x % 8), i8 = (int)(blockIdx.x / 8);
    const int m = (i8 / slots) * 8 + xcd, slot = i8 % slots, tid = threadIdx.x;
    // frame: fixed_w > 0 = the caller's frame; points outside it are an error (err != null: the
    // multi-GPU count images) or go to the outside list; otherwise the bounding box of the points
    // inside the kImgSide^2 image
    const bool fixed = fixed_w > 0;
    uint32_t w = fixed_w, h = fixed_h;
    if (!fixed) reduce_extent(ext, n_ext, s_red, w, h);
    const uint32_t lim_x = fixed ? w : kImgSide, lim_y = fixed ? h : kImgSide;
    const int64_t cells = (int64_t)w * h;
    if (blockIdx.x == 0 && tid == 0) {
        wh[0] = w;
        wh[1] = h;
    }
    parts = parts_used(parts, cells);
    if (m >= parts) return;
    const int64_t s0 = segs.n_segs * m / parts, s1 = segs.n_segs * (m + 1) / parts;
    const int64_t n_chunks = (cells + kHistChunk - 1) / kHistChunk;
    for (int64_t c = slot; c < (n_chunks > 0 ? n_chunks : 1); c += slots) {
        const int64_t lo = c * kHistChunk;
        const int n_loc = (int)((cells - lo) < kHistChunk ? (cells - lo) : kHistChunk);
        for (int i = tid; i < kHistChunk; i += kHistThreads) hist[i] = 0u;
        __syncthreads();
        // kHistSegs segments per trip, kHistUnroll x 1024 points of each: 16 independent loads per
        // lane in flight (a bench segment holds ~3150 points, so one segment per trip left the
        // trips latency-bound: 30 dependent trips per part)
        for (int64_t sg = s0; sg < s1; sg += kHistSegs) {
            int64_t cnt[kHistSegs], base[kHistSegs], cmax = 0;
            int32_t cl[kHistSegs];  // the counts' loads together (clamped segment, no branch between)
            if (segs.counts) {
#pragma unroll
                for (int i = 0; i < kHistSegs; ++i) cl[i] = segs.counts[sg + i < s1 ? sg + i : s1 - 1];
            } else {
#pragma unroll
                for (int i = 0; i < kHistSegs; ++i) cl[i] = (int32_t)segs.count(sg + i);
            }
            // clamped to [0, stride] like Segs::count (ecc::seg_points' rule) where the loaded value
            // is first used, so nothing waits for the loads earlier than before; past the part's
            // last segment the upper bound is 0
            const int32_t cap = (int32_t)segs.stride;
#pragma unroll
            for (int i = 0; i < kHistSegs; ++i) {
                cnt[i] = max(min(cl[i], sg + i < s1 ? cap : 0), 0);
                base[i] = (sg + i) * segs.stride;
                cmax = cnt[i] > cmax ? cnt[i] : cmax;
            }
            // per segment a buffer view (0 past its count): the 16 loads are unconditional, so all
            // of them are in flight together (a load under a per-lane condition waited for the last)
            __amdgpu_buffer_rsrc_t vs[kHistSegs];
#pragma unroll
            for (int i = 0; i < kHistSegs; ++i) vs[i] = ecc::buffer_view(xy + base[i], (uint32_t)cnt[i] * 4u);
            for (int64_t j0 = 0; j0 < cmax; j0 += kHistUnroll * kHistThreads) {
                uint32_t v[kHistSegs][kHistUnroll];
#pragma unroll
                for (int i = 0; i < kHistSegs; ++i)
#pragma unroll
                    for (int u = 0; u < kHistUnroll; ++u)
                        v[i][u] = ecc::buffer_load_u32(vs[i], (uint32_t)tid * 4u, (uint32_t)(j0 + u * kHistThreads) * 4u);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < kHistSegs; ++i)
#pragma unroll
                    for (int u = 0; u < kHistUnroll; ++u) {
                        if (j0 + u * kHistThreads + tid >= cnt[i]) continue;
                        const uint32_t x = v[i][u] & 0xffffu, y = v[i][u] >> 16;
                        if (x < lim_x && y < lim_y) {
                            const int64_t idx = (int64_t)y * w + x - lo;
                            if (idx >= 0 && idx < n_loc) atomicAdd(&hist[idx], 1u);
                        } else if (c == 0) {
                            if (err) *err = 1;
                            else outside[atomicAdd(n_outside, 1u)] = v[i][u];
                        }
                    }
            }
        }
        __syncthreads();
        uint32_t *out = partial + (int64_t)m * cells + lo;
        for (int i = tid; i < n_loc; i += kHistThreads) out[i] = hist[i];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads)
kmeans_count_sum_kernel(const uint32_t *__restrict__ partial, int parts, const uint32_t *__restrict__ wh,
                        uint32_t *__restrict__ cnt) {
    const int64_t cells = (int64_t)wh[0] * wh[1];
    parts = parts_used(parts, cells);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kThreads) {
        uint32_t t = 0;
        int m = 0;
        for (; m + 8 <= parts; m += 8) {  // eight independent loads in flight
            uint32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(int64_t)(m + u) * cells + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) t += v[u];
        }
        for (; m < parts; ++m) t += partial[(int64_t)m * cells + i];
        cnt[i] = t;
    }
}

// One kmeans_step_kernel per Lloyd pass replaces "update, then label image": every workgroup
// re-derives the centroid update from the previous pass's accumulator replicas (a few hundred
// L2 reads), so no second launch and no grid-wide hand-off is needed.  Buffers alternate by pass:
// pass it accumulates into acc[it & 1] and labels with C_it, stored in cb[it & 1].  step(it)
// reads acc[(it-1) & 1] and cb[(it-1) & 1], so WG 0 alone may write cb[it & 1], the caller's
// centroids and the state, and zero acc[it & 1] (last read by step(it-1)).  The update
// arithmetic is kmeans_update_kernel's, in the same order.
struct StepArgs {
    const unsigned long long *acc_in;  // pass it-1's replicas (nullptr: no update in this step)
    unsigned long long *acc_zero;      // pass it's replicas, zeroed by WG 0
    const float *c_prev;               // C_{it-1} (or C_0 when acc_in is null)
    float *c_next;                     // cb[it & 1]
    float *cent;                       // the caller's centroids (final result)
    int n_copies, k;
    float thr, tol;
    bool final_pass;                   // after the last pass: update, then label image if wanted
    bool want_image;
};

// kPix: instead of a label image, the pass itself — (n, n*x, n*y) of every occupied pixel (cnt)
// and (1, x, y) of every outside point, into acc_out; WG 0 zeroes acc_zero, the replicas the
// NEXT pass accumulates into (three sets rotate: read by this pass's update, written, zeroed).
struct PixArgs {
    const uint32_t *cnt, *outside, *n_outside;
    unsigned long long *acc_out;
    const uint32_t *wh;  // bounding box (w, h), or null: reduce the per-WG extents
};

template <int K, bool kPix>
__global__ void __launch_bounds__(kThreads)
kmeans_step_kernel(StepArgs a, const uint32_t *__restrict__ ext, int n_ext, uint8_t *__restrict__ img,
                   KmState *st, PixArgs px) {
    // tol < 0 never sets done (fixed pass count): no dependent read of the state before the update
    const bool done_in = a.tol >= 0.f && st->done != 0;
    if (done_in && !a.final_pass) return;
    const int tid = threadIdx.x;
    __shared__ uint32_t s_wh[2][kThreads];
    __shared__ unsigned long long s_sum[3][K];
    __shared__ float s_c[2][K];
    __shared__ int s_done;
    const bool update = a.acc_in && !done_in;
    const float *c_src = done_in ? a.cent : a.c_prev;  // converged earlier: the caller's array is final
    if (update) {
        if (tid < 3 * a.k) {
            const int c = tid / 3, f = tid - 3 * c;
            unsigned long long t[kAccCopies], v = 0;  // all replicas' loads in flight together
#pragma unroll
            for (int r = 0; r < kAccCopies; ++r) t[r] = r < a.n_copies ? a.acc_in[r * kAccStride + 3 * c + f] : 0ull;
#pragma unroll
            for (int r = 0; r < kAccCopies; ++r) v += t[r];
            s_sum[f][c] = v;
        }
        if (blockIdx.x == 0)
            for (int i = tid; i < a.n_copies * kAccStride; i += kThreads) a.acc_zero[i] = 0ull;
        __syncthreads();
        if (tid < 64) {
            float shift = 0.f;
            if (tid < a.k) {
                const float ox = c_src[2 * tid], oy = c_src[2 * tid + 1];
                float nx = ox, ny = oy;
                const double n_pts = (double)s_sum[0][tid];
                if (n_pts > 0.0) {
                    nx = (float)((double)s_sum[1][tid] / n_pts);
                    ny = (float)((double)s_sum[2][tid] / n_pts);
                    shift = fmaxf(fabsf(nx - ox), fabsf(ny - oy));
                }
                s_c[0][tid] = nx;
                s_c[1][tid] = ny;
                if (blockIdx.x == 0) {
                    a.c_next[2 * tid] = nx;
                    a.c_next[2 * tid + 1] = ny;
                    a.cent[2 * tid] = nx;
                    a.cent[2 * tid + 1] = ny;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) shift = fmaxf(shift, __shfl_xor(shift, o));
            if (tid == 0) {
                const int done = (a.tol >= 0.f && shift <= a.tol) ? 1 : 0;
                s_done = done;
                if (blockIdx.x == 0) {
                    st->iters += 1;
                    st->done = done;
                }
            }
        }
    } else {
        if (tid < a.k) {
            s_c[0][tid] = c_src[2 * tid];
            s_c[1][tid] = c_src[2 * tid + 1];
            if (blockIdx.x == 0 && !done_in) {
                a.c_next[2 * tid] = s_c[0][tid];
                a.c_next[2 * tid + 1] = s_c[1][tid];
            }
        }
        if (tid == 0) s_done = done_in ? 1 : 0;
    }
    if (px.wh) {  // bounding box stored by kmeans_count_kernel
        if (tid == 0) {
            s_wh[0][0] = px.wh[0];
            s_wh[1][0] = px.wh[1];
        }
        __syncthreads();
    } else {  // bounding box = max over the extent kernel's per-WG maxima
        uint32_t p = 0, q = 0;
        for (int i = tid; i < n_ext; i += kThreads) { p = max(p, ext[2 * i]); q = max(q, ext[2 * i + 1]); }
        s_wh[0][tid] = p;
        s_wh[1][tid] = q;
        __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) {
            if (tid < o) {
                s_wh[0][tid] = max(s_wh[0][tid], s_wh[0][tid + o]);
                s_wh[1][tid] = max(s_wh[1][tid], s_wh[1][tid + o]);
            }
            __syncthreads();
        }
    }
    // a pass that converged runs no further accumulation: its image is only needed for labels
    if (a.final_pass ? !a.want_image : s_done != 0) return;
    float cx[K], cy[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        cx[i] = uniform_f32(i < a.k ? s_c[0][i] : __builtin_inff());
        cy[i] = uniform_f32(i < a.k ? s_c[1][i] : __builtin_inff());
    }
    const uint32_t w = s_wh[0][0], h = s_wh[1][0];
    const int64_t cells = (int64_t)w * h;
    if constexpr (!kPix) {
        for (uint32_t c = blockIdx.x * kThreads + tid; c < (uint32_t)cells; c += gridDim.x * kThreads) {
            const uint32_t y = c / w, x = c - y * w;  // cells <= kImgSide^2: 32-bit index
            img[(int64_t)y * kImgSide + x] = (uint8_t)assign_fast<K>((float)x, (float)y, cx, cy, a.thr);
        }
    } else {
        __shared__ unsigned long long w_acc[3][K];
        for (int i = tid; i < 3 * K; i += kThreads) (&w_acc[0][0])[i] = 0ull;
        __syncthreads();
        for (uint32_t c = blockIdx.x * kThreads + tid; c < (uint32_t)cells; c += gridDim.x * kThreads) {
            const uint32_t y = c / w, x = c - y * w;  // cells <= kImgSide^2: 32-bit index
            const uint32_t n = px.cnt[c];
            if (!n) continue;
            const uint32_t l = assign_fast<K>((float)x, (float)y, cx, cy, a.thr);
            if (l >= (uint32_t)K) continue;
            atomicAdd(&w_acc[0][l], (unsigned long long)n);
            atomicAdd(&w_acc[1][l], (unsigned long long)n * x);
            atomicAdd(&w_acc[2][l], (unsigned long long)n * y);
        }
        const uint32_t n_out = *px.n_outside;  // (cnt is compact: cnt[y * w + x])
        for (uint32_t i = blockIdx.x * kThreads + tid; i < n_out; i += gridDim.x * kThreads) {
            const uint32_t v = px.outside[i], x = v & 0xffffu, y = v >> 16;
            const uint32_t l = assign_fast<K>((float)x, (float)y, cx, cy, a.thr);
            if (l >= (uint32_t)K) continue;
            atomicAdd(&w_acc[0][l], 1ull);
            atomicAdd(&w_acc[1][l], (unsigned long long)x);
            atomicAdd(&w_acc[2][l], (unsigned long long)y);
        }
        __syncthreads();
        if (tid < 3 * a.k) {
            const int f = tid / a.k, c = tid - f * a.k;
            const unsigned long long sum = w_acc[f][c];
            if (sum) atomicAdd(&px.acc_out[(int)(blockIdx.x % a.n_copies) * kAccStride + 3 * c + f], sum);
        }
    }
}

// Launch helpers for the fast path (k <= kFastMaxK); false when k needs the generic kernel.
template <bool kAccumulate>
bool launch_fast(int k, dim3 grid, hipStream_t s, const uint32_t *xy, const Segs &segs, const float *cent,
                 float thr, unsigned long long *acc, int n_copies, const KmState *st, uint8_t *labels) {
    if (k > kFastMaxK) return false;
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((kmeans_fast_kernel<decltype(K)::value, kAccumulate>), grid, dim3(kThreads), 0, s, xy, segs,
                           cent, k, thr, acc, n_copies, st, labels);
    });
    return true;
}

// The caller's segments; without counts, a dense array of n_segs * seg_stride points, re-cut into
// 16384-point segments.
Segs make_segs(int64_t n_segs, int64_t seg_stride, const int32_t *seg_counts) {
    Segs segs{seg_counts, n_segs, seg_stride, n_segs * seg_stride};
    if (!seg_counts) {
        const int64_t n = n_segs * seg_stride;
        segs.stride = 16384;
        segs.n_segs = (n + segs.stride - 1) / segs.stride;
        segs.n_dense = n;
    }
    return segs;
}

// Workspace of the per-pixel passes, laid out once for both callers: three sets of kAccCopies
// accumulator replicas (rotating by pass; the generic path uses copy 0 of set 0), the state and
// the centroid history cb[2], which are zeroed together (kZeroBytes); then, for points (full), the
// per-WG extents, the label image, the per-pixel counts, the count partials, the words (n_out,
// w, h) and the outside-point list; for a caller's count image only the words (w, h, n_out).
struct PixWs {
    static constexpr size_t kAccBytes = (size_t)kAccCopies * kAccStride * 8;
    static constexpr size_t kOffSt = 3 * kAccBytes, kOffCb = kOffSt + 64, kZeroBytes = kOffSt + 64;
    bool full;
    size_t off_ext, off_img, off_cnt, off_part, off_out, bytes;
    char *base = nullptr;  // the context's workspace, once `bytes` are reserved

    explicit PixWs(bool full_, int n_ext = 0, int64_t n_pts = 0) : full(full_) {
        off_ext = ecc::align_up(kOffCb + 2 * 2 * kMaxK * sizeof(float), 256);
        off_img = ecc::align_up(off_ext + (size_t)n_ext * 8, 256);
        off_cnt = ecc::align_up(off_img + (size_t)kImgSide * kImgSide, 256);
        off_part = off_cnt + (size_t)kImgSide * kImgSide * 4;
        off_out = off_part + (size_t)kHistBudget * 4;
        bytes = full ? off_out + 256 + (size_t)n_pts * 4 : off_ext + 256;
    }
    template <class T>
    T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    unsigned long long *acc(int set) const { return at<unsigned long long>((size_t)(set % 3) * kAccBytes); }
    KmState *state() const { return at<KmState>(kOffSt); }
    float *cb(int it) const { return at<float>(kOffCb) + (it & 1) * 2 * kMaxK; }
    uint32_t *n_out() const { return full ? at<uint32_t>(off_out) : at<uint32_t>(off_ext) + 2; }
    uint32_t *wh() const { return full ? at<uint32_t>(off_out) + 1 : at<uint32_t>(off_ext); }
    // full only
    uint32_t *ext() const { return at<uint32_t>(off_ext); }
    uint8_t *img() const { return at<uint8_t>(off_img); }
    uint32_t *cnt() const { return at<uint32_t>(off_cnt); }
    uint32_t *partial() const { return at<uint32_t>(off_part); }
    uint32_t *outside() const { return at<uint32_t>(off_out + 256); }
};

// Per-pixel counts of the segments' points: the parts' partial counts, then their sum into cnt.
// Frame, ext, outside and err as kmeans_count_kernel takes them.  Returns status.
int launch_counts(ecc_ctx *ctx, hipStream_t s, const uint32_t *xy, const Segs &segs, const uint32_t *ext, int n_ext,
                  int32_t frame_w, int32_t frame_h, uint32_t *partial, uint32_t *wh, uint32_t *outside,
                  uint32_t *n_out, int32_t *err, uint32_t *cnt) {
    int parts, slots;
    count_layout(segs.n_segs, (int64_t)frame_w * frame_h, parts, slots);
    if (int rc = ecc::allow_dynamic_lds(ctx, kmeans_count_kernel, kHistChunk * 4, "kmeans_count LDS")) return rc;
    {
        ECC_TIMED(ctx, s, "kmeans_count_kernel");
        hipLaunchKernelGGL(kmeans_count_kernel, dim3(count_grid(parts, slots)), dim3(kHistThreads), kHistChunk * 4, s,
                           xy, segs, ext, n_ext, parts, slots, partial, wh, outside, n_out, (uint32_t)frame_w,
                           (uint32_t)frame_h, err);
    }
    {
        ECC_TIMED(ctx, s, "kmeans_count_sum_kernel");
        hipLaunchKernelGGL(kmeans_count_sum_kernel, dim3(1024), dim3(kThreads), 0, s, (const uint32_t *)partial, parts,
                           (const uint32_t *)wh, cnt);
    }
    return ECC_OK;
}

// The Lloyd passes over a count image (cnt) and an outside list: cfg->max_iters pixel passes, one
// launch each, then the final step (the last update, and the label image if wanted) on grid_final
// workgroups.  ws.wh() and ws.n_out() are set by the caller; ext / n_ext / img as the final step
// takes them.
void run_pixel_passes(ecc_ctx *ctx, hipStream_t s, const PixWs &ws, const uint32_t *cnt, const uint32_t *outside,
                      const uint32_t *ext, int n_ext, uint8_t *img, int grid_final, const ecc_kmeans_cfg *cfg,
                      float *centroids, bool want_image) {
    auto step = [&](int it, bool final_pass) {
        StepArgs a{};
        a.acc_in = it ? ws.acc(it - 1) : nullptr;
        a.acc_zero = ws.acc(it + 1);
        a.c_prev = it ? ws.cb(it - 1) : centroids;
        a.c_next = ws.cb(it);
        a.cent = centroids;
        a.n_copies = kAccCopies;
        a.k = cfg->k;
        a.thr = cfg->threshold;
        a.tol = cfg->tol;
        a.final_pass = final_pass;
        a.want_image = want_image;
        const PixArgs px{cnt, outside, ws.n_out(), ws.acc(it), ws.wh()};
        ECC_TIMED(ctx, s, final_pass ? "kmeans_step_kernel" : "kmeans_pixel_pass");
        dispatch_k(cfg->k, [&](auto K) {
            if (final_pass)
                hipLaunchKernelGGL((kmeans_step_kernel<decltype(K)::value, false>), dim3(grid_final), dim3(kThreads), 0,
                                   s, a, ext, n_ext, img, ws.state(), px);
            else
                hipLaunchKernelGGL((kmeans_step_kernel<decltype(K)::value, true>), dim3(kPixGrid), dim3(kThreads), 0, s,
                                   a, ext, n_ext, img, ws.state(), px);
        });
    };
    for (int it = 0; it < cfg->max_iters; ++it) step(it, false);
    if (cfg->max_iters > 0 || want_image) step(cfg->max_iters, true);  // last update (+ image for labels)
}

}  // namespace

ECC_API void ecc_kmeans_cfg_default(ecc_kmeans_cfg *cfg) {
    if (!cfg) return;
    cfg->k = 16;            // BASELINE.json C3 (the reference hard-codes 8, assign_to_centers.cl:14)
    cfg->max_iters = 20;
    cfg->threshold = 50.f;  // assign_to_centers.cl:11
    cfg->tol = 1e-3f;
}

static int kmeans_run_xy16_impl(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs, int64_t seg_stride,
                                const int32_t *seg_counts, int32_t frame_w, int32_t frame_h,
                                const ecc_kmeans_cfg *cfg, float *centroids, uint8_t *labels,
                                int32_t *iters_out, ecc_stream_t stream) {
    int rc = kmeans_check(ctx, cfg, centroids);
    if (rc) return rc;
    if (n_segs < 0 || seg_stride < 1) return ECC_ERR_INVALID;
    if (frame_w < 0 || frame_h < 0 || frame_w > kImgSide || frame_h > kImgSide || (frame_w == 0) != (frame_h == 0))
        return ECC_ERR_INVALID;
    const Segs segs = make_segs(n_segs, seg_stride, seg_counts);
    if (segs.n_segs > 0 && !xy) return ECC_ERR_INVALID;
    // per-WG packed counts must stay < 2^24 points (sum_x < 2^40)
    const int grid = grid_for(segs.n_segs);
    if (segs.n_segs * segs.stride / grid >= (1ll << 24)) return ECC_ERR_INVALID;
    PixWs ws(true, grid, segs.n_segs * segs.stride);
    rc = ecc::ws_reserve(ctx, ws.bytes);
    if (rc) return rc;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    ws.base = static_cast<char *>(ctx->ws);
    KmState *st = ws.state();
    ECC_CHECK_HIP(ctx, hipMemsetAsync(ws.base, 0, PixWs::kZeroBytes, s), "memset(kmeans acc)");
    if (segs.n_segs == 0) {
        if (iters_out)
            ECC_CHECK_HIP(ctx, hipMemcpyAsync(iters_out, &st->iters, 4, hipMemcpyDeviceToDevice, s), "copy iters");
        return ECC_OK;
    }
    if (cfg->k > kFastMaxK) {  // generic kernel: assign per point, separate update launch
        for (int it = 0; it < cfg->max_iters; ++it) {
            {
                ECC_TIMED(ctx, s, "kmeans_xy16_kernel");
                hipLaunchKernelGGL(kmeans_xy16_kernel<true>, dim3(grid), dim3(kThreads), 0, s, xy, segs, centroids,
                                   cfg->k, cfg->threshold, ws.acc(0), st, (uint8_t *)nullptr);
            }
            {
                ECC_TIMED(ctx, s, "kmeans_update_kernel");
                hipLaunchKernelGGL(kmeans_update_kernel<unsigned long long>, dim3(1), dim3(64), 0, s, ws.acc(0), 1,
                                   centroids, cfg->k, cfg->tol, st);
            }
        }
        ECC_CHECK_LAUNCH(ctx, "kmeans_xy16 iteration");
        if (labels) {
            ECC_TIMED(ctx, s, "kmeans_xy16_labels");
            hipLaunchKernelGGL(kmeans_xy16_kernel<false>, dim3(grid), dim3(kThreads), 0, s, xy, segs, centroids,
                               cfg->k, cfg->threshold, ws.acc(0), st, labels);
            ECC_CHECK_LAUNCH(ctx, "kmeans_xy16 labels");
        }
    } else {
        // per-pixel passes: the points are counted per pixel once, every Lloyd pass is ONE launch
        // over the occupied pixels of the bounding box (+ the outside list); labels come from the
        // final label image
        ECC_CHECK_HIP(ctx, hipMemsetAsync(ws.n_out(), 0, 4, s), "memset(kmeans outside)");
        if (frame_w == 0) {  // no frame given: the points' bounding box
            ECC_TIMED(ctx, s, "kmeans_extent_kernel");
            hipLaunchKernelGGL(kmeans_extent_kernel, dim3(grid), dim3(kThreads), 0, s, xy, segs, ws.ext());
        }
        rc = launch_counts(ctx, s, xy, segs, ws.ext(), grid, frame_w, frame_h, ws.partial(), ws.wh(), ws.outside(),
                           ws.n_out(), nullptr, ws.cnt());
        if (rc) return rc;
        run_pixel_passes(ctx, s, ws, ws.cnt(), ws.outside(), ws.ext(), grid, ws.img(), 512, cfg, centroids,
                         labels != nullptr);
        ECC_CHECK_LAUNCH(ctx, "kmeans_xy16 iteration");
        if (labels) {
            ECC_TIMED(ctx, s, "kmeans_xy16_labels");
            const int64_t frame_px = (int64_t)frame_w * frame_h;
            const int64_t frame_lds = (int64_t)ecc::align_up((size_t)frame_w, 4) * frame_h;
            const bool in_lds = frame_px > 0 && frame_lds <= kLabLdsBytes;  // the frame's label image fits in LDS
            dispatch_k(cfg->k, [&](auto K) {
                constexpr int kK = decltype(K)::value;
                if (in_lds) {
                    rc = ecc::allow_dynamic_lds(ctx, kmeans_lds_labels_kernel<kK>, kLabLdsBytes, "kmeans labels LDS");
                    if (rc) return;
                    const dim3 g((unsigned)std::min<int64_t>((segs.n_segs + 3) / 4, ECC_KM_LAB_GRID));
                    hipLaunchKernelGGL(kmeans_lds_labels_kernel<kK>, g, dim3(kLabLdsThreads), (int)frame_lds, s, xy,
                                       segs, centroids, cfg->k, cfg->threshold, ws.img(), ws.wh(), labels);
                } else {
                    const int grid_pts = (int)std::min<int64_t>(segs.n_segs, kMaxGridPts);
                    hipLaunchKernelGGL(kmeans_img_labels_kernel<kK>, dim3(grid_pts), dim3(kThreads), 0, s, xy, segs,
                                       centroids, cfg->k, cfg->threshold, ws.img(), ws.wh(), labels);
                }
            });
            if (rc) return rc;
            ECC_CHECK_LAUNCH(ctx, "kmeans_xy16 labels");
        }
    }
    if (iters_out)
        ECC_CHECK_HIP(ctx, hipMemcpyAsync(iters_out, &st->iters, 4, hipMemcpyDeviceToDevice, s),
                      "copy iters");
    return ECC_OK;
}

ECC_API int ecc_kmeans_run_xy16(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs, int64_t seg_stride,
                                const int32_t *seg_counts, const ecc_kmeans_cfg *cfg, float *centroids,
                                uint8_t *labels, int32_t *iters_out, ecc_stream_t stream) {
    return kmeans_run_xy16_impl(ctx, xy, n_segs, seg_stride, seg_counts, 0, 0, cfg, centroids, labels, iters_out,
                                stream);
}

ECC_API int ecc_kmeans_run_xy16_frame(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs, int64_t seg_stride,
                                      const int32_t *seg_counts, int32_t frame_w, int32_t frame_h,
                                      const ecc_kmeans_cfg *cfg, float *centroids, uint8_t *labels,
                                      int32_t *iters_out, ecc_stream_t stream) {
    if (frame_w < 1 || frame_h < 1) return ECC_ERR_INVALID;
    return kmeans_run_xy16_impl(ctx, xy, n_segs, seg_stride, seg_counts, frame_w, frame_h, cfg, centroids, labels,
                                iters_out, stream);
}

// ---- split form (multi-GPU: accumulate -> all-reduce(acc) -> update) ---------------------
ECC_API int ecc_kmeans_accumulate_xy16(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs,
                                       int64_t seg_stride, const int32_t *seg_counts,
                                       const float *centroids, int32_t k, float threshold,
                                       uint64_t *acc, const int32_t *state, ecc_stream_t stream) {
    if (!ctx || !centroids || !acc || !state || k < 1 || k > kMaxK || n_segs < 0 || seg_stride < 1)
        return ECC_ERR_INVALID;
    const Segs segs = make_segs(n_segs, seg_stride, seg_counts);
    if (segs.n_segs == 0) return ECC_OK;
    if (!xy) return ECC_ERR_INVALID;
    const int grid = grid_for(segs.n_segs);
    if (segs.n_segs * segs.stride / grid >= (1ll << 24)) return ECC_ERR_INVALID;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    {
        ECC_TIMED(ctx, s, "kmeans_xy16_kernel");
        auto *acc64 = reinterpret_cast<unsigned long long *>(acc);
        auto *km = reinterpret_cast<const KmState *>(state);
        if (!launch_fast<true>(k, dim3(grid), s, xy, segs, centroids, threshold, acc64, 1, km, nullptr))
            hipLaunchKernelGGL(kmeans_xy16_kernel<true>, dim3(grid), dim3(kThreads), 0, s, xy, segs,
                               centroids, k, threshold, acc64, km, (uint8_t *)nullptr);
    }
    ECC_CHECK_LAUNCH(ctx, "kmeans accumulate");
    return ECC_OK;
}

ECC_API int ecc_kmeans_update(ecc_ctx *ctx, uint64_t *acc, float *centroids, int32_t k, float tol,
                              int32_t *state, ecc_stream_t stream) {
    if (!ctx || !acc || !centroids || !state || k < 1 || k > kMaxK) return ECC_ERR_INVALID;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    {
        ECC_TIMED(ctx, s, "kmeans_update_kernel");
        hipLaunchKernelGGL(kmeans_update_kernel<unsigned long long>, dim3(1), dim3(64), 0, s,
                           reinterpret_cast<unsigned long long *>(acc), 1, centroids, k, tol,
                           reinterpret_cast<KmState *>(state));
    }
    ECC_CHECK_LAUNCH(ctx, "kmeans update");
    return ECC_OK;
}

ECC_API int ecc_kmeans_labels_xy16(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs,
                                   int64_t seg_stride, const int32_t *seg_counts,
                                   const float *centroids, int32_t k, float threshold,
                                   uint8_t *labels, ecc_stream_t stream) {
    if (!ctx || !centroids || !labels || k < 1 || k > kMaxK || n_segs < 0 || seg_stride < 1)
        return ECC_ERR_INVALID;
    const Segs segs = make_segs(n_segs, seg_stride, seg_counts);
    if (segs.n_segs == 0) return ECC_OK;
    if (!xy) return ECC_ERR_INVALID;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    {
        ECC_TIMED(ctx, s, "kmeans_xy16_labels");
        const dim3 grid(grid_for(segs.n_segs));
        if (!launch_fast<false>(k, grid, s, xy, segs, centroids, threshold, nullptr, 1, nullptr, labels))
            hipLaunchKernelGGL(kmeans_xy16_kernel<false>, grid, dim3(kThreads), 0, s, xy, segs, centroids, k,
                               threshold, (unsigned long long *)nullptr, (const KmState *)nullptr, labels);
    }
    ECC_CHECK_LAUNCH(ctx, "kmeans labels");
    return ECC_OK;
}

// ---- count images (multi-GPU k-means: one all-reduce of the counts instead of one per pass) ----
// A shard's representatives counted per pixel of a caller-given frame (counts[y * w + x], u32).
// Counts are additive over shards, and a Lloyd pass over a count image adds exactly the integer
// sums of the points it counts, so summing the shards' images once and running every pass
// locally gives each rank the single-GPU centroids.

__global__ void kmeans_set_wh_kernel(uint32_t *wh, uint32_t w, uint32_t h) {
    wh[0] = w;
    wh[1] = h;
}

ECC_API int ecc_kmeans_counts_xy16(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs, int64_t seg_stride,
                                   const int32_t *seg_counts, int32_t frame_w, int32_t frame_h, uint32_t *counts,
                                   ecc_stream_t stream) {
    if (!ctx || !counts || n_segs < 0 || seg_stride < 1 || frame_w < 1 || frame_h < 1 || frame_w > 65536 ||
        frame_h > 65536)
        return ECC_ERR_INVALID;
    const Segs segs = make_segs(n_segs, seg_stride, seg_counts);
    const int64_t cells = (int64_t)frame_w * frame_h;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    ECC_CHECK_HIP(ctx, hipMemsetAsync(&ctx->dev->kmeans_frame, 0, 4, s), "memset(kmeans err)");
    if (segs.n_segs == 0) {
        ECC_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)cells * 4, s), "memset(counts)");
        return ECC_OK;
    }
    if (!xy) return ECC_ERR_INVALID;
    // workspace: the frame words (w, h), then the count partials
    const size_t off_part = 256;
    int rc = ecc::ws_reserve(ctx, off_part + (size_t)kHistBudget * 4);
    if (rc) return rc;
    char *ws = static_cast<char *>(ctx->ws);
    rc = launch_counts(ctx, s, xy, segs, nullptr, 0, frame_w, frame_h, reinterpret_cast<uint32_t *>(ws + off_part),
                       reinterpret_cast<uint32_t *>(ws), nullptr, nullptr, &ctx->dev->kmeans_frame, counts);
    if (rc) return rc;
    ECC_CHECK_LAUNCH(ctx, "kmeans counts");
    return ECC_OK;
}

ECC_API int ecc_kmeans_counts_status(ecc_ctx *ctx, ecc_stream_t stream) {
    if (!ctx) return ECC_ERR_INVALID;
    int32_t f = 0;
    if (int rc = ecc::read_dev_words(ctx, &ctx->dev->kmeans_frame, 1, &f, ecc::as_stream(stream))) return rc;
    return f ? ECC_ERR_INVALID : ECC_OK;
}

ECC_API int ecc_kmeans_run_counts(ecc_ctx *ctx, const uint32_t *counts, int32_t frame_w, int32_t frame_h,
                                  const ecc_kmeans_cfg *cfg, float *centroids, int32_t *iters_out,
                                  ecc_stream_t stream) {
    int rc = kmeans_check(ctx, cfg, centroids);
    if (rc) return rc;
    if (!counts || frame_w < 1 || frame_h < 1 || frame_w > 65536 || frame_h > 65536) return ECC_ERR_INVALID;
    if (cfg->k > kFastMaxK) return ECC_ERR_INVALID;  // pixel passes: k <= 32
    PixWs ws(false);
    rc = ecc::ws_reserve(ctx, ws.bytes);
    if (rc) return rc;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    ws.base = static_cast<char *>(ctx->ws);
    ECC_CHECK_HIP(ctx, hipMemsetAsync(ws.base, 0, PixWs::kZeroBytes, s), "memset(kmeans acc)");
    ECC_CHECK_HIP(ctx, hipMemsetAsync(ws.n_out(), 0, 4, s), "memset(kmeans outside)");
    hipLaunchKernelGGL(kmeans_set_wh_kernel, dim3(1), dim3(1), 0, s, ws.wh(), (uint32_t)frame_w, (uint32_t)frame_h);
    // no outside points (n_out = 0): the list is never read
    run_pixel_passes(ctx, s, ws, counts, ws.n_out(), nullptr, 0, nullptr, 1, cfg, centroids, false);
    ECC_CHECK_LAUNCH(ctx, "kmeans run_counts");
    if (iters_out)
        ECC_CHECK_HIP(ctx, hipMemcpyAsync(iters_out, &ws.state()->iters, 4, hipMemcpyDeviceToDevice, s), "copy iters");
    return ECC_OK;
}
