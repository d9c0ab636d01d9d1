// k-means per downsample window (ecc_kmeans_windows_xy16): every segment is its own "fixed"-mode
// Lloyd problem, as the reference's downsample -> cluster chain fits centres per slice
// (DSA/…opencl_store.cpp:389-445, 470-518; TWE/…:396-448), and all of them run in ONE launch:
// one workgroup per segment with the whole loop inside the kernel.  A segment's result is what
// ecc_kmeans_run_xy16 gives for that segment alone (the oracle's orc_kmeans_run_xy16 on its points).
// ecc_kmeans_windows_flow_host (the per-id displacement against the previous slice) is in
// host/kmeans_windows.cpp.
#include "kmeans_common.hpp"

namespace {

constexpr int kWinMaxStride = 16384;  // the largest segment any per-segment entry point takes
// 256 CUs x 8 workgroups of 4 waves: the wave slots of the device (8 per SIMD).  More workgroups
// could not be resident whatever the stride, so the segments beyond the cap are strided over.
constexpr int kWinMaxGrid = ECC_KMEANS_WINDOWS_MAX_GRID;

// Dynamic LDS, in 4-byte words (everything is carved from the dynamic region, whose base is
// 16-byte aligned): the segment's packed points (the stride rounded up to 4), then K centre x and
// K centre y (the centres from k on hold +inf, which no comparison of assign_lds selects), the
// accumulators [wave][n, sum x, sum y][K] and the exit word.  Only the points grow with the stride.
__host__ __device__ constexpr int win_point_words(int64_t stride) { return (int)((stride + 3) & ~(int64_t)3); }
template <int K>
__host__ __device__ constexpr int win_fixed_words() { return 2 * K + kWaves * 3 * K + 4; }

// n, sum x and sum y per centre are u32: a segment has at most 16384 points of coordinates up to
// 65535, so a sum stays below 2^30 and is exact (the packed u64 slots of the global passes are per
// wave and 512 points).  Each wave adds into its own slots (ds_add_u32, no return value); wave 0
// sums the four copies in the update, so the order of the adds cannot matter.
template <int K>
__global__ void __launch_bounds__(kThreads)
kmeans_windows_kernel(const uint32_t *__restrict__ xy, ecc::SegView sv, int k, int max_iters, float thr, float tol,
                      const float *__restrict__ init, float *__restrict__ centroids, uint8_t *__restrict__ labels,
                      int32_t *__restrict__ sizes, int32_t *__restrict__ iters) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_win[];
    uint32_t *s_pts = s_win;
    float *s_cx = reinterpret_cast<float *>(s_win + win_point_words(sv.stride));
    float *s_cy = s_cx + K;
    uint32_t *s_acc = reinterpret_cast<uint32_t *>(s_cy + K);
    int *s_done = reinterpret_cast<int *>(s_acc + kWaves * 3 * K);
    const int tid = threadIdx.x;
    uint32_t *acc_w = s_acc + (tid >> 6) * 3 * K;  // this wave's slots
    const int64_t lab_skew = (int64_t)(reinterpret_cast<uintptr_t>(labels) & 3);

    for (int64_t s = blockIdx.x; s < sv.n_segs; s += gridDim.x) {
        const int cnt = ecc::seg_points(sv, s);
        const int64_t base = s * sv.stride;
        // per-segment state: the points (read from HBM once), the starting centres, zero sums
        for (int j = tid; j < cnt; j += kThreads) s_pts[j] = xy[base + j];
        if (tid < K) {
            const float *src = init ? init : centroids + s * 2 * k;
            s_cx[tid] = tid < k ? src[2 * tid] : __builtin_inff();
            s_cy[tid] = tid < k ? src[2 * tid + 1] : __builtin_inff();
        }
        for (int i = tid; i < kWaves * 3 * K; i += kThreads) s_acc[i] = 0u;
        __syncthreads();

        int it = 0;
        while (it < max_iters) {
            for (int j = tid; j < cnt; j += kThreads) {
                const uint32_t w = s_pts[j];
                const uint32_t x = (uint32_t)ecc::xy_x(w), y = (uint32_t)ecc::xy_y(w);
                const uint32_t l = assign_lds<K>((float)x, (float)y, s_cx, s_cy, thr);
                if (l != 255u) {
                    atomicAdd(&acc_w[l], 1u);
                    atomicAdd(&acc_w[K + l], x);
                    atomicAdd(&acc_w[2 * K + l], y);
                }
            }
            __syncthreads();
            if (tid < 64) {  // wave 0: c = (float)(sum / n) in fp64, shift = max |new - old|
                float shift = 0.f;
                if (tid < k) {
                    uint32_t a[3] = {0u, 0u, 0u};
#pragma unroll
                    for (int wv = 0; wv < kWaves; ++wv)
#pragma unroll
                        for (int f = 0; f < 3; ++f) {
                            a[f] += s_acc[(wv * 3 + f) * K + tid];
                            s_acc[(wv * 3 + f) * K + tid] = 0u;
                        }
                    const double n_pts = (double)a[0];
                    if (n_pts > 0.0) {
                        const float ox = s_cx[tid], oy = s_cy[tid];
                        const float nx = (float)((double)a[1] / n_pts);
                        const float ny = (float)((double)a[2] / n_pts);
                        shift = fmaxf(fabsf(nx - ox), fabsf(ny - oy));
                        s_cx[tid] = nx;
                        s_cy[tid] = ny;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) shift = fmaxf(shift, __shfl_xor(shift, o));
                if (tid == 0) *s_done = (tol >= 0.f && shift <= tol) ? 1 : 0;
            }
            __syncthreads();
            ++it;
            // the exit word is next written behind the next pass's barrier: every wave reads the
            // same value here and leaves the loop in the same pass
            if (*s_done) break;
        }

        if (tid < k) {
            centroids[s * 2 * k + 2 * tid] = s_cx[tid];
            centroids[s * 2 * k + 2 * tid + 1] = s_cy[tid];
        }
        if (iters && tid == 0) iters[s] = it;

        if (labels || sizes) {  // final pass: labels against the final centres, 4 points per lane
            const bool st_ok = ((base + lab_skew) & 3) == 0;  // 4-B label stores by address (uniform)
            for (int j = 4 * tid; j < cnt; j += 4 * kThreads) {
                const uint4 q = *reinterpret_cast<const uint4 *>(s_pts + j);  // words past cnt: not used
                const uint32_t v[4] = {q.x, q.y, q.z, q.w};
                uint32_t lab[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lab[e] = 255u;
                    if (j + e < cnt) {
                        lab[e] = assign_lds<K>((float)ecc::xy_x(v[e]), (float)ecc::xy_y(v[e]), s_cx, s_cy, thr);
                        if (sizes && lab[e] != 255u) atomicAdd(&acc_w[lab[e]], 1u);
                    }
                }
                if (labels) {
                    if (j + 3 < cnt && st_ok) {
                        *reinterpret_cast<uint32_t *>(labels + base + j) =
                            lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (j + e < cnt) labels[base + j + e] = (uint8_t)lab[e];
                    }
                }
            }
            if (sizes) {
                __syncthreads();
                if (tid < k) {
                    uint32_t n = 0u;
#pragma unroll
                    for (int wv = 0; wv < kWaves; ++wv) n += s_acc[wv * 3 * K + tid];
                    sizes[s * k + tid] = (int32_t)n;
                }
            }
        }
        __syncthreads();  // the next segment re-initialises the points, the centres and the sums
    }
}

template <class F>
void dispatch_pad(int k, F &&f) {  // the padded centre count: 16, 32 or 64
    if (k <= 16) f(std::integral_constant<int, 16>{});
    else if (k <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

}  // namespace

ECC_API int ecc_kmeans_windows_xy16(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs, int64_t seg_stride,
                                    const int32_t *seg_counts, const ecc_kmeans_cfg *cfg, const float *init,
                                    float *centroids, uint8_t *labels, int32_t *sizes, int32_t *iters,
                                    ecc_stream_t stream) {
    int rc = kmeans_check(ctx, cfg, centroids);
    if (rc) return rc;
    if (n_segs < 0 || seg_stride < 1 || seg_stride > kWinMaxStride) return ECC_ERR_INVALID;
    if (n_segs > 0 && !xy) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    const ecc::SegView sv{seg_counts, n_segs, seg_stride};
    const unsigned grid = (unsigned)std::min<int64_t>(n_segs, kWinMaxGrid);
    dispatch_pad(cfg->k, [&](auto K) {
        constexpr int kK = decltype(K)::value;
        static_assert((win_point_words(kWinMaxStride) + win_fixed_words<kK>()) * 4 <= 160 * 1024,
                      "LDS of kmeans_windows_kernel at the largest stride");
        const int lds = (win_point_words(seg_stride) + win_fixed_words<kK>()) * 4;
        if (lds > 64 * 1024) {
            rc = ecc::allow_dynamic_lds(ctx, kmeans_windows_kernel<kK>, lds, "kmeans_windows LDS");
            if (rc) return;
        }
        ECC_TIMED(ctx, s, "kmeans_windows_kernel");
        hipLaunchKernelGGL(kmeans_windows_kernel<kK>, dim3(grid), dim3(kThreads), lds, s, xy, sv, (int)cfg->k,
                           (int)cfg->max_iters, cfg->threshold, cfg->tol, init, centroids, labels, sizes, iters);
    });
    if (rc) return rc;
    ECC_CHECK_LAUNCH(ctx, "kmeans_windows");
    return ECC_OK;
}
