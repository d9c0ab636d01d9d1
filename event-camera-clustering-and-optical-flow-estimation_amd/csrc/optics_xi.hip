// OPTICS xi ("chi") cluster extraction for every segment in one launch: the literal loop of
// optics::get_chi_clusters_flat (OPT/include/optics/optics.hpp:803-944) over the reachability
// plots ecc_optics_grid / ecc_optics_f64 write (fp64, negative = undefined).
//
// The main loop is sequential in idx, so a segment is one wave's job: a workgroup holds kWaves
// waves with a segment each (no workgroup barrier anywhere), segments beyond the grid are
// strided.  Nothing in LDS grows with seg_stride:
//   * the plot is read 64 positions at a time.  A chunk's lanes hold g(pos) and the chunk's four
//     per-position predicates as ballots (steep-down :830-834, steep-up :835-838, g(i) > g(i-1)
//     :854, g(i) < g(i-1) :866), which the scalar walk tests bit by bit; the next chunk's loads
//     are issued when a chunk is entered and consumed when it is left, so the walk does not wait
//     on a load per step.  A jump back past the held chunk (an area end behind the scan, at most
//     once per chunk crossed) reloads it.
//   * max_reach (:819-820) is a wave reduction over the segment, done first.
//   * the SDA list {begin, end, mib} (+ g(begin), which filter_sdas :839-847 and cluster_borders
//     :873 re-read) lives in list order: the first kLdsSdas entries in the wave's LDS, the rest
//     in the wave's slice of the context workspace (at most n/2 + 1 entries: two SDAs begin at
//     least 2 apart).  filter_sdas is a ballot-and-prefix compaction, 64 entries per trip;
//     emission (:933-937) runs a lane per SDA: valid_combination, prefix count, cluster_borders,
//     in-order append — the reference's push order.
// Every loop is bounded by the segment length whatever the values are.
#include "ecc_internal.hpp"

#include <cmath>

namespace {

constexpr int kWaves = 4;  // waves (= segments in flight) per workgroup
constexpr int kNT = kWaves * 64;
constexpr int kLdsSdas = 128;    // SDA entries per wave held in LDS (3 KiB per wave)
constexpr int kMaxBlocks = 1024;  // 4096 waves: 16 per CU on 256 CUs

__device__ __forceinline__ double uniform_lane(double v, int l) {
    return __longlong_as_double(ecc::lane_value64(__double_as_longlong(v), l));
}

// One segment's plot, get_reach_dist (:823-829): g(0) = g(n) = max_reach, negative = 2 * max_reach.
struct Plot {
    const double *r;
    int n;
    double maxr;
    __device__ __forceinline__ double conv(int64_t p, double raw) const {
        return (p <= 0 || p >= n) ? maxr : (raw < 0.0 ? 2 * maxr : raw);
    }
    __device__ __forceinline__ double g(int64_t p) const {  // any lane, any p (read only inside (0, n))
        return (p <= 0 || p >= n) ? maxr : conv(p, r[p]);
    }
};

// The chunk the walk stands in (values + predicate ballots) and the raw loads of the one after.
struct Window {
    int c = -2;
    double vc = 0.0;
    uint64_t sd = 0, su = 0, gt = 0, lt = 0;
    double nm = 0.0, nc = 0.0, np = 0.0;
};

__device__ __forceinline__ void load_raw(const Plot &P, int ch, int lane, double &m, double &c, double &p) {
    const int64_t pos = (int64_t)ch * 64 + lane;
    m = (pos >= 1 && pos - 1 < P.n) ? P.r[pos - 1] : 0.0;
    c = pos < P.n ? P.r[pos] : 0.0;
    p = pos + 1 < P.n ? P.r[pos + 1] : 0.0;
}

__device__ __forceinline__ void enter(const Plot &P, Window &W, int idx, int lane, double omc) {
    const int ch = idx >> 6;
    if (ch == W.c) return;
    double m, c, p;
    if (ch == W.c + 1) {
        m = W.nm, c = W.nc, p = W.np;
    } else {
        load_raw(P, ch, lane, m, c, p);
    }
    load_raw(P, ch + 1, lane, W.nm, W.nc, W.np);  // in flight while this chunk is walked
    const int64_t pos = (int64_t)ch * 64 + lane;
    const double gm = P.conv(pos - 1, m), gc = P.conv(pos, c), gp = P.conv(pos + 1, p);
    const bool in = pos < P.n;
    W.sd = __ballot(in && (pos == 0 || (pos + 1 < P.n && gp <= gc * omc)));  // :830-834
    W.su = __ballot(in && (pos + 1 >= P.n || gp * omc >= gc));               // :835-838
    W.gt = __ballot(in && pos >= 1 && gc > gm);
    W.lt = __ballot(in && pos >= 1 && gc < gm);
    W.vc = gc;
    W.c = ch;
}

// g(p) for a wave-uniform p in [0, n]: from the held chunk, the one in flight, or memory.
__device__ __forceinline__ double g_uniform(const Plot &P, const Window &W, int p) {
    const int ch = p >> 6;
    if (ch == W.c) return uniform_lane(W.vc, p & 63);
    if (ch == W.c + 1) return P.conv(p, uniform_lane(W.nc, p & 63));
    return P.g(p);
}

// get_sda_end (:848-859) / get_sua_end (:860-871)
template <bool kDown>
__device__ __forceinline__ int area_end(const Plot &P, Window &W, int start, int min_pts, int lane, double omc) {
    int last = start;
    for (int i = start + 1; i < P.n; ++i) {
        if (i - last >= min_pts) return last;
        enter(P, W, i, lane, omc);
        const uint64_t bit = 1ull << (i & 63);
        if ((kDown ? W.gt : W.lt) & bit) return last;
        if ((kDown ? W.sd : W.su) & bit) last = i;
    }
    return max(P.n - 2, last);
}

// The SDA list of one wave: entry k in LDS for k < kLdsSdas, else in the wave's workspace slice.
// The spill words go through agent-scope atomics (the vector L1 is not coherent across lanes'
// stores), and a fence follows every phase that wrote them.
struct SdaList {
    volatile uint64_t *l_be;
    volatile double *l_mib, *l_gb;
    uint64_t *spill;
    int64_t spill_entries;
    int cnt;
    __device__ __forceinline__ void load(int k, uint64_t &be, double &mib, double &gb) const {
        if (k < kLdsSdas) {
            be = l_be[k], mib = l_mib[k], gb = l_gb[k];
        } else {
            const uint64_t *q = spill + (int64_t)(k - kLdsSdas) * 3;
            be = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mib = __longlong_as_double((long long)__hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            gb = __longlong_as_double((long long)__hip_atomic_load(q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
    }
    __device__ __forceinline__ bool fits(int k) const { return k < kLdsSdas + spill_entries; }
    __device__ __forceinline__ void store(int k, uint64_t be, double mib, double gb) const {  // fits(k)
        if (k < kLdsSdas) {
            l_be[k] = be, l_mib[k] = mib, l_gb[k] = gb;
            return;
        }
        uint64_t *q = spill + (int64_t)(k - kLdsSdas) * 3;
        __hip_atomic_store(q, be, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(q + 1, (uint64_t)__double_as_longlong(mib), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(q + 2, (uint64_t)__double_as_longlong(gb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void publish(int hi) const {
        if (hi > kLdsSdas) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    }
};

__device__ __forceinline__ int lanes_below(uint64_t mask, int lane) {
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// filter_sdas (:839-847): keep the entries with mib <= g(begin) * (1 - f) in order, then
// mib = max(mib, ...) on the survivors.  In place: a trip writes at or below what it has read.
__device__ __forceinline__ void filter_sdas(SdaList &L, double mib, double omf, int lane) {
    const int cnt = L.cnt;
    int out = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int k = base + lane;
        uint64_t be = 0;
        double m = 0.0, gb = 0.0;
        if (k < cnt) L.load(k, be, m, gb);
        const bool keep = k < cnt && mib <= gb * omf;
        const uint64_t mask = __ballot(keep);
        if (keep) L.store(out + lanes_below(mask, lane), be, m < mib ? mib : m, gb);  // std::max(sda.mib, mib)
        out += __popcll(mask);
    }
    L.publish(cnt);
    L.cnt = out;
}

// cluster_borders (:872-895) for one SDA (a lane each); in_range(a, b, range) is |a - b| <= range.
__device__ __forceinline__ void cluster_borders(const Plot &P, int b, int en, double start_reach, double end_reach,
                                                double chi, int sua_begin, int sua_end, int &ob, int &oe) {
    if (fabs(start_reach - end_reach) <= start_reach * chi) {
        ob = b, oe = sua_end;
    } else if (start_reach > end_reach) {
        int si = b + 1;
        while (si <= en && P.g(si) > end_reach) ++si;
        ob = si - 1, oe = sua_end;
    } else if (start_reach < end_reach) {
        int ei = sua_end;
        while (ei >= sua_begin && P.g(ei) >= start_reach) --ei;
        ob = b, oe = ei + 1;
    } else {
        ob = 0, oe = 0;
    }
}

__global__ __launch_bounds__(kNT) void optics_xi_kernel(const double *__restrict__ reach, int64_t n_segs,
                                                         int64_t stride, const int32_t *__restrict__ seg_counts,
                                                         double chi, int min_pts, double samd,
                                                         int32_t *__restrict__ clusters, int64_t cap,
                                                         int32_t *__restrict__ n_clusters, uint64_t *spill,
                                                         int64_t spill_entries, int32_t *flag) {
    __shared__ uint64_t s_be[kWaves][kLdsSdas];
    __shared__ double s_mib[kWaves][kLdsSdas], s_gb[kWaves][kLdsSdas];
    const int lane = ecc::lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t wg = (int64_t)blockIdx.x * kWaves + wave, n_waves = (int64_t)gridDim.x * kWaves;
    const double omc = 1 - chi, oms = 1.0 - samd;
    const double f = chi < samd ? samd : chi, omf = 1 - f;  // fplus::max(chi, steep_area_min_diff)
    SdaList L{s_be[wave], s_mib[wave], s_gb[wave], spill + wg * spill_entries * 3, spill_entries, 0};

    for (int64_t s = wg; s < n_segs; s += n_waves) {
        const int n = __builtin_amdgcn_readfirstlane(ecc::seg_points(seg_counts, stride, s));
        Plot P{reach + s * stride, n, 0.0};
        int64_t n_out = 0;
        bool guard = false;
        if (n >= 2) {  // fewer than 2 points: no clusters (the reference's n - 2 wraps)
            double m = 0.0;  // :819-820
            for (int64_t p = lane; p < n; p += 64) {
                const double r = P.r[p];
                if (r > m) m = r;
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const double o = __shfl_xor(m, off);
                if (o > m) m = o;
            }
            P.maxr = uniform_lane(m, 0);

            Window W;
            L.cnt = 0;
            double mib = 0.0;
            int32_t *out = clusters + s * cap * 2;
            for (int idx = 0; idx < n; ++idx) {  // :910-942
                enter(P, W, idx, lane, omc);
                const double reach_i = uniform_lane(W.vc, idx & 63);
                const uint64_t bit = 1ull << (idx & 63);
                if (W.sd & bit) {
                    if (reach_i > mib) mib = reach_i;
                    filter_sdas(L, mib, omf, lane);
                    const int e = area_end<true>(P, W, idx, min_pts, lane, omc);
                    if (reach_i * oms < g_uniform(P, W, e + 1)) continue;
                    // cnt <= n/2 + 1 fits for ordinary values (two SDAs begin at least 2 apart); the
                    // check keeps a plot of NaNs inside the workspace slice
                    if (L.fits(L.cnt)) {
                        if (lane == 0) L.store(L.cnt, (uint64_t)(uint32_t)idx | ((uint64_t)(uint32_t)e << 32), 0.0, reach_i);
                        L.publish(L.cnt + 1);
                        L.cnt += 1;
                    } else {
                        guard = true;
                    }
                    idx = e;
                    if (idx < n - 1) mib = g_uniform(P, W, idx + 1);
                } else if (W.su & bit) {
                    filter_sdas(L, mib, omf, lane);
                    const int e = area_end<false>(P, W, idx, min_pts, lane, omc);
                    const double after = g_uniform(P, W, e + 1);
                    if (reach_i > after * oms) continue;
                    const double thr = after * omf;                             // :898
                    const double end_reach = g_uniform(P, W, min(e + 1, n - 1));  // :874
                    const uint64_t sua_middle = (uint64_t)idx + (uint64_t)(e - idx) / 2;
                    for (int base = 0; base < L.cnt; base += 64) {  // :933-937
                        const int k = base + lane;
                        uint64_t be = 0;
                        double sm = 0.0, gb = 0.0;
                        if (k < L.cnt) L.load(k, be, sm, gb);
                        const int b = (int)(uint32_t)be, en = (int)(uint32_t)(be >> 32);
                        bool ok = k < L.cnt && !(sm > thr);
                        const uint64_t sda_middle = (uint64_t)b + (uint64_t)(en - b) / 2;
                        if (sua_middle - sda_middle < (uint64_t)min_pts - 2) ok = false;  // :900-904
                        const uint64_t mask = __ballot(ok);
                        const int64_t slot = n_out + lanes_below(mask, lane);
                        if (ok && slot < cap) {
                            int ob, oe;
                            cluster_borders(P, b, en, gb, end_reach, chi, idx, e, ob, oe);
                            out[slot * 2] = ob;
                            out[slot * 2 + 1] = oe;
                        }
                        n_out += __popcll(mask);
                    }
                    idx = e;
                    if (idx < n - 1) mib = g_uniform(P, W, idx + 1);
                } else {
                    if (reach_i > mib) mib = reach_i;
                }
            }
        }
        if (lane == 0) {
            n_clusters[s] = (int32_t)(n_out > INT32_MAX ? INT32_MAX : n_out);
            if (n_out > cap) *flag = 1;
        }
        if (guard && lane == 0) flag[1] = 1;
    }
}

}  // namespace

ECC_API int ecc_optics_xi(ecc_ctx *ctx, const double *reach, int64_t n_segs, int64_t seg_stride,
                          const int32_t *seg_counts, double chi, int32_t min_pts, double steep_area_min_diff,
                          int32_t *clusters, int64_t cap, int32_t *n_clusters, ecc_stream_t stream) {
    if (!ctx || n_segs < 0 || cap < 0 || seg_stride < 1 || seg_stride > INT32_MAX || !std::isfinite(chi) ||
        !(chi > 0.0 && chi < 1.0) || !std::isfinite(steep_area_min_diff) ||
        !(steep_area_min_diff >= 0.0 && steep_area_min_diff < 1.0) || min_pts < 2)
        return ECC_ERR_INVALID;
    if (n_segs > 0 && (!reach || !clusters || !n_clusters)) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    const unsigned grid = (unsigned)std::min<int64_t>((n_segs + kWaves - 1) / kWaves, kMaxBlocks);
    // SDAs begin at least 2 apart: at most n/2 + 1 of them; what LDS does not hold is spilled
    const int64_t spill_entries = std::max<int64_t>(0, seg_stride / 2 + 2 - kLdsSdas);
    const size_t ws_bytes = (size_t)grid * kWaves * (size_t)spill_entries * 24;
    if (int rc = ecc::ws_reserve(ctx, std::max<size_t>(ws_bytes, 64)); rc != ECC_OK) return rc;
    ECC_CHECK_HIP(ctx, hipMemsetAsync(ctx->dev->optics_xi, 0, 8, s), "memset(optics xi err)");
    ECC_TIMED(ctx, s, "optics_xi_kernel");
    hipLaunchKernelGGL(optics_xi_kernel, dim3(grid), dim3(kNT), 0, s, reach, n_segs, seg_stride, seg_counts, chi,
                       (int)min_pts, steep_area_min_diff, clusters, cap, n_clusters,
                       reinterpret_cast<uint64_t *>(ctx->ws), spill_entries, ctx->dev->optics_xi);
    ECC_CHECK_LAUNCH(ctx, "optics_xi");
    return ECC_OK;
}

ECC_API int ecc_optics_xi_status(ecc_ctx *ctx, ecc_stream_t stream) {
    if (!ctx) return ECC_ERR_INVALID;
    int32_t f[2] = {0, 0};
    if (int rc = ecc::read_dev_words(ctx, ctx->dev->optics_xi, 2, f, ecc::as_stream(stream))) return rc;
    return (f[0] | f[1]) ? ECC_ERR_CAPACITY : ECC_OK;
}

// Segments (waves) of optics_xi_kernel one compute unit holds at once, from the runtime's
// occupancy query for the kernel as built (registers and the 12 KiB of LDS per workgroup).
ECC_API int ecc_optics_xi_resident_segments(ecc_ctx *ctx, int32_t *per_cu) {
    if (!ctx || !per_cu) return ECC_ERR_INVALID;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    int blocks = 0;
    ECC_CHECK_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, optics_xi_kernel, kNT, 0),
                  "occupancy(optics_xi)");
    *per_cu = blocks * kWaves;
    return ECC_OK;
}
