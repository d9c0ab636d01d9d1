// Size, centroid and per-axis variance of every cluster of every segment in one launch: the loop of
// the reference's OPTICS event driver (OPT/test/cluster_event_data.cpp:472-527) over the points
// optics::get_cluster_points selects (OPT/include/optics/optics.hpp:692-721 for the threshold
// clusters, :724-774 for xi pairs), on the order / cluster / pairs arrays that ecc_optics_grid and
// ecc_optics_xi leave on the device.
//
// A cluster is an interval [begin, end] of one segment's ordered plot.  The sums of the
// coordinates are integers below 2^30 (at most 8192 points of at most 65535), exact in any order;
// the variance chain acc += d * d rounds at every step, so it is walked serially in plot order
// with a separate multiply and add (the build is -ffp-contract=off).  The parallelism is across
// clusters, across the two axes and across segments:
//   * one workgroup per segment, segments beyond the grid strided;
//   * xy[order[i]] is gathered into LDS in plot order (4 bytes per point of the stride);
//   * runs form: the run starts become a bit per position (ballots), the bits a list of begins
//     by a count-and-prefix over the 128 mask words (2 bytes per point of the stride);
//   * a lane per (cluster, axis): an integer sum walk for the centroid, then the chain, four
//     LDS reads and four d * d ahead of four dependent adds.
// Nothing grows with the number of clusters beyond the segment's length, and every loop is bounded
// by it whatever the values are: an order entry outside the segment is never used as an index, and
// a pair outside it never reaches the walk.
//
// The lists form (ecc_cluster_stats_lists) walks the intervals of ecc_dbscan_lists' `members` rows,
// which name their points directly and may be longer than the segment (a membership given twice):
// the row takes the place of `order`, xy[members[i]] is gathered into LDS in list order (up to
// kListLds entries of the row; an interval that reaches past them, fabricated input only, is walked
// through global memory), and the walk is the pairs form's.  A members value outside the segment
// refuses the record, as an order entry does.
#include "ecc_internal.hpp"

#include <algorithm>

namespace {

constexpr int kNT = 256;
constexpr int kMaxStride = 8192;
constexpr int kMaskWords = kMaxStride / 64;
constexpr int kListLds = 16384;  // entries of a members row gathered into LDS (lists form)
constexpr int kMaxBlocks = 2048;  // 8 per CU on 256 CUs; LDS admits 3 (runs) or 4 (pairs) at stride 8192

__device__ __forceinline__ uint32_t axis_of(uint32_t w, int sh) { return (w >> sh) & 0xffffu; }

// One axis of one cluster [b, e] of the points pt(i): centroid and variance, the reference's
// expressions (:497-526): sum / (double)m, then acc += d * d in plot order, acc / (double)m.
template <class Pt>
__device__ __forceinline__ void axis_stats(Pt pt, int b, int e, int sh, double &c, double &v) {
    uint32_t sum = 0;
    for (int i = b; i <= e; ++i) sum += axis_of(pt(i), sh);
    const double m = (double)(e - b + 1);
    c = (double)sum / m;
    double acc = 0.0;
    int i = b;
    for (; i + 3 <= e; i += 4) {
        const double d0 = (double)axis_of(pt(i), sh) - c, d1 = (double)axis_of(pt(i + 1), sh) - c;
        const double d2 = (double)axis_of(pt(i + 2), sh) - c, d3 = (double)axis_of(pt(i + 3), sh) - c;
        const double t0 = d0 * d0, t1 = d1 * d1, t2 = d2 * d2, t3 = d3 * d3;
        acc += t0;
        acc += t1;
        acc += t2;
        acc += t3;
    }
    for (; i <= e; ++i) {
        const double d = (double)axis_of(pt(i), sh) - c;
        acc += d * d;
    }
    v = acc / m;
}

enum Form { kFormRuns, kFormPairs, kFormLists };

// kForm == kFormLists: `order` is the members array, rows of `order_stride` entries of which segment s
// holds min(order_len[s], order_stride); the first `list_lds` of them are gathered.
template <Form kForm>
__global__ __launch_bounds__(kNT) void cluster_stats_kernel(const uint32_t *__restrict__ xy,
                                                            const int32_t *__restrict__ order,
                                                            const int32_t *__restrict__ src,  // cluster ids | pairs
                                                            const int32_t *__restrict__ n_src,  // - | n_pairs
                                                            int64_t n_segs, int64_t stride,
                                                            const int32_t *__restrict__ seg_counts,
                                                            ecc_cluster_stat *__restrict__ stats, int64_t cap,
                                                            int32_t *__restrict__ n_stats, int32_t *flag,
                                                            int64_t order_stride, const int64_t *__restrict__ order_len,
                                                            int list_lds) {
    constexpr bool kRuns = kForm == kFormRuns, kLists = kForm == kFormLists;
    constexpr int kBadWords = kLists ? kListLds / 64 : kMaskWords;
    extern __shared__ uint32_t s_mem[];
    uint32_t *s_xy = s_mem;                                             // [stride] points in plot order
    uint16_t *s_beg = reinterpret_cast<uint16_t *>(s_mem + stride);     // [stride] run begins (runs form)
    static_assert(kListLds / 64 == kNT, "a thread per mask word of a gathered row");
    __shared__ uint64_t s_start[kLists ? 1 : kMaskWords], s_bad[kBadWords];  // a bit per plot position
    __shared__ int s_wave_total[kNT / 64], s_any_bad;
    const int tid = (int)threadIdx.x, lane = ecc::lane_id(), wave = tid >> 6;

    for (int64_t s = blockIdx.x; s < n_segs; s += gridDim.x) {
        const int n = ecc::seg_points(seg_counts, stride, s);
        const int64_t seg = s * stride;
        if (kLists) s_bad[tid] = 0;
        else if (tid < kMaskWords) s_start[tid] = 0, s_bad[tid] = 0;
        if (tid == 0) s_any_bad = 0;
        __syncthreads();
        const int32_t *row = kLists ? order + s * order_stride : order + seg;
        int64_t row_len = n;
        if (kLists) {
            row_len = order_len[s];
            row_len = row_len < 0 ? 0 : (row_len < order_stride ? row_len : order_stride);
        }
        const int n_plot = kLists ? (int)(row_len < list_lds ? row_len : list_lds) : n;  // positions gathered

        // gather in plot order; a wave's 64 positions are one mask word, written by its lane 0
        for (int base = 0; base < n_plot; base += kNT) {
            const int i = base + tid;
            const bool in = i < n_plot;
            const int o = in ? row[i] : 0;
            const bool bad = in && (uint32_t)o >= (uint32_t)n;
            if (in) s_xy[i] = bad ? 0u : xy[seg + o];
            const uint64_t bad_mask = __ballot(bad);
            uint64_t start_mask = 0;
            if (kRuns) start_mask = __ballot(in && (i == 0 || src[seg + i] != src[seg + i - 1]));
            if (lane == 0) {
                s_bad[i >> 6] = bad_mask;
                if (kRuns) s_start[i >> 6] = start_mask;
                if (bad_mask) s_any_bad = 1;
            }
        }
        __syncthreads();

        int n_all = 0;  // runs of the segment | pairs of the segment
        if (kRuns) {
            // begins, in order: thread t owns mask word t; exclusive prefix of the words' counts
            const uint64_t w = tid < kMaskWords ? s_start[tid] : 0;
            const int c = __popcll(w), incl = ecc::wave_incl_scan(c);
            if (lane == 63) s_wave_total[wave] = incl;
            __syncthreads();
            int k = incl - c;
            for (int v = 0; v < kNT / 64; ++v) {
                if (v < wave) k += s_wave_total[v];
                n_all += s_wave_total[v];
            }
            for (uint64_t rest = w; rest; rest &= rest - 1) s_beg[k++] = (uint16_t)(tid * 64 + __ffsll((long long)rest) - 1);
            __syncthreads();
        } else {
            n_all = n_src[s];
            n_all = n_all < 0 ? 0 : n_all;
        }
        const int n_out = (int)(n_all < cap ? n_all : cap);
        const bool any_bad = s_any_bad != 0;
        if (tid == 0) {
            if (kRuns) {
                n_stats[s] = n_all;
                if (n_all > cap) flag[0] = 1;
            }
            if (any_bad) flag[1] = 1;
        }

        // a lane per (cluster, axis): lanes 2k and 2k + 1 share record k
        ecc_cluster_stat *out = stats + s * cap;
        for (int64_t q = tid; q < 2 * (int64_t)n_out; q += kNT) {
            const int k = (int)(q >> 1), axis = (int)(q & 1);
            int b, e;
            bool ok = true;
            if (kRuns) {
                b = s_beg[k];
                e = (k + 1 < n_all ? (int)s_beg[k + 1] : n) - 1;
            } else {
                b = src[(s * cap + k) * 2], e = src[(s * cap + k) * 2 + 1];
                ok = b >= 0 && b <= e && (kLists ? e < row_len : e < n);
                if (!ok) flag[1] = 1;
            }
            const bool far = kLists && ok && e >= n_plot;  // past the gathered part of a long row
            if (far) {
                for (int i = b; i <= e && ok; ++i) ok = (uint32_t)row[i] < (uint32_t)n;
                if (!ok) flag[1] = 1;
            } else if (ok && any_bad) {  // rare: does the interval hold a position whose order entry was refused?
                for (int i = b; i <= e && ok; ++i) ok = !((s_bad[i >> 6] >> (i & 63)) & 1);
            }
            double c = 0.0, v = 0.0;
            if (ok) {
                if (far) axis_stats([&](int i) { return xy[seg + row[i]]; }, b, e, axis * 16, c, v);
                else axis_stats([&](int i) { return s_xy[i]; }, b, e, axis * 16, c, v);
            }
            if (axis == 0) {
                out[k].begin = b, out[k].size = ok ? e - b + 1 : 0;
                out[k].cx = c, out[k].vx = v;
            } else {
                out[k].cy = c, out[k].vy = v;
            }
        }
        __syncthreads();  // the next segment overwrites LDS
    }
}

int launch(ecc_ctx *ctx, Form form, const uint32_t *xy, const int32_t *order, const int32_t *src,
           const int32_t *n_src, int64_t n_segs, int64_t stride, const int32_t *seg_counts, ecc_cluster_stat *stats,
           int64_t cap, int32_t *n_stats, ecc_stream_t stream, int64_t order_stride = 0,
           const int64_t *order_len = nullptr) {
    const bool runs = form == kFormRuns;
    const int list_lds = (int)std::min<int64_t>(std::max<int64_t>(order_stride, 1), kListLds);
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    const unsigned grid = (unsigned)std::min<int64_t>(n_segs, kMaxBlocks);
    const size_t lds = form == kFormLists ? (size_t)list_lds * 4
                                          : (size_t)stride * 4 + (runs ? ecc::align_up((size_t)stride * 2, 4) : 0);
    if (form == kFormLists)
        if (int rc = ecc::allow_dynamic_lds(ctx, cluster_stats_kernel<kFormLists>, (int)lds, "cluster_stats_lists LDS"))
            return rc;
    ECC_CHECK_HIP(ctx, hipMemsetAsync(ctx->dev->cluster_stats, 0, 8, s), "memset(cluster stats err)");
    ECC_TIMED(ctx, s, runs ? "cluster_stats_runs_kernel"
                           : (form == kFormPairs ? "cluster_stats_pairs_kernel" : "cluster_stats_lists_kernel"));
    if (runs)
        hipLaunchKernelGGL(cluster_stats_kernel<kFormRuns>, dim3(grid), dim3(kNT), lds, s, xy, order, src, n_src, n_segs,
                           stride, seg_counts, stats, cap, n_stats, ctx->dev->cluster_stats, order_stride, order_len, list_lds);
    else if (form == kFormPairs)
        hipLaunchKernelGGL(cluster_stats_kernel<kFormPairs>, dim3(grid), dim3(kNT), lds, s, xy, order, src, n_src, n_segs,
                           stride, seg_counts, stats, cap, n_stats, ctx->dev->cluster_stats, order_stride, order_len, list_lds);
    else
        hipLaunchKernelGGL(cluster_stats_kernel<kFormLists>, dim3(grid), dim3(kNT), lds, s, xy, order, src, n_src, n_segs,
                           stride, seg_counts, stats, cap, n_stats, ctx->dev->cluster_stats, order_stride, order_len, list_lds);
    ECC_CHECK_LAUNCH(ctx, "cluster_stats");
    return ECC_OK;
}

}  // namespace

ECC_API int ecc_cluster_stats_runs(ecc_ctx *ctx, const uint32_t *xy, const int32_t *order, const int32_t *cluster,
                                   int64_t n_segs, int64_t seg_stride, const int32_t *seg_counts,
                                   ecc_cluster_stat *stats, int64_t cap, int32_t *n_stats, ecc_stream_t stream) {
    if (!ctx || n_segs < 0 || cap < 0 || seg_stride < 1 || seg_stride > kMaxStride) return ECC_ERR_INVALID;
    if (n_segs > 0 && (!xy || !order || !cluster || !stats || !n_stats)) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    return launch(ctx, kFormRuns, xy, order, cluster, nullptr, n_segs, seg_stride, seg_counts, stats, cap, n_stats, stream);
}

ECC_API int ecc_cluster_stats_pairs(ecc_ctx *ctx, const uint32_t *xy, const int32_t *order, const int32_t *pairs,
                                    int64_t pair_cap, const int32_t *n_pairs, int64_t n_segs, int64_t seg_stride,
                                    const int32_t *seg_counts, ecc_cluster_stat *stats, ecc_stream_t stream) {
    if (!ctx || n_segs < 0 || pair_cap < 0 || seg_stride < 1 || seg_stride > kMaxStride) return ECC_ERR_INVALID;
    if (n_segs > 0 && (!xy || !order || !pairs || !n_pairs || !stats)) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    return launch(ctx, kFormPairs, xy, order, pairs, n_pairs, n_segs, seg_stride, seg_counts, stats, pair_cap, nullptr,
                  stream);
}

ECC_API int ecc_cluster_stats_lists(ecc_ctx *ctx, const uint32_t *xy, const int32_t *members, int64_t member_stride,
                                    const int64_t *n_members, const int32_t *pairs, int64_t pair_cap,
                                    const int32_t *n_pairs, int64_t n_segs, int64_t seg_stride,
                                    const int32_t *seg_counts, ecc_cluster_stat *stats, ecc_stream_t stream) {
    if (!ctx || n_segs < 0 || pair_cap < 0 || seg_stride < 1 || seg_stride > kMaxStride) return ECC_ERR_INVALID;
    if (member_stride < 0 || member_stride > INT32_MAX) return ECC_ERR_INVALID;
    if (n_segs > 0 && (!xy || !members || !n_members || !pairs || !n_pairs || !stats)) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    return launch(ctx, kFormLists, xy, members, pairs, n_pairs, n_segs, seg_stride, seg_counts, stats, pair_cap, nullptr,
                  stream, member_stride, n_members);
}

ECC_API int ecc_cluster_stats_status(ecc_ctx *ctx, ecc_stream_t stream) {
    if (!ctx) return ECC_ERR_INVALID;
    int32_t f[2] = {0, 0};
    if (int rc = ecc::read_dev_words(ctx, ctx->dev->cluster_stats, 2, f, ecc::as_stream(stream))) return rc;
    return f[1] ? ECC_ERR_INVALID : (f[0] ? ECC_ERR_CAPACITY : ECC_OK);
}
