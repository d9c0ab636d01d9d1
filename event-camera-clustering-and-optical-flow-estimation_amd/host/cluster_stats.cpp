// The statistics loop of the reference's OPTICS event driver (OPT/test/cluster_event_data.cpp:
// 472-527) on the host, for the intervals of one ordered plot of any length: size, centroid and
// per-axis variance of the points optics::get_cluster_points selects (optics.hpp:692-721,
// :724-774).  The reference's fp64 expressions in its operation order (-ffp-contract=off): one
// add per point for the sums, one multiply and one add per point for the variance chain.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/ecc.hpp"

extern "C" __attribute__((visibility("default"))) int ecc_cluster_stats_host(const uint32_t *xy, const int32_t *order,
                                                                             int64_t n, const int32_t *pairs,
                                                                             int64_t n_pairs, ecc_cluster_stat *stats) {
    if (n < 0 || n > INT32_MAX || n_pairs < 0 || (n > 0 && (!xy || !order)) || (n_pairs > 0 && (!pairs || !stats)))
        return ECC_ERR_INVALID;
    bool invalid = false;
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int64_t b = pairs[2 * k], e = pairs[2 * k + 1];
        bool ok = b >= 0 && b <= e && e < n;
        for (int64_t i = b; ok && i <= e; ++i) ok = order[i] >= 0 && order[i] < n;
        ecc_cluster_stat &r = stats[k];
        r = ecc_cluster_stat{(int32_t)b, 0, 0.0, 0.0, 0.0, 0.0};
        if (!ok) {
            invalid = true;
            continue;
        }
        const double m = (double)(e - b + 1);
        double sx = 0.0, sy = 0.0;  // :495-499
        for (int64_t i = b; i <= e; ++i) {
            const uint32_t w = xy[order[i]];
            sx += (double)(w & 0xffffu);
            sy += (double)(w >> 16);
        }
        const double cx = sx / m, cy = sy / m;  // :503-504
        double ax = 0.0, ay = 0.0;              // :511-520
        for (int64_t i = b; i <= e; ++i) {
            const uint32_t w = xy[order[i]];
            const double dx = (double)(w & 0xffffu) - cx;
            ax += dx * dx;
            const double dy = (double)(w >> 16) - cy;
            ay += dy * dy;
        }
        r.size = (int32_t)(e - b + 1);
        r.cx = cx, r.cy = cy, r.vx = ax / m, r.vy = ay / m;  // :525-526
    }
    return invalid ? ECC_ERR_INVALID : ECC_OK;
}

namespace ecc {
namespace optics {

namespace {

void check(int rc, const char *what) {
    if (rc != ECC_OK) throw Error(rc, what);
}

// records [s * cap + k], k < counts[s] (at most cap), of the device array into one vector per segment
std::vector<std::vector<cluster_stat<2>>> fetch(Context &ctx, const DeviceBuffer &d_stats, int64_t n_segs, int64_t cap,
                                                const std::vector<int32_t> &counts) {
    std::vector<ecc_cluster_stat> h((size_t)n_segs * (size_t)cap);
    d_stats.download(h.data(), h.size() * sizeof(ecc_cluster_stat), ctx.stream());
    ctx.sync();
    std::vector<std::vector<cluster_stat<2>>> result((size_t)n_segs);
    for (int64_t g = 0; g < n_segs; ++g) {
        const int64_t m = std::min<int64_t>(std::max<int32_t>(counts[(size_t)g], 0), cap);
        result[(size_t)g].reserve((size_t)m);
        for (int64_t k = 0; k < m; ++k) {
            const ecc_cluster_stat &r = h[(size_t)(g * cap + k)];
            result[(size_t)g].push_back({(std::size_t)r.begin, (std::size_t)r.size, {r.cx, r.cy}, {r.vx, r.vy}});
        }
    }
    return result;
}

}  // namespace

std::vector<std::vector<cluster_stat<2>>> cluster_statistics_windows(Context &ctx, const uint32_t *device_xy,
                                                                     const int32_t *device_order,
                                                                     const int32_t *device_cluster, int64_t n_segs,
                                                                     int64_t seg_stride,
                                                                     const int32_t *device_seg_counts) {
    if (n_segs < 0) check(ECC_ERR_INVALID, "ecc_cluster_stats_runs");
    ecc_stream_t s = ctx.stream();
    DeviceBuffer d_n(std::max<size_t>((size_t)n_segs, 1) * 4), d_stats;
    std::vector<int32_t> counts((size_t)n_segs);
    // a second pass with the largest count as capacity when the first guess was too small
    for (int64_t cap = 64;;) {
        d_stats.reserve(std::max<size_t>((size_t)n_segs * (size_t)cap, 1) * sizeof(ecc_cluster_stat));
        check(ecc_cluster_stats_runs(ctx.get(), device_xy, device_order, device_cluster, n_segs, seg_stride,
                                     device_seg_counts, d_stats.as<ecc_cluster_stat>(), cap, d_n.as<int32_t>(), s),
              "ecc_cluster_stats_runs");
        if (n_segs == 0) return {};
        d_n.download(counts.data(), (size_t)n_segs * 4, s);
        const int rc = ecc_cluster_stats_status(ctx.get(), s);
        if (rc == ECC_ERR_CAPACITY) {
            cap = *std::max_element(counts.begin(), counts.end());
            continue;
        }
        check(rc, "ecc_cluster_stats_runs");
        return fetch(ctx, d_stats, n_segs, cap, counts);
    }
}

std::vector<std::vector<cluster_stat<2>>> cluster_statistics_windows(Context &ctx, const uint32_t *device_xy,
                                                                     const int32_t *device_order,
                                                                     const int32_t *device_pairs, int64_t pair_cap,
                                                                     const int32_t *device_n_pairs, int64_t n_segs,
                                                                     int64_t seg_stride,
                                                                     const int32_t *device_seg_counts) {
    if (n_segs < 0 || pair_cap < 0) check(ECC_ERR_INVALID, "ecc_cluster_stats_pairs");
    ecc_stream_t s = ctx.stream();
    DeviceBuffer d_stats(std::max<size_t>((size_t)n_segs * (size_t)pair_cap, 1) * sizeof(ecc_cluster_stat));
    check(ecc_cluster_stats_pairs(ctx.get(), device_xy, device_order, device_pairs, pair_cap, device_n_pairs, n_segs,
                                  seg_stride, device_seg_counts, d_stats.as<ecc_cluster_stat>(), s),
          "ecc_cluster_stats_pairs");
    if (n_segs == 0) return {};
    std::vector<int32_t> counts((size_t)n_segs);
    check(ecc_memcpy_d2h(counts.data(), device_n_pairs, (size_t)n_segs * 4, s), "read n_pairs");
    check(ecc_cluster_stats_status(ctx.get(), s), "ecc_cluster_stats_pairs");
    return fetch(ctx, d_stats, n_segs, pair_cap, counts);
}

}  // namespace optics
}  // namespace ecc
