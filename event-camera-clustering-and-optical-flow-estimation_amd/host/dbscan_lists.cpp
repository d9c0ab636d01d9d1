// What DBSCANSimpleCluster::extract returns (PCC/DBSCAN_simple.h:27-90; read cluster by cluster at
// PCC/pcl_cluster.cpp:131-142) from one segment's labels and further memberships, on the host: a
// push_back per label and per dup pair, then std::sort per cluster (:82), laid out as
// ecc_dbscan_lists lays it out on the device (members, {begin, end} pairs, n_members).
// Also the C++ entries that run the device route for many windows.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/ecc.hpp"

extern "C" __attribute__((visibility("default"))) int ecc_dbscan_lists_host(
    const int32_t *labels, int64_t n, int32_t n_clusters, const int64_t *dups, int64_t n_dups, int32_t *members,
    int64_t member_cap, int64_t *n_members, int32_t *pairs, int64_t pair_cap) {
    if (n < 0 || n > INT32_MAX || n_dups < 0 || member_cap < 0 || pair_cap < 0 || !n_members) return ECC_ERR_INVALID;
    if ((n > 0 && !labels) || (n_dups > 0 && !dups)) return ECC_ERR_INVALID;
    bool invalid = n_clusters < 0;
    const int64_t nc = n_clusters < 0 ? 0 : n_clusters;
    // memberships first, so that a list too large for its room is never built
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (labels[i] >= 0 && labels[i] < nc) ++total;
        else if (labels[i] != -1) invalid = true;
    }
    for (int64_t k = 0; k < n_dups; ++k) {
        const int64_t p = dups[2 * k], c = dups[2 * k + 1];
        if (p >= 0 && p < n && c >= 0 && c < nc) ++total;
        else invalid = true;
    }
    *n_members = total;
    if (total > member_cap || nc > pair_cap) return invalid ? ECC_ERR_INVALID : ECC_ERR_CAPACITY;
    if ((total > 0 && !members) || (nc > 0 && !pairs)) return ECC_ERR_INVALID;

    std::vector<std::vector<int>> lists((size_t)nc);
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] >= 0 && labels[i] < nc) lists[(size_t)labels[i]].push_back((int)i);
    for (int64_t k = 0; k < n_dups; ++k) {
        const int64_t p = dups[2 * k], c = dups[2 * k + 1];
        if (p >= 0 && p < n && c >= 0 && c < nc) lists[(size_t)c].push_back((int)p);
    }
    int64_t at = 0;
    for (int64_t c = 0; c < nc; ++c) {
        std::vector<int> &m = lists[(size_t)c];
        std::sort(m.begin(), m.end());  // :82
        pairs[2 * c] = (int32_t)at;
        for (int v : m) members[at++] = v;
        pairs[2 * c + 1] = (int32_t)(at - 1);
    }
    return invalid ? ECC_ERR_INVALID : ECC_OK;
}

namespace ecc {

namespace {

void check(int rc, const char *what) {
    if (rc != ECC_OK) throw Error(rc, what);
}

// The lists of every window on the device: members rows of `member_stride`, pairs rows of `pair_cap`.
struct DeviceLists {
    DeviceBuffer members, n_members, pairs, n_clusters;
    int64_t member_stride = 0, pair_cap = 0;
    std::vector<int64_t> counts;    // memberships per window
    std::vector<int32_t> clusters;  // clusters per window
};

// ecc_dbscan_grid, then ecc_dbscan_lists; the dup room and the rows grow to what the device reports.
DeviceLists lists_of_windows(Context &ctx, const uint32_t *device_xy, int64_t n_segs, int64_t seg_stride,
                             const int32_t *device_seg_counts, double eps, int min_pts, int min_cluster_size,
                             int max_cluster_size) {
    if (n_segs < 0 || seg_stride < 1) check(ECC_ERR_INVALID, "ecc_dbscan_grid");
    DeviceLists L;
    if (n_segs == 0) return L;
    ecc_stream_t s = ctx.stream();
    const size_t n = (size_t)n_segs * (size_t)seg_stride;
    DeviceBuffer d_lab(n * 4), d_nd(8), d_dups;
    L.n_clusters.reserve((size_t)n_segs * 4);
    DeviceBuffer &d_nc = L.n_clusters;
    int64_t dup_cap = std::max<int64_t>((int64_t)n / 8, 1024), nd = 0;
    for (;;) {
        d_dups.reserve((size_t)dup_cap * 16);
        check(ecc_dbscan_grid(ctx.get(), device_xy, n_segs, seg_stride, device_seg_counts, eps, min_pts,
                              min_cluster_size, max_cluster_size, d_lab.as<int32_t>(), d_nc.as<int32_t>(),
                              d_dups.as<int64_t>(), dup_cap, d_nd.as<int64_t>(), s),
              "ecc_dbscan_grid");
        const int st = ecc_dbscan_status(ctx.get(), s);
        d_nd.download(&nd, 8, s);
        ctx.sync();
        if (st == ECC_ERR_CAPACITY && nd > dup_cap) {
            dup_cap = nd;
            continue;
        }
        check(st, "ecc_dbscan_grid");
        break;
    }
    L.clusters.resize((size_t)n_segs);
    L.counts.resize((size_t)n_segs);
    d_nc.download(L.clusters.data(), (size_t)n_segs * 4, s);
    ctx.sync();
    L.pair_cap = std::max<int32_t>(*std::max_element(L.clusters.begin(), L.clusters.end()), 1);
    L.member_stride = seg_stride;
    L.n_members.reserve((size_t)n_segs * 8);
    L.pairs.reserve((size_t)n_segs * (size_t)L.pair_cap * 8);
    for (;;) {  // a second pass with the largest count as stride when a window has double memberships past it
        L.members.reserve((size_t)n_segs * (size_t)L.member_stride * 4);
        check(ecc_dbscan_lists(ctx.get(), d_lab.as<int32_t>(), d_nc.as<int32_t>(), d_dups.as<int64_t>(), dup_cap,
                               d_nd.as<int64_t>(), n_segs, seg_stride, device_seg_counts, L.members.as<int32_t>(),
                               L.member_stride, L.n_members.as<int64_t>(), L.pairs.as<int32_t>(), L.pair_cap, s),
              "ecc_dbscan_lists");
        const int st = ecc_dbscan_lists_status(ctx.get(), s);
        L.n_members.download(L.counts.data(), (size_t)n_segs * 8, s);
        ctx.sync();
        const int64_t most = *std::max_element(L.counts.begin(), L.counts.end());
        if (st == ECC_ERR_CAPACITY && most > L.member_stride) {
            L.member_stride = most;
            continue;
        }
        check(st, "ecc_dbscan_lists");
        return L;
    }
}

}  // namespace

std::vector<std::vector<PointIndices>> dbscan_extract_windows(Context &ctx, const uint32_t *device_xy, int64_t n_segs,
                                                              int64_t seg_stride, const int32_t *device_seg_counts,
                                                              double eps, int min_pts, int min_cluster_size,
                                                              int max_cluster_size) {
    const DeviceLists L = lists_of_windows(ctx, device_xy, n_segs, seg_stride, device_seg_counts, eps, min_pts,
                                           min_cluster_size, max_cluster_size);
    std::vector<std::vector<PointIndices>> result((size_t)std::max<int64_t>(n_segs, 0));
    if (n_segs <= 0) return result;
    ecc_stream_t s = ctx.stream();
    std::vector<int32_t> members((size_t)n_segs * (size_t)L.member_stride), pairs((size_t)n_segs * (size_t)L.pair_cap * 2);
    L.members.download(members.data(), members.size() * 4, s);
    L.pairs.download(pairs.data(), pairs.size() * 4, s);
    ctx.sync();
    for (int64_t g = 0; g < n_segs; ++g) {
        const int32_t *row = members.data() + g * L.member_stride;
        result[(size_t)g].resize((size_t)L.clusters[(size_t)g]);
        for (int32_t c = 0; c < L.clusters[(size_t)g]; ++c) {
            const int32_t b = pairs[(size_t)((g * L.pair_cap + c) * 2)], e = pairs[(size_t)((g * L.pair_cap + c) * 2 + 1)];
            result[(size_t)g][(size_t)c].indices.assign(row + b, row + e + 1);
        }
    }
    return result;
}

std::vector<std::vector<optics::cluster_stat<2>>> dbscan_statistics_windows(
    Context &ctx, const uint32_t *device_xy, int64_t n_segs, int64_t seg_stride, const int32_t *device_seg_counts,
    double eps, int min_pts, int min_cluster_size, int max_cluster_size) {
    const DeviceLists L = lists_of_windows(ctx, device_xy, n_segs, seg_stride, device_seg_counts, eps, min_pts,
                                           min_cluster_size, max_cluster_size);
    std::vector<std::vector<optics::cluster_stat<2>>> result((size_t)std::max<int64_t>(n_segs, 0));
    if (n_segs <= 0) return result;
    ecc_stream_t s = ctx.stream();
    DeviceBuffer d_stats((size_t)n_segs * (size_t)L.pair_cap * sizeof(ecc_cluster_stat));
    check(ecc_cluster_stats_lists(ctx.get(), device_xy, L.members.as<int32_t>(), L.member_stride,
                                  L.n_members.as<int64_t>(), L.pairs.as<int32_t>(), L.pair_cap, L.n_clusters.as<int32_t>(),
                                  n_segs, seg_stride, device_seg_counts, d_stats.as<ecc_cluster_stat>(), s),
          "ecc_cluster_stats_lists");
    check(ecc_cluster_stats_status(ctx.get(), s), "ecc_cluster_stats_lists");
    std::vector<ecc_cluster_stat> h((size_t)n_segs * (size_t)L.pair_cap);
    d_stats.download(h.data(), h.size() * sizeof(ecc_cluster_stat), s);
    ctx.sync();
    for (int64_t g = 0; g < n_segs; ++g)
        for (int32_t c = 0; c < L.clusters[(size_t)g]; ++c) {
            const ecc_cluster_stat &r = h[(size_t)(g * L.pair_cap + c)];
            result[(size_t)g].push_back({(std::size_t)r.begin, (std::size_t)r.size, {r.cx, r.cy}, {r.vx, r.vy}});
        }
    return result;
}

}  // namespace ecc
