// optics::get_chi_clusters_flat (OPT/include/optics/optics.hpp:803-944) on the host, for one
// reachability plot of any length: the xi ("chi") extraction of nested clusters.  Every
// comparison is the reference's fp64 expression in its operation order (-ffp-contract=off).
// Decisions where the reference is unreadable or undefined (quirk register Q25-Q27):
// geom::in_range(a, b, range) is |a - b| <= range; fewer than 2 points give no clusters (the
// reference's n - 2 wraps); min_pts < 2 is rejected (min_pts - 2 wraps).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "optics_xi_pairs.hpp"

namespace {

struct SDA {  // :803-808
    int64_t begin_idx, end_idx;
    double mib;
};

// calls emit(begin, end) for every pair, in the reference's push order
template <class Emit>
void chi_clusters(const double *reach, int64_t n, double chi, int64_t min_pts, double steep_area_min_diff, Emit emit) {
    if (n < 2) return;
    std::vector<SDA> SDAs;
    double mib = 0, max_reach = 0.0;
    for (int64_t i = 0; i < n; ++i)
        if (reach[i] > max_reach) max_reach = reach[i];
    const auto g = [&](int64_t idx) -> double {  // get_reach_dist :823-829
        if (idx >= n || idx <= 0) return max_reach;
        const double r = reach[idx];
        return (r < 0) ? 2 * max_reach : r;
    };
    const auto is_steep_down_pt = [&](int64_t idx) {
        if (idx == 0) return true;
        if (idx + 1 >= n) return false;
        return g(idx + 1) <= g(idx) * (1 - chi);
    };
    const auto is_steep_up_pt = [&](int64_t idx) {
        if (idx + 1 >= n) return true;
        return g(idx + 1) * (1 - chi) >= g(idx);
    };
    const double f = std::max(chi, steep_area_min_diff);
    const auto filter_sdas = [&]() {  // :839-847
        SDAs.erase(std::remove_if(SDAs.begin(), SDAs.end(),
                                  [&](const SDA &sda) { return !(mib <= g(sda.begin_idx) * (1 - f)); }),
                   SDAs.end());
        for (auto &sda : SDAs) sda.mib = std::max(sda.mib, mib);
    };
    const auto get_sda_end = [&](int64_t start_idx) {  // :848-859
        int64_t last = start_idx;
        for (int64_t idx = start_idx + 1; idx < n; ++idx) {
            if (idx - last >= min_pts) return last;
            if (g(idx) > g(idx - 1)) return last;
            if (is_steep_down_pt(idx)) last = idx;
        }
        return std::max(n - 2, last);
    };
    const auto get_sua_end = [&](int64_t start_idx) {  // :860-871
        int64_t last = start_idx;
        for (int64_t idx = start_idx + 1; idx < n; ++idx) {
            if (idx - last >= min_pts) return last;
            if (g(idx) < g(idx - 1)) return last;
            if (is_steep_up_pt(idx)) last = idx;
        }
        return std::max(n - 2, last);
    };
    const auto cluster_borders = [&](const SDA &sda, int64_t sua_begin, int64_t sua_end, int64_t &b, int64_t &e) {
        const double start_reach = g(sda.begin_idx);  // :872-895
        const double end_reach = g(std::min(sua_end + 1, n - 1));
        if (std::fabs(start_reach - end_reach) <= start_reach * chi) {
            b = sda.begin_idx, e = sua_end;
        } else if (start_reach > end_reach) {
            int64_t start_idx = sda.begin_idx + 1;
            while (start_idx <= sda.end_idx && g(start_idx) > end_reach) start_idx++;
            b = start_idx - 1, e = sua_end;
        } else if (start_reach < end_reach) {
            int64_t end_idx = sua_end;
            while (end_idx >= sua_begin && g(end_idx) >= start_reach) end_idx--;
            b = sda.begin_idx, e = end_idx + 1;
        } else {
            b = 0, e = 0;
        }
    };
    const auto valid_combination = [&](const SDA &sda, int64_t sua_begin, int64_t sua_end) {  // :896-907
        if (sda.mib > g(sua_end + 1) * (1 - f)) return false;
        const uint64_t sda_middle = (uint64_t)sda.begin_idx + (uint64_t)(sda.end_idx - sda.begin_idx) / 2;
        const uint64_t sua_middle = (uint64_t)sua_begin + (uint64_t)(sua_end - sua_begin) / 2;
        return !(sua_middle - sda_middle < (uint64_t)min_pts - 2);
    };

    for (int64_t idx = 0; idx < n; idx++) {  // :910-942
        const double reach_i = g(idx);
        if (is_steep_down_pt(idx)) {
            if (reach_i > mib) mib = reach_i;
            filter_sdas();
            const int64_t sda_end = get_sda_end(idx);
            if (reach_i * (1.0 - steep_area_min_diff) < g(sda_end + 1)) continue;
            SDAs.push_back(SDA{idx, sda_end, 0.0});
            idx = sda_end;
            if (idx < n - 1) mib = g(idx + 1);
        } else if (is_steep_up_pt(idx)) {
            filter_sdas();
            const int64_t sua_end = get_sua_end(idx);
            if (reach_i > g(sua_end + 1) * (1.0 - steep_area_min_diff)) continue;
            for (const auto &sda : SDAs)
                if (valid_combination(sda, idx, sua_end)) {
                    int64_t b, e;
                    cluster_borders(sda, idx, sua_end, b, e);
                    emit(b, e);
                }
            idx = sua_end;
            if (idx < n - 1) mib = g(idx + 1);
        } else if (reach_i > mib) {
            mib = reach_i;
        }
    }
}

bool valid_params(double chi, int64_t min_pts, double samd) {
    return std::isfinite(chi) && chi > 0.0 && chi < 1.0 && std::isfinite(samd) && samd >= 0.0 && samd < 1.0 &&
           min_pts >= 2;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int ecc_optics_xi_host(const double *reach, int64_t n, double chi,
                                                                         int32_t min_pts, double steep_area_min_diff,
                                                                         int32_t *clusters, int64_t cap,
                                                                         int64_t *n_out) {
    if (n < 0 || n > INT32_MAX || cap < 0 || !n_out || (n > 0 && !reach) || (cap > 0 && !clusters) ||
        !valid_params(chi, min_pts, steep_area_min_diff))
        return ECC_ERR_INVALID;
    int64_t k = 0;
    chi_clusters(reach, n, chi, min_pts, steep_area_min_diff, [&](int64_t b, int64_t e) {
        if (k < cap) clusters[2 * k] = (int32_t)b, clusters[2 * k + 1] = (int32_t)e;
        ++k;
    });
    *n_out = k;
    return k > cap ? ECC_ERR_CAPACITY : ECC_OK;
}

namespace ecc {
namespace optics {

std::vector<std::pair<std::size_t, std::size_t>> get_chi_clusters_flat(const std::vector<reachability_dist> &reach_dists,
                                                                       double chi, std::size_t min_pts,
                                                                       double steep_area_min_diff) {
    if (min_pts > (std::size_t)INT32_MAX || !valid_params(chi, (int64_t)min_pts, steep_area_min_diff))
        throw Error(ECC_ERR_INVALID, "get_chi_clusters_flat");
    std::vector<double> r(reach_dists.size());
    for (std::size_t i = 0; i < r.size(); ++i) r[i] = reach_dists[i].reach_dist;
    std::vector<std::pair<std::size_t, std::size_t>> out;
    chi_clusters(r.data(), (int64_t)r.size(), chi, (int64_t)min_pts, steep_area_min_diff,
                 [&](int64_t b, int64_t e) { out.emplace_back((std::size_t)b, (std::size_t)e); });
    return out;
}

int64_t xi_pairs_on_device(Context &ctx, const double *device_reach, int64_t n_segs, int64_t seg_stride,
                           const int32_t *device_seg_counts, double chi, std::size_t min_pts,
                           double steep_area_min_diff, DeviceBuffer &d_pairs, DeviceBuffer &d_n,
                           std::vector<int32_t> &counts) {
    const auto check = [](int rc) {
        if (rc != ECC_OK) throw Error(rc, "ecc_optics_xi");
    };
    if (n_segs < 1 || min_pts > (std::size_t)INT32_MAX) check(ECC_ERR_INVALID);
    ecc_stream_t s = ctx.stream();
    d_n.reserve((size_t)n_segs * 4);
    counts.resize((size_t)n_segs);
    for (int64_t cap = 64;;) {
        d_pairs.reserve((size_t)n_segs * (size_t)std::max<int64_t>(cap, 1) * 8);
        check(ecc_optics_xi(ctx.get(), device_reach, n_segs, seg_stride, device_seg_counts, chi, (int32_t)min_pts,
                            steep_area_min_diff, d_pairs.as<int32_t>(), cap, d_n.as<int32_t>(), s));
        d_n.download(counts.data(), (size_t)n_segs * 4, s);
        const int rc = ecc_optics_xi_status(ctx.get(), s);
        if (rc == ECC_ERR_CAPACITY) {
            const int64_t most = *std::max_element(counts.begin(), counts.end());
            if (most <= cap) check(rc);  // the workspace check, not the pair capacity
            cap = most;
            continue;
        }
        check(rc);
        return cap;
    }
}

std::vector<std::vector<std::pair<std::size_t, std::size_t>>> get_chi_clusters_flat_windows(
    Context &ctx, const double *device_reach, int64_t n_segs, int64_t seg_stride, const int32_t *device_seg_counts,
    double chi, std::size_t min_pts, double steep_area_min_diff) {
    if (n_segs < 0) throw Error(ECC_ERR_INVALID, "ecc_optics_xi");
    std::vector<std::vector<std::pair<std::size_t, std::size_t>>> result((size_t)n_segs);
    if (n_segs == 0) {  // the parameter checks alone
        const int rc = min_pts > (std::size_t)INT32_MAX
                           ? ECC_ERR_INVALID
                           : ecc_optics_xi(ctx.get(), device_reach, 0, seg_stride, device_seg_counts, chi,
                                           (int32_t)min_pts, steep_area_min_diff, nullptr, 0, nullptr, ctx.stream());
        if (rc != ECC_OK) throw Error(rc, "ecc_optics_xi");
        return result;
    }
    DeviceBuffer d_n, d_pairs;
    std::vector<int32_t> counts, pairs;
    const int64_t cap = xi_pairs_on_device(ctx, device_reach, n_segs, seg_stride, device_seg_counts, chi, min_pts,
                                           steep_area_min_diff, d_pairs, d_n, counts);
    pairs.resize((size_t)n_segs * (size_t)cap * 2);
    d_pairs.download(pairs.data(), pairs.size() * 4, ctx.stream());
    ctx.sync();
    for (int64_t g = 0; g < n_segs; ++g)
        for (int64_t k = 0; k < counts[(size_t)g]; ++k)
            result[(size_t)g].emplace_back((std::size_t)pairs[(size_t)((g * cap + k) * 2)],
                                           (std::size_t)pairs[(size_t)((g * cap + k) * 2 + 1)]);
    return result;
}

}  // namespace optics
}  // namespace ecc
