// optics::flat_clusters_to_tree and optics::get_chi_clusters (OPT/include/optics/optics.hpp:948-995,
// :1018-1021) on the host: the reference's two loops, literally, on (first, second) pairs in
// get_chi_clusters_flat's push order; and the forests of many device-resident plots built from the
// (sorted, parent) arrays ecc_optics_xi_tree leaves.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "optics_xi_pairs.hpp"

extern "C" __attribute__((visibility("default"))) int ecc_optics_xi_tree_host(const int32_t *pairs, int64_t n_pairs,
                                                                              int32_t *sorted, int32_t *parent,
                                                                              int32_t *level, int64_t *n_roots) {
    if (n_pairs < 0 || n_pairs > INT32_MAX || !n_roots || (n_pairs > 0 && (!pairs || !sorted || !parent)))
        return ECC_ERR_INVALID;
    const int64_t P = n_pairs;
    // :950-966 — children before their parents: entry idx goes `run` free slots past the cursor,
    // run = the following entries whose second does not exceed its own
    std::vector<char> filled((size_t)P, 0);
    int64_t next_free = 0;
    for (int64_t idx = 0; idx < P; ++idx) {
        while (next_free < P && filled[(size_t)next_free]) ++next_free;
        int64_t pos = next_free;
        for (int64_t following = idx + 1; following < P && pairs[2 * following + 1] <= pairs[2 * idx + 1]; ++following)
            ++pos;
        // the runs nest, so the slot is free and inside the list (the reference's assert, :966)
        if (pos >= P || filled[(size_t)pos]) return ECC_ERR_INVALID;
        filled[(size_t)pos] = 1;
        sorted[2 * pos] = pairs[2 * idx], sorted[2 * pos + 1] = pairs[2 * idx + 1];
    }
    // :974-992 — the first later entry whose interval holds this one's
    int64_t roots = 0;
    for (int64_t k = 0; k < P; ++k) {
        int64_t j = k + 1;
        while (j < P && !(sorted[2 * k] >= sorted[2 * j] && sorted[2 * k + 1] <= sorted[2 * j + 1])) ++j;
        parent[k] = j < P ? (int32_t)j : -1;
        roots += j >= P;
    }
    if (level)
        for (int64_t k = P - 1; k >= 0; --k) level[k] = parent[k] < 0 ? 0 : level[parent[k]] + 1;
    *n_roots = roots;
    return ECC_OK;
}

namespace ecc {
namespace optics {

namespace {

using TreeNode = Node<chi_cluster_indices>;

// The reference's second loop (:984-992) on the parents already found: a node is complete when its
// turn comes, because its children stand before it.
std::vector<cluster_tree> forest(const int32_t *sorted, const int32_t *parent, int64_t n) {
    std::vector<TreeNode> nodes;
    nodes.reserve((size_t)std::max<int64_t>(n, 0));
    for (int64_t k = 0; k < n; ++k)
        nodes.emplace_back(chi_cluster_indices((std::size_t)sorted[2 * k], (std::size_t)sorted[2 * k + 1]));
    std::vector<cluster_tree> result;
    for (int64_t k = 0; k < n; ++k) {
        if (parent[k] < 0) result.emplace_back(std::move(nodes[(size_t)k]));
        else nodes[(size_t)parent[k]].get_children().push_back(std::move(nodes[(size_t)k]));
    }
    return result;
}

void check(int rc, const char *what) {
    if (rc != ECC_OK) throw Error(rc, what);
}

}  // namespace

std::vector<cluster_tree> flat_clusters_to_tree(const std::vector<chi_cluster_indices> &clusters_flat) {
    const size_t n = clusters_flat.size();
    if (n > (size_t)INT32_MAX) check(ECC_ERR_INVALID, "flat_clusters_to_tree");
    std::vector<int32_t> pairs(n * 2), sorted(n * 2), parent(n);
    for (size_t k = 0; k < n; ++k) {
        if (clusters_flat[k].first > (size_t)INT32_MAX || clusters_flat[k].second > (size_t)INT32_MAX)
            check(ECC_ERR_INVALID, "flat_clusters_to_tree");
        pairs[2 * k] = (int32_t)clusters_flat[k].first, pairs[2 * k + 1] = (int32_t)clusters_flat[k].second;
    }
    int64_t n_roots = 0;
    check(ecc_optics_xi_tree_host(pairs.data(), (int64_t)n, sorted.data(), parent.data(), nullptr, &n_roots),
          "ecc_optics_xi_tree_host");
    return forest(sorted.data(), parent.data(), (int64_t)n);
}

std::vector<cluster_tree> get_chi_clusters(const std::vector<reachability_dist> &reach_dists, double chi,
                                           std::size_t min_pts, double steep_area_min_diff) {
    return flat_clusters_to_tree(get_chi_clusters_flat(reach_dists, chi, min_pts, steep_area_min_diff));
}

std::vector<std::vector<cluster_tree>> get_chi_clusters_windows(Context &ctx, const double *device_reach,
                                                                int64_t n_segs, int64_t seg_stride,
                                                                const int32_t *device_seg_counts, double chi,
                                                                std::size_t min_pts, double steep_area_min_diff) {
    if (n_segs <= 0)  // its checks; no segments, no forests
        return std::vector<std::vector<cluster_tree>>(get_chi_clusters_flat_windows(
            ctx, device_reach, n_segs, seg_stride, device_seg_counts, chi, min_pts, steep_area_min_diff).size());
    std::vector<std::vector<cluster_tree>> result((size_t)n_segs);
    ecc_stream_t s = ctx.stream();
    DeviceBuffer d_n, d_pairs;
    std::vector<int32_t> counts;
    const int64_t cap = xi_pairs_on_device(ctx, device_reach, n_segs, seg_stride, device_seg_counts, chi, min_pts,
                                           steep_area_min_diff, d_pairs, d_n, counts);
    const size_t slots = (size_t)n_segs * (size_t)cap;
    DeviceBuffer d_sorted(slots * 8), d_parent(slots * 4), d_roots((size_t)n_segs * 4);
    check(ecc_optics_xi_tree(ctx.get(), d_pairs.as<int32_t>(), cap, d_n.as<int32_t>(), n_segs, d_sorted.as<int32_t>(),
                             d_parent.as<int32_t>(), nullptr, d_roots.as<int32_t>(), s),
          "ecc_optics_xi_tree");
    check(ecc_optics_xi_tree_status(ctx.get(), s), "ecc_optics_xi_tree");
    std::vector<int32_t> sorted(slots * 2), parent(slots);
    d_sorted.download(sorted.data(), sorted.size() * 4, s);
    d_parent.download(parent.data(), parent.size() * 4, s);
    ctx.sync();
    for (int64_t g = 0; g < n_segs; ++g)
        result[(size_t)g] = forest(sorted.data() + g * cap * 2, parent.data() + g * cap, counts[(size_t)g]);
    return result;
}

}  // namespace optics
}  // namespace ecc
