// Host program mirroring OPT/test/cluster_event_data.cpp (clustering_test_1 :429-545): read the
// (x,y) of an event CSV, optics::compute_reachability_dists(points, min_pts = 2, eps = 10)
// (:449), get_cluster_indices(reach, 10) (:454), and print each cluster's size, centroid and
// variance (:470-530).  eps-neighbourhoods/core distances on the GPU, ordering on the host; with
// --device-order (at most 8192 points) the ordering runs on the GPU too and prints the same.
// --chi X [--steep-min-diff Y]: additionally get_chi_clusters_flat(reach, X, min_pts, Y)
// (optics.hpp:803-944), printed as "xi_clusters K" and one "begin end" line per pair after the
// existing output; on the host by default, with --device-order from the reach left on the device.
// --chi-tree (with --chi): after the pairs, get_chi_clusters' forest (optics.hpp:948-995, :1018-1021)
// as "xi_tree K roots R" and one "level begin end" line per node, depth first; on the host by
// default, with --device-order from ecc_optics_xi_tree on the pairs left on the device.
// --stats: after all that, "stats_clusters K" and one "begin size cx cy vx vy" line (%.17g) per
// threshold cluster and, with --chi, "stats_xi K" and one such line per pair and, with --chi-tree,
// "stats_xi_tree K" and one such line per pair in the tree's placed order (children before
// parents); with --device-order these and the "cluster ..." lines come from
// ecc_cluster_stats_runs / _pairs on the device.
#include <algorithm>
#include <cmath>

#include "app_common.hpp"

// --points <file>: "x,y" lines with signed integers (the KAT point sets of OPT/test/test_main.cpp)
static std::vector<std::array<int, 2>> read_points(const char *path) {
    std::vector<std::array<int, 2>> pts;
    FILE *f = std::fopen(path, "r");
    if (!f) { std::perror(path); std::exit(1); }
    int x, y;
    while (std::fscanf(f, "%d,%d", &x, &y) == 2) pts.push_back({x, y});
    std::fclose(f);
    return pts;
}

// The points as one segment of packed u16 xy through ecc_optics_grid (ordering and threshold cluster
// ids), ecc_cluster_stats_runs on the order / cluster arrays it leaves on the device and, with xi,
// ecc_optics_xi on the reach and ecc_cluster_stats_pairs on its pairs.  Points outside
// [0, 65535]^2 are translated to the bounding box's corner: distances do not change, but the bits
// of the statistics do, so those are then left to the host loop (stats_exact = false).
using XiPairs = std::vector<ecc::optics::chi_cluster_indices>;
using Stats = std::vector<ecc::optics::cluster_stat<2>>;
struct DeviceOrder {
    std::vector<ecc::optics::reachability_dist> reach;
    bool stats_exact = false;
    Stats clusters, xi_stats, xi_tree_stats;
    XiPairs xi;
    std::vector<ecc::optics::cluster_tree> xi_trees;
};

static void check(int rc, const char *what) {
    if (rc != ECC_OK) throw ecc::Error(rc, what);
}

static DeviceOrder device_order(const std::vector<std::array<int, 2>> &pts, size_t min_pts, double eps, double thr,
                                bool with_xi, double chi, double steep_min_diff, bool with_tree) {
    DeviceOrder out;
    if (pts.empty()) return out;
    if (pts.size() > 8192) {
        std::fprintf(stderr, "--device-order: %zu points, one device segment holds at most 8192\n", pts.size());
        std::exit(1);
    }
    if (eps <= 0.0) eps = ecc::optics::epsilon_estimation(pts, min_pts);
    int xmn = pts[0][0], ymn = pts[0][1], xmx = xmn, ymx = ymn;
    for (const auto &p : pts) {
        xmn = std::min(xmn, p[0]); xmx = std::max(xmx, p[0]);
        ymn = std::min(ymn, p[1]); ymx = std::max(ymx, p[1]);
    }
    if ((int64_t)xmx - xmn > 65535 || (int64_t)ymx - ymn > 65535) {
        std::fprintf(stderr, "--device-order: the points span more than 65535 on an axis\n");
        std::exit(1);
    }
    out.stats_exact = xmn >= 0 && ymn >= 0 && xmx <= 65535 && ymx <= 65535;
    if (out.stats_exact) xmn = ymn = 0;
    std::vector<uint32_t> xy(pts.size());
    for (size_t i = 0; i < pts.size(); ++i) xy[i] = ecc::pack_xy(pts[i][0] - xmn, pts[i][1] - ymn);
    ecc::Context &ctx = ecc::Context::default_context();
    ecc::DeviceBuffer d_xy;
    d_xy.upload(xy.data(), xy.size() * 4, ctx.stream());
    const int64_t n = (int64_t)pts.size();
    ecc::DeviceBuffer d_order((size_t)n * 4), d_reach((size_t)n * 8), d_cluster((size_t)n * 4), d_ncl(4);
    check(min_pts > 64 ? ECC_ERR_INVALID
                       : ecc_optics_grid(ctx.get(), d_xy.as<uint32_t>(), 1, n, nullptr, eps, (int32_t)min_pts, thr,
                                         d_order.as<int32_t>(), d_reach.as<double>(), d_cluster.as<int32_t>(),
                                         d_ncl.as<int32_t>(), ctx.stream()),
          "ecc_optics_grid");
    out.clusters = ecc::optics::cluster_statistics_windows(ctx, d_xy.as<uint32_t>(), d_order.as<int32_t>(),
                                                           d_cluster.as<int32_t>(), 1, n, nullptr)[0];
    if (with_xi) {
        if (min_pts > (size_t)INT32_MAX) check(ECC_ERR_INVALID, "ecc_optics_xi");
        ecc::DeviceBuffer d_pairs, d_np(4);
        int32_t np = 0;
        // a second pass with the count as capacity when the first guess was too small
        for (int64_t cap = 64;;) {
            d_pairs.reserve((size_t)std::max<int64_t>(cap, 1) * 8);
            check(ecc_optics_xi(ctx.get(), d_reach.as<double>(), 1, n, nullptr, chi, (int32_t)min_pts, steep_min_diff,
                                d_pairs.as<int32_t>(), cap, d_np.as<int32_t>(), ctx.stream()),
                  "ecc_optics_xi");
            d_np.download(&np, 4, ctx.stream());
            const int rc = ecc_optics_xi_status(ctx.get(), ctx.stream());
            if (rc == ECC_ERR_CAPACITY && np > cap) {
                cap = np;
                continue;
            }
            check(rc, "ecc_optics_xi");
            std::vector<int32_t> pairs((size_t)np * 2);
            d_pairs.download(pairs.data(), pairs.size() * 4, ctx.stream());
            ctx.sync();
            for (int32_t k = 0; k < np; ++k) out.xi.emplace_back((size_t)pairs[(size_t)k * 2], (size_t)pairs[(size_t)k * 2 + 1]);
            out.xi_stats = ecc::optics::cluster_statistics_windows(ctx, d_xy.as<uint32_t>(), d_order.as<int32_t>(),
                                                                   d_pairs.as<int32_t>(), cap, d_np.as<int32_t>(), 1, n,
                                                                   nullptr)[0];
            if (with_tree) {
                out.xi_trees = ecc::optics::get_chi_clusters_windows(ctx, d_reach.as<double>(), 1, n, nullptr, chi,
                                                                     min_pts, steep_min_diff)[0];
                // the statistics in the placed order: `sorted` as ecc_cluster_stats_pairs' pairs
                const size_t slots = (size_t)std::max<int64_t>(cap, 1);
                ecc::DeviceBuffer d_sorted(slots * 8), d_parent(slots * 4), d_roots(4);
                check(ecc_optics_xi_tree(ctx.get(), d_pairs.as<int32_t>(), cap, d_np.as<int32_t>(), 1,
                                         d_sorted.as<int32_t>(), d_parent.as<int32_t>(), nullptr,
                                         d_roots.as<int32_t>(), ctx.stream()),
                      "ecc_optics_xi_tree");
                check(ecc_optics_xi_tree_status(ctx.get(), ctx.stream()), "ecc_optics_xi_tree");
                out.xi_tree_stats = ecc::optics::cluster_statistics_windows(ctx, d_xy.as<uint32_t>(), d_order.as<int32_t>(),
                                                                            d_sorted.as<int32_t>(), cap, d_np.as<int32_t>(),
                                                                            1, n, nullptr)[0];
            }
            break;
        }
    }
    std::vector<int32_t> order((size_t)n);
    std::vector<double> reach((size_t)n);
    d_order.download(order.data(), (size_t)n * 4, ctx.stream());
    d_reach.download(reach.data(), (size_t)n * 8, ctx.stream());
    ctx.sync();
    for (int64_t i = 0; i < n; ++i) out.reach.emplace_back((std::size_t)order[(size_t)i], reach[(size_t)i]);
    return out;
}

static void print_stats(const char *title, const Stats &stats) {
    std::printf("%s %zu\n", title, stats.size());
    for (const auto &c : stats)
        std::printf("%zu %zu %.17g %.17g %.17g %.17g\n", c.begin, c.size, c.centroid[0], c.centroid[1], c.variance[0],
                    c.variance[1]);
}

static void print_node(const ecc::optics::Node<ecc::optics::chi_cluster_indices> &node, size_t level) {
    std::printf("%zu %zu %zu\n", level, node.get_data().first, node.get_data().second);
    for (const auto &c : node.get_children()) print_node(c, level + 1);
}

// the placed ("sorted") list of flat_clusters_to_tree (ecc_optics_xi_tree_host)
static XiPairs placed_order(const XiPairs &xi) {
    std::vector<int32_t> pairs(xi.size() * 2), sorted(xi.size() * 2), parent(xi.size());
    for (size_t k = 0; k < xi.size(); ++k) pairs[2 * k] = (int32_t)xi[k].first, pairs[2 * k + 1] = (int32_t)xi[k].second;
    int64_t n_roots = 0;
    check(ecc_optics_xi_tree_host(pairs.data(), (int64_t)xi.size(), sorted.data(), parent.data(), nullptr, &n_roots),
          "ecc_optics_xi_tree_host");
    XiPairs out;
    for (size_t k = 0; k < xi.size(); ++k) out.emplace_back((size_t)sorted[2 * k], (size_t)sorted[2 * k + 1]);
    return out;
}

int main(int argc, char **argv) {
    try {
        std::vector<std::array<int, 2>> pts;
        if (argc >= 3 && !std::strcmp(argv[1], "--points")) {
            pts = read_points(argv[2]);
        } else {
            Events ev = load_events(argc, argv, 1280, 720);
            pts.resize(ev.xy.size());
            for (size_t i = 0; i < ev.xy.size(); ++i) pts[i] = {(int)(ev.xy[i] & 0xffff), (int)(ev.xy[i] >> 16)};
        }
        const size_t min_pts = (size_t)opt_int(argc, argv, "--min-pts", 2);
        const double eps = opt_int(argc, argv, "--eps", 10), thr = opt_int(argc, argv, "--threshold", 10);
        // --eps 0 or negative: estimated (optics.hpp:428-430)
        // --device-order: the whole ordering on the GPU, the points as one ecc_optics_grid segment
        const bool with_xi = has_flag(argc, argv, "--chi"), on_device = has_flag(argc, argv, "--device-order");
        const bool with_stats = has_flag(argc, argv, "--stats");
        const double chi = opt_double(argc, argv, "--chi", 0.0);
        const double steep_min_diff = opt_double(argc, argv, "--steep-min-diff", 0.0);
        const bool with_tree = has_flag(argc, argv, "--chi-tree");
        if (with_tree && !with_xi) {
            std::fprintf(stderr, "--chi-tree needs --chi X\n");
            return 1;
        }
        DeviceOrder dev;
        if (on_device) dev = device_order(pts, min_pts, eps, thr, with_xi, chi, steep_min_diff, with_tree);
        const bool from_device = on_device && !pts.empty();
        const auto reach = from_device ? dev.reach : ecc::optics::compute_reachability_dists(pts, min_pts, eps);
        const XiPairs xi = !with_xi      ? XiPairs{}
                           : from_device ? dev.xi
                                         : ecc::optics::get_chi_clusters_flat(reach, chi, min_pts, steep_min_diff);
        // get_cluster_points (:470) and the statistics loop (:472-527)
        const Stats clusters = from_device && dev.stats_exact ? dev.clusters
                                                              : ecc::optics::cluster_statistics(pts, reach, thr);
        std::printf("points %zu clusters %zu\n", pts.size(), clusters.size());
        for (size_t c = 0; c < clusters.size(); ++c)
            std::printf("cluster %zu size %zu centroid (%.4f, %.4f) variance (%.4f, %.4f)\n", c, clusters[c].size,
                        clusters[c].centroid[0], clusters[c].centroid[1], clusters[c].variance[0], clusters[c].variance[1]);
        std::printf("order");
        for (const auto &r : reach) std::printf(" %zu:%.17g", r.point_index, r.reach_dist);
        std::printf("\n");
        if (with_xi) {
            std::printf("xi_clusters %zu\n", xi.size());
            for (const auto &c : xi) std::printf("%zu %zu\n", c.first, c.second);
        }
        if (with_tree) {
            const auto trees = from_device ? dev.xi_trees
                                           : ecc::optics::get_chi_clusters(reach, chi, min_pts, steep_min_diff);
            std::printf("xi_tree %zu roots %zu\n", xi.size(), trees.size());
            for (const auto &t : trees) print_node(t.get_root(), 0);
        }
        if (with_stats) {
            print_stats("stats_clusters", clusters);
            if (with_xi)
                print_stats("stats_xi", from_device && dev.stats_exact ? dev.xi_stats
                                                                       : ecc::optics::cluster_statistics(pts, reach, xi));
            if (with_tree)
                print_stats("stats_xi_tree", from_device && dev.stats_exact
                                                 ? dev.xi_tree_stats
                                                 : ecc::optics::cluster_statistics(pts, reach, placed_order(xi)));
        }
    } catch (const ecc::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
