// Host program mirroring OPT/test/cluster_event_data.cpp (clustering_test_1 :429-545): read the
// (x,y) of an event CSV, optics::compute_reachability_dists(points, min_pts = 2, eps = 10)
// (:449), get_cluster_indices(reach, 10) (:454), and print each cluster's size, centroid and
// variance (:470-530).  eps-neighbourhoods/core distances on the GPU, ordering on the host; with
// --device-order (at most 8192 points) the ordering runs on the GPU too and prints the same.
// --chi X [--steep-min-diff Y]: additionally get_chi_clusters_flat(reach, X, min_pts, Y)
// (optics.hpp:803-944), printed as "xi_clusters K" and one "begin end" line per pair after the
// existing output; on the host by default, with --device-order from the reach left on the device.
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

// The points as one segment of packed u16 xy (translated to the bounding box's corner: distances
// do not change) through ecc_optics_grid; with xi, the reach stays on the device for ecc_optics_xi.
using XiPairs = std::vector<std::pair<std::size_t, std::size_t>>;
static std::vector<ecc::optics::reachability_dist> device_order(const std::vector<std::array<int, 2>> &pts,
                                                                size_t min_pts, double eps, XiPairs *xi, double chi,
                                                                double steep_min_diff) {
    if (pts.empty()) return {};
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
    std::vector<uint32_t> xy(pts.size());
    for (size_t i = 0; i < pts.size(); ++i) xy[i] = ecc::pack_xy(pts[i][0] - xmn, pts[i][1] - ymn);
    ecc::Context &ctx = ecc::Context::default_context();
    ecc::DeviceBuffer d_xy;
    d_xy.upload(xy.data(), xy.size() * 4, ctx.stream());
    if (!xi)
        return ecc::optics::compute_reachability_dists_windows(ctx, d_xy.as<uint32_t>(), 1, (int64_t)pts.size(),
                                                               nullptr, min_pts, eps)[0];
    const int64_t n = (int64_t)pts.size();
    ecc::DeviceBuffer d_order((size_t)n * 4), d_reach((size_t)n * 8);
    const int rc = min_pts > 64 ? ECC_ERR_INVALID
                                : ecc_optics_grid(ctx.get(), d_xy.as<uint32_t>(), 1, n, nullptr, eps, (int32_t)min_pts, 0.0,
                                                  d_order.as<int32_t>(), d_reach.as<double>(), nullptr, nullptr,
                                                  ctx.stream());
    if (rc != ECC_OK) throw ecc::Error(rc, "ecc_optics_grid");
    *xi = ecc::optics::get_chi_clusters_flat_windows(ctx, d_reach.as<double>(), 1, n, nullptr, chi, min_pts,
                                                     steep_min_diff)[0];
    std::vector<int32_t> order((size_t)n);
    std::vector<double> reach((size_t)n);
    d_order.download(order.data(), (size_t)n * 4, ctx.stream());
    d_reach.download(reach.data(), (size_t)n * 8, ctx.stream());
    ctx.sync();
    std::vector<ecc::optics::reachability_dist> out;
    for (int64_t i = 0; i < n; ++i) out.emplace_back((std::size_t)order[(size_t)i], reach[(size_t)i]);
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
        const double chi = opt_double(argc, argv, "--chi", 0.0);
        const double steep_min_diff = opt_double(argc, argv, "--steep-min-diff", 0.0);
        XiPairs xi;
        auto reach = on_device ? device_order(pts, min_pts, eps, with_xi ? &xi : nullptr, chi, steep_min_diff)
                               : ecc::optics::compute_reachability_dists(pts, min_pts, eps);
        if (with_xi && !(on_device && !pts.empty()))
            xi = ecc::optics::get_chi_clusters_flat(reach, chi, min_pts, steep_min_diff);
        auto clusters = ecc::optics::get_cluster_indices(reach, thr);
        std::printf("points %zu clusters %zu\n", pts.size(), clusters.size());
        for (size_t c = 0; c < clusters.size(); ++c) {
            double sx = 0, sy = 0;
            for (size_t i : clusters[c]) { sx += pts[i][0]; sy += pts[i][1]; }
            const double m = (double)clusters[c].size(), cx = sx / m, cy = sy / m;
            double vx = 0, vy = 0;
            for (size_t i : clusters[c]) { vx += (pts[i][0] - cx) * (pts[i][0] - cx); vy += (pts[i][1] - cy) * (pts[i][1] - cy); }
            std::printf("cluster %zu size %zu centroid (%.4f, %.4f) variance (%.4f, %.4f)\n", c, clusters[c].size(), cx, cy, vx / m, vy / m);
        }
        std::printf("order");
        for (const auto &r : reach) std::printf(" %zu:%.17g", r.point_index, r.reach_dist);
        std::printf("\n");
        if (with_xi) {
            std::printf("xi_clusters %zu\n", xi.size());
            for (const auto &c : xi) std::printf("%zu %zu\n", c.first, c.second);
        }
    } catch (const ecc::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
