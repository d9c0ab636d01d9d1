// ref_optics: runs the REFERENCE's own OPTICS code — reachability_dist and its ordering, the core
// distance, seed-set update and expansion loop of OPT/include/optics/optics.hpp, its threshold and
// xi cluster extraction, flat_clusters_to_tree, the kd-tree of kdTree.hpp and the statistics loop
// of OPT/test/cluster_event_data.cpp — on flat binary files, so that tests can compare the oracle,
// the Python restatements, the host library and the device with the reference itself.
// TEST INFRASTRUCTURE ONLY; never a product path.
//
// This file is our code.  The reference text is not in it: oracle/ref/Makefile copies the needed
// line spans into oracle/_ref/ (git-ignored) at build time, each behind a guard on its first line,
// its last line and its brace balance, and they are included below where the reference has them.
// kdTree.hpp and tree.hpp are included from where they lie.  The FunctionalPlus and Geometry names
// they use come from the stand-ins under oracle/ref/standin/ (our code as well; their headers say
// what they leave unpinned).  The whole of optics.hpp is not compiled: it needs Boost.Geometry and
// nanoflann for back ends the reference does not select (method = KDTREE, :410).
//
//   ref_optics run pts.i32 N EPS MIN_PTS THRESHOLD ball|kdtree XI order.i32 reach.f64 meta.i32
//                  sizes.i32 xi.i32 forest.i32 stats.u64
//
// pts.i32: N points (x, y) as int32 (std::array<int, 2>, the driver's point type).  N must be one
// of the sizes compiled in below: the kd-tree takes its point count as a template argument.
// For every point both the exact eps-ball (dx^2 + dy^2 <= eps^2 in double, indices ascending) and
// kdt::make_KDTree<int, 2, N, 8>(points)->radius_search (the back end of :492-503) are computed;
// meta[0] is the number of points whose two sets differ (quirk Q22).  "ball" feeds the expansion
// loop the exact balls, "kdtree" the kd-tree's own lists, and then fails if any set differed.
// XI: "chi,min_pts,steep_area_min_diff;..." parameter sets for get_chi_clusters_flat (skipped for
// N < 2).  Outputs: order and reach of the ordered plot; meta = {differing sets, threshold
// clusters}; sizes of the threshold clusters (their members are consecutive plot positions, which
// is checked); xi.i32 and forest.i32 in the "lists" format (int32: number of lists, then per list a
// count and count records) with records (begin, end) and depth-first (level, first, second);
// stats.u64 = records of 5 words {size, bits of centroid x, y, bits of variance x, y} for the
// threshold clusters, then for every xi list's pairs in order.
#include <array>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include <fplus/fplus.hpp>
#include <geometry/geometry.hpp>

#include "tree.hpp"    // the reference's headers, found through -I
#include "kdTree.hpp"

namespace optics {

#include "opt_types.inc"  // optics.hpp:50-72   typedefs, reachability_dist, its < and ==
#include "opt_core.inc"   // optics.hpp:286-337 compute_core_dist, erase_idx_from_set, pop_from_set, update

// the two drawing names get_cluster_indices (:685-688) mentions; never reached (the path stays "")
struct bgr_image {
    void save(const std::string &) const {}
};
inline bgr_image draw_reachability_plot(const std::vector<reachability_dist> &) { return bgr_image(); }

// compute_reachability_dists (:413-565) from its expansion loop on, over neighbour lists computed
// by the caller; the trackers are initialised as :434-437 initialise them.
template <typename T, std::size_t dimension>
std::vector<reachability_dist> expand(const std::vector<std::array<T, dimension>> &points, std::size_t min_pts,
                                      const std::vector<std::vector<std::size_t>> &neighbors) {
    std::vector<bool> processed(points.size(), false);
    std::vector<std::size_t> ordered_list;
    ordered_list.reserve(points.size());
    std::vector<double> reachability(points.size(), -1.0f);
#include "opt_loop.inc"  // optics.hpp:525-564 the expansion loop and the merge into the result
}

#include "opt_threshold.inc"  // optics.hpp:674-690 get_cluster_indices by threshold
#include "opt_xi_indices.inc"  // optics.hpp:724-739 get_cluster_indices by xi pairs
#include "opt_xi.inc"          // optics.hpp:803-944 SDA, get_chi_clusters_flat
#include "opt_tree.inc"        // optics.hpp:948-995 flat_clusters_to_tree

}  // namespace optics

namespace {

using point = std::array<int, 2>;

[[noreturn]] void die(const std::string &m) {
    std::fprintf(stderr, "ref_optics: %s\n", m.c_str());
    std::exit(2);
}

template <typename T>
std::vector<T> read_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) die(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)sizeof(T)) die(std::string("bad size: ") + path);
    std::vector<T> v((std::size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) die(std::string("short read: ") + path);
    std::fclose(f);
    return v;
}

template <typename T>
void write_file(const char *path, const std::vector<T> &v) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f) die(std::string("cannot write ") + path);
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) die(std::string("short write: ") + path);
    std::fclose(f);
}

std::uint64_t bits(double v) {
    std::uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// The statistics loop of the reference's event driver over `cluster_points`, as the driver names
// them; what it prints goes nowhere, what it leaves in centroids / deviations is appended to out.
void statistics(const std::vector<std::vector<point>> &cluster_points, std::vector<std::uint64_t> &out) {
    using namespace std;
    std::ostringstream sink;
    std::streambuf *const keep = std::cout.rdbuf(sink.rdbuf());
#include "ced_stats.inc"  // cluster_event_data.cpp:472-530
    std::cout.rdbuf(keep);
    for (std::size_t j = 0; j < cluster_points.size(); ++j) {
        out.push_back(cluster_points[j].size());
        out.push_back(bits(centroids[j][0]));
        out.push_back(bits(centroids[j][1]));
        out.push_back(bits(deviations[j][0]));
        out.push_back(bits(deviations[j][1]));
    }
}

std::vector<std::vector<point>> gather(const std::vector<point> &points, const std::vector<std::vector<std::size_t>> &lists) {
    std::vector<std::vector<point>> out;
    out.reserve(lists.size());
    for (const auto &l : lists) {
        out.emplace_back();
        for (const std::size_t i : l) {
            if (i >= points.size()) die("a cluster names a point outside the set");
            out.back().push_back(points[i]);
        }
    }
    return out;
}

void dfs(const optics::Node<optics::chi_cluster_indices> &n, std::int32_t level, std::vector<std::int32_t> &out) {
    out.push_back(level);
    out.push_back((std::int32_t)n.get_data().first);
    out.push_back((std::int32_t)n.get_data().second);
    for (const auto &c : n.get_children()) dfs(c, level + 1, out);
}

struct XiParams {
    double chi;
    std::size_t min_pts;
    double steep_area_min_diff;
};

std::vector<XiParams> parse_xi(const char *s) {
    std::vector<XiParams> out;
    const char *p = s;
    while (*p) {
        char *e;
        XiParams x;
        x.chi = std::strtod(p, &e);
        if (e == p || *e != ',') die("bad xi parameters");
        p = e + 1;
        x.min_pts = (std::size_t)std::strtoull(p, &e, 10);
        if (e == p || *e != ',') die("bad xi parameters");
        p = e + 1;
        x.steep_area_min_diff = std::strtod(p, &e);
        if (e == p || (*e != ';' && *e != 0)) die("bad xi parameters");
        p = *e ? e + 1 : e;
        out.push_back(x);
    }
    return out;
}

template <std::size_t N>
int run(const std::vector<point> &points, double eps, std::size_t min_pts, double threshold, bool feed_kdtree,
        const std::vector<XiParams> &xi, char **out) {
    // neighbours: the exact ball and the reference's default back end (:492-503)
    const double r2 = eps * eps;
    std::vector<std::vector<std::size_t>> ball(N), tree_sets(N);
    for (std::size_t i = 0; i < N; ++i)
        for (std::size_t j = 0; j < N; ++j) {
            const double dx = (double)points[j][0] - (double)points[i][0], dy = (double)points[j][1] - (double)points[i][1];
            if (dx * dx + dy * dy <= r2) ball[i].push_back(j);
        }
    const auto kd_tree = kdt::make_KDTree<int, 2, N, 8>(points);
    std::int32_t differing = 0;
    for (std::size_t i = 0; i < N; ++i) {
        tree_sets[i] = kd_tree->radius_search(points[i], eps);
        std::vector<std::size_t> sorted(tree_sets[i]);
        std::sort(sorted.begin(), sorted.end());
        differing += sorted != ball[i];
    }
    if (feed_kdtree && differing) die(std::to_string(differing) + " kd-tree sets differ from the exact ball in a case that feeds them");

    const std::vector<optics::reachability_dist> reach_dists = optics::expand<int, 2>(points, min_pts, feed_kdtree ? tree_sets : ball);
    if (reach_dists.size() != N) die("the ordering lost points");
    std::vector<std::int32_t> order;
    std::vector<double> reach;
    for (const auto &r : reach_dists) {
        order.push_back((std::int32_t)r.point_index);
        reach.push_back(r.reach_dist);
    }

    // threshold clusters: consecutive runs of the plot
    const auto clusters = optics::get_cluster_indices(reach_dists, threshold);
    std::vector<std::int32_t> sizes;
    std::size_t pos = 0;
    for (const auto &c : clusters) {
        sizes.push_back((std::int32_t)c.size());
        for (const std::size_t i : c)
            if (pos >= N || i != reach_dists[pos++].point_index) die("a threshold cluster is no run of the plot");
    }
    if (pos != N) die("the threshold clusters do not cover the plot");
    std::vector<std::uint64_t> stats;
    statistics(gather(points, clusters), stats);

    std::vector<std::int32_t> xi_words{(std::int32_t)xi.size()}, forest_words{(std::int32_t)xi.size()};
    for (const auto &x : xi) {
        std::vector<optics::chi_cluster_indices> flat;
        if (N >= 2) flat = optics::get_chi_clusters_flat(reach_dists, x.chi, x.min_pts, x.steep_area_min_diff);
        xi_words.push_back((std::int32_t)flat.size());
        for (const auto &c : flat) {
            if (c.first > c.second || c.second >= N) die("a xi pair lies outside the plot");
            xi_words.push_back((std::int32_t)c.first);
            xi_words.push_back((std::int32_t)c.second);
        }
        std::vector<std::int32_t> nodes;
        for (const auto &t : optics::flat_clusters_to_tree(flat)) dfs(t.get_root(), 0, nodes);
        forest_words.push_back((std::int32_t)(nodes.size() / 3));
        forest_words.insert(forest_words.end(), nodes.begin(), nodes.end());
        statistics(gather(points, optics::get_cluster_indices(reach_dists, flat)), stats);
    }

    write_file(out[0], order);
    write_file(out[1], reach);
    write_file(out[2], std::vector<std::int32_t>{differing, (std::int32_t)clusters.size()});
    write_file(out[3], sizes);
    write_file(out[4], xi_words);
    write_file(out[5], forest_words);
    write_file(out[6], stats);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 16 || std::string(argv[1]) != "run") die("usage: see the head of oracle/ref/ref_optics.cpp");
    const std::vector<std::int32_t> words = read_file<std::int32_t>(argv[2]);
    const std::size_t n = (std::size_t)std::strtoull(argv[3], nullptr, 10);
    if (words.size() != 2 * n) die("pts.i32 does not hold N points");
    std::vector<point> points(n);
    for (std::size_t i = 0; i < n; ++i) points[i] = {words[2 * i], words[2 * i + 1]};
    const double eps = std::strtod(argv[4], nullptr);
    const std::size_t min_pts = (std::size_t)std::strtoull(argv[5], nullptr, 10);
    const double threshold = std::strtod(argv[6], nullptr);
    const std::string feed = argv[7];
    if (feed != "ball" && feed != "kdtree") die("feed is ball or kdtree");
    if (!(eps > 0.0) || min_pts < 1) die("eps must be positive, min_pts at least 1");
    const std::vector<XiParams> xi = parse_xi(argv[8]);
    char **out = argv + 9;
    switch (n) {  // the case sizes of tests/ref_optics_cases.py
    case 9: return run<9>(points, eps, min_pts, threshold, feed == "kdtree", xi, out);
    case 320: return run<320>(points, eps, min_pts, threshold, feed == "kdtree", xi, out);
    case 600: return run<600>(points, eps, min_pts, threshold, feed == "kdtree", xi, out);
    case 1024: return run<1024>(points, eps, min_pts, threshold, feed == "kdtree", xi, out);
    case 8192: return run<8192>(points, eps, min_pts, threshold, feed == "kdtree", xi, out);
    default: die("N is not one of the compiled sizes 9, 320, 600, 1024, 8192");
    }
}
