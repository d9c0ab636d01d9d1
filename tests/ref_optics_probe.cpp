// Stand-alone program of tests/test_ref_optics.py: include/ecc.hpp's host OPTICS extraction —
// ecc::optics::get_cluster_indices, get_chi_clusters_flat, get_chi_clusters and
// flat_clusters_to_tree — on a recorded ordered plot, written in the formats of
// oracle/ref/ref_optics.cpp for the test to compare with the reference's answers.
//   probe order.i32 reach.f64 THRESHOLD XI sizes.i32 xi.i32 forest.i32 forest_flat.i32
// XI: "chi,min_pts,steep_area_min_diff;...".  forest.i32 comes from get_chi_clusters, forest_flat.i32
// from flat_clusters_to_tree(get_chi_clusters_flat(...)).  Exits 2 when a threshold cluster is no run
// of the plot.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ecc.hpp"

using namespace ecc::optics;

template <typename T>
static std::vector<T> read_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) std::exit(1);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(1);
    std::fclose(f);
    return v;
}

static void write_file(const char *path, const std::vector<int32_t> &v) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f || (!v.empty() && std::fwrite(v.data(), sizeof(int32_t), v.size(), f) != v.size())) std::exit(1);
    std::fclose(f);
}

static void dfs(const Node<chi_cluster_indices> &n, int32_t level, std::vector<int32_t> &out) {
    out.push_back(level);
    out.push_back((int32_t)n.get_data().first);
    out.push_back((int32_t)n.get_data().second);
    for (const auto &c : n.get_children()) dfs(c, level + 1, out);
}

static void append_forest(const std::vector<cluster_tree> &trees, std::vector<int32_t> &words) {
    std::vector<int32_t> nodes;
    for (const auto &t : trees) dfs(t.get_root(), 0, nodes);
    words.push_back((int32_t)(nodes.size() / 3));
    words.insert(words.end(), nodes.begin(), nodes.end());
}

int main(int argc, char **argv) {
    if (argc != 9) return 1;
    const auto order = read_file<int32_t>(argv[1]);
    const auto reach = read_file<double>(argv[2]);
    if (order.size() != reach.size()) return 1;
    std::vector<reachability_dist> plot;
    for (size_t i = 0; i < order.size(); ++i) plot.emplace_back((size_t)order[i], reach[i]);
    try {
        std::vector<int32_t> sizes;
        size_t pos = 0;
        for (const auto &c : get_cluster_indices(plot, std::atof(argv[3]))) {
            sizes.push_back((int32_t)c.size());
            for (const size_t i : c)
                if (pos >= plot.size() || i != plot[pos++].point_index) return 2;
        }
        if (pos != plot.size()) return 2;
        write_file(argv[5], sizes);

        std::vector<int32_t> xi{0}, forest{0}, forest_flat{0};
        const char *p = argv[4];
        while (*p) {
            char *e;
            const double chi = std::strtod(p, &e);
            const size_t min_pts = (size_t)std::strtoull(e + 1, &e, 10);
            const double samd = std::strtod(e + 1, &e);
            p = *e ? e + 1 : e;
            const auto flat = get_chi_clusters_flat(plot, chi, min_pts, samd);
            xi.push_back((int32_t)flat.size());
            for (const auto &c : flat) {
                xi.push_back((int32_t)c.first);
                xi.push_back((int32_t)c.second);
            }
            append_forest(get_chi_clusters(plot, chi, min_pts, samd), forest);
            append_forest(flat_clusters_to_tree(flat), forest_flat);
            ++xi[0], ++forest[0], ++forest_flat[0];
        }
        write_file(argv[6], xi);
        write_file(argv[7], forest);
        write_file(argv[8], forest_flat);
    } catch (const ecc::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
