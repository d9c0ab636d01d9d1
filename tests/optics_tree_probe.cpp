// Stand-alone program of tests/test_optics_tree_host.py: the forests of ecc::optics::get_chi_clusters
// and flat_clusters_to_tree (include/ecc.hpp) on the host, printed for the test to compare.
//   probe plot <chi> <min_pts> <steep_area_min_diff> r0 r1 ...   get_chi_clusters of one plot
//   probe flat a0 b0 a1 b1 ...                                      flat_clusters_to_tree of one list
// Per tree: "tree <tree_depth> <tree_size> <nested form>", then one "first second" line per
// flatten_dfs entry.  Exits 2 when the tree interface disagrees with itself.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ecc.hpp"

using namespace ecc::optics;
using TreeNode = Node<chi_cluster_indices>;

static std::string nested(const TreeNode &n) {
    std::string s = "[" + std::to_string(n.get_data().first) + ", " + std::to_string(n.get_data().second) + ", [";
    for (size_t i = 0; i < n.get_children().size(); ++i) s += (i ? ", " : "") + nested(n.get_children()[i]);
    return s + "]]";
}

// the same tree again through the mutating interface: add_child for the first child, add_children for the rest
static TreeNode rebuilt(const TreeNode &n) {
    TreeNode out(n.get_data());
    std::vector<TreeNode> rest;
    for (size_t i = 0; i < n.get_children().size(); ++i) {
        if (i == 0) out.add_child(rebuilt(n.get_children()[i]));
        else rest.push_back(rebuilt(n.get_children()[i]));
    }
    out.add_children(rest);
    return out;
}

int main(int argc, char **argv) {
    if (argc < 2) return 1;
    std::vector<cluster_tree> trees;
    try {
        if (std::string(argv[1]) == "plot" && argc >= 5) {
            std::vector<reachability_dist> reach;
            for (int i = 5; i < argc; ++i) reach.emplace_back((size_t)(i - 4), std::atof(argv[i]));
            trees = get_chi_clusters(reach, std::atof(argv[2]), (size_t)std::atoll(argv[3]), std::atof(argv[4]));
        } else if (std::string(argv[1]) == "flat" && argc % 2 == 0) {
            std::vector<chi_cluster_indices> flat;
            for (int i = 2; i + 1 < argc; i += 2) flat.emplace_back((size_t)std::atoll(argv[i]), (size_t)std::atoll(argv[i + 1]));
            trees = flat_clusters_to_tree(flat);
        } else {
            return 1;
        }
    } catch (const ecc::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    for (const auto &t : trees) {
        const auto flat = flatten_dfs(t);
        cluster_tree copy(rebuilt(t.get_root()));
        if (flat.size() != tree_size(t.get_root()) || copy.flatten() != flat || nested(copy.get_root()) != nested(t.get_root()) ||
            tree_depth(copy.get_root()) != tree_depth(t.get_root()))
            return 2;
        std::printf("tree %zu %zu %s\n", tree_depth(t.get_root()), tree_size(t.get_root()), nested(t.get_root()).c_str());
        for (const auto &c : flat) std::printf("%zu %zu\n", c.first, c.second);
    }
    if (cluster_tree().get_root().get_data() != chi_cluster_indices(0, 0)) return 2;  // Tree(): root {0, 0}
    return 0;
}
