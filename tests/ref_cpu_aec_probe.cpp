// Drives the host library's ecc::AEClustering (host/aeclustering.cpp) exactly as oracle/ref's
// `ref_cpu aec` drives the reference's class: FEED (double t, x, y per update), WIN_COUNTS (int32
// updates per window), OUT (double): per window the number of clusters, then per cluster in deque
// order id, n, getClusterCentroid(), getMu().  Built and run by tests/test_ref_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ecc.hpp"

template <typename T>
static std::vector<T> read_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<T> v((std::size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const auto feed = read_file<double>(argv[1]);
    const auto wins = read_file<int32_t>(argv[2]);
    ecc::AEClustering ae;
    std::vector<double> o;
    std::size_t r = 0;
    for (int32_t n : wins) {
        for (int32_t k = 0; k < n; ++k, ++r) {
            if (3 * r + 2 >= feed.size()) return 2;
            ae.update(std::deque<double>{feed[3 * r], feed[3 * r + 1], feed[3 * r + 2], 0.0});
        }
        o.push_back((double)ae.clusters.size());
        for (const auto &c : ae.clusters) {
            const ecc::Vec2d cen = c.getClusterCentroid(), mu = c.getMu();
            o.push_back(c.getClusterId()); o.push_back(c.getN());
            o.push_back(cen[0]); o.push_back(cen[1]); o.push_back(mu[0]); o.push_back(mu[1]);
        }
    }
    std::FILE *f = std::fopen(argv[3], "wb");
    if (!f || (!o.empty() && std::fwrite(o.data(), sizeof(double), o.size(), f) != o.size())) return 2;
    std::fclose(f);
    return 0;
}
