// Host program mirroring the DBSCAN part of PCC/pcl_cluster.cpp (:97-148): DBSCAN with eps 20,
// core minPts 20, cluster size 100..25000 over the event points, writing "x,y,z,cluster%8" CSV
// lines (:140).  The cloud is (x, y, 0), or with --t-scale S the (x, y, t) event cloud with
// z = float(t * S) (north_star's clustering over event point clouds).  PCL's PCD input, VoxelGrid
// and RANSAC stages are out of scope.  --precomp runs DBSCANPrecompCluster (the driver's "test 2",
// :106-108); --cloud-first calls setInputCloud before the setters, which for the precomputed
// variant freezes the adjacency at the tolerance set so far (DBSCAN_precomp.h:10-16, :28).
// --windows: the event stream -> ecc_downsample_hash -> ecc_dbscan_grid -> ecc_dbscan_lists ->
// ecc_cluster_stats_lists, all on the device (ecc::dbscan_statistics_windows): per downsample
// window one line "window W points U clusters K", then one line "j,size,cx,cy,devx,devy" per
// cluster in output order (%.17g, as ecc_optics_events --stats prints its records).
#include "app_common.hpp"

static int run_windows(int argc, char **argv, const Events &ev) {
    ecc::Context ctx(0);
    ecc::HashDownsampler ds(ctx);
    const int64_t n = (int64_t)ev.xy.size(), window = ds.config().window, nw = (n + window - 1) / window;
    if (n == 0) return 0;
    ecc::DeviceBuffer d_xy, d_rep((size_t)(nw * window) * 4), d_u((size_t)nw * 4);
    d_xy.upload(ev.xy.data(), (size_t)n * 4, ctx.stream());
    ds.run(d_xy.as<uint32_t>(), n, d_rep.as<uint32_t>(), nullptr, d_u.as<int32_t>(), nullptr);
    const auto stats = ecc::dbscan_statistics_windows(
        ctx, d_rep.as<uint32_t>(), nw, window, d_u.as<int32_t>(), opt_double(argc, argv, "--eps", 20.0),
        opt_int(argc, argv, "--min-pts", 20), opt_int(argc, argv, "--min-size", 100),
        opt_int(argc, argv, "--max-size", 25000));
    std::vector<int32_t> uniq((size_t)nw);
    d_u.download(uniq.data(), uniq.size() * 4, ctx.stream());
    ctx.sync();
    for (int64_t w = 0; w < nw; ++w) {
        std::printf("window %lld points %d clusters %zu\n", (long long)w, uniq[(size_t)w], stats[(size_t)w].size());
        for (size_t j = 0; j < stats[(size_t)w].size(); ++j) {
            const auto &c = stats[(size_t)w][j];
            std::printf("%zu,%zu,%.17g,%.17g,%.17g,%.17g\n", j, c.size, c.centroid[0], c.centroid[1], c.variance[0],
                        c.variance[1]);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    try {
        Events ev = load_events(argc, argv, 1280, 720);
        if (has_flag(argc, argv, "--windows")) return run_windows(argc, argv, ev);
        const double ts = opt_double(argc, argv, "--t-scale", 0.0);
        std::vector<ecc::PointXYZ> cloud(ev.xy.size());
        for (size_t i = 0; i < ev.xy.size(); ++i)
            cloud[i] = {(float)(ev.xy[i] & 0xffff), (float)(ev.xy[i] >> 16), ts != 0.0 ? (float)(ev.t[i] * ts) : 0.f};
        ecc::Context ctx(0);
        const bool precomp = has_flag(argc, argv, "--precomp"), cloud_first = has_flag(argc, argv, "--cloud-first");
        ecc::DBSCANSimpleCluster simple(ctx);
        ecc::DBSCANPrecompCluster pre(ctx);
        ecc::DBSCANSimpleCluster &ec = precomp ? pre : simple;
        if (cloud_first) ec.setInputCloud(cloud);
        ec.setCorePointMinPts(opt_int(argc, argv, "--min-pts", 20));
        ec.setClusterTolerance(opt_double(argc, argv, "--eps", 20.0));
        ec.setMinClusterSize(opt_int(argc, argv, "--min-size", 100));
        ec.setMaxClusterSize(opt_int(argc, argv, "--max-size", 25000));
        if (!cloud_first) ec.setInputCloud(cloud);
        std::vector<ecc::PointIndices> clusters;
        ec.extract(clusters);
        std::printf("cluster size : %zu\n", clusters.size());
        for (size_t j = 0; j < clusters.size(); ++j)
            for (int idx : clusters[j].indices)
                std::printf("%g,%g,%g,%zu\n", cloud[idx].x, cloud[idx].y, cloud[idx].z, j % 8);
    } catch (const ecc::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
