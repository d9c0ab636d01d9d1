// Host program mirroring KM/assign_to_centers2.c (main :105-568): data[i] = i % 100 for 4096
// floats (2048 points), 8 centroids {1,1,10,10,...,80,80} (:131), threshold 50; the k-means
// loop runs on the GPU in "fixed" mode (correct Lloyd update, Appendix A Q7-Q9) and prints the
// updated centroids with their point counts like the reference (:539-543).
//
// --windows <events.raw|events.csv | --synthetic N> [--k K] [--iters I]: the reference's downsample
// -> cluster chain per slice (DSA/…opencl_store.cpp:389-445, TWE/…:396-448) on a 346x260 sensor:
// hash-map downsample, k-means per 8192-event window in one launch (K centres, default 8, started
// on a regular grid over the frame; at most I updates, default 20; threshold 50, tol 1e-3), then
// every centre's displacement against the previous window.  One CSV line per window and centre:
// window,centre,x,y,n,has_prev,dx,dy (floats as %.9g).
#include <cmath>

#include "app_common.hpp"

static int run_windows(int argc, char **argv) {
    const int W = 346, H = 260;
    const int k = opt_int(argc, argv, "--k", 8), iters = opt_int(argc, argv, "--iters", 20);
    Events ev = load_events(argc - 1, argv + 1, W, H);  // the input follows --windows
    ecc::Context ctx(0);
    ecc::HashDownsampler ds(ctx);
    const int64_t n = (int64_t)ev.xy.size(), window = ds.config().window, nw = (n + window - 1) / window;
    std::vector<uint32_t> rep((size_t)(nw * window));
    std::vector<int32_t> uniq((size_t)nw);
    if (n > 0) {
        ecc::DeviceBuffer d_xy, d_rep(rep.size() * 4), d_u(uniq.size() * 4);
        d_xy.upload(ev.xy.data(), (size_t)n * 4, ctx.stream());
        ds.run(d_xy.as<uint32_t>(), n, d_rep.as<uint32_t>(), nullptr, d_u.as<int32_t>(), nullptr);
        d_rep.download(rep.data(), rep.size() * 4, ctx.stream());
        d_u.download(uniq.data(), uniq.size() * 4, ctx.stream());
        ctx.sync();
    }
    ecc::KMeans km(ctx, k, iters, 50.f, 1e-3f);
    const int g = (int)std::ceil(std::sqrt((double)(k > 0 ? k : 1)));  // a g x g grid holds k centres
    std::vector<std::array<float, 2>> init((size_t)(k > 0 ? k : 0));
    for (int i = 0; i < k; ++i)
        init[i] = {(float)((i % g + 0.5) * W / g), (float)((i / g + 0.5) * H / g)};
    const ecc::KMeans::Windows r = km.fit_windows(rep, window, uniq, init);
    const ecc::WindowFlow f = ecc::window_centroid_flow(r.centroids, r.sizes, k);
    std::printf("window,centre,x,y,n,has_prev,dx,dy\n");
    for (int64_t w = 0; w < r.n_windows; ++w)
        for (int c = 0; c < k; ++c) {
            const int64_t i = w * k + c;
            std::printf("%lld,%d,%.9g,%.9g,%d,%d,%.9g,%.9g\n", (long long)w, c, r.centroids[2 * i], r.centroids[2 * i + 1],
                        r.sizes[i], (int)f.has_prev[i], f.diff[2 * i], f.diff[2 * i + 1]);
        }
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "--windows")) return run_windows(argc, argv);
        std::vector<std::array<float, 2>> pts(2048);
        for (int i = 0; i < 4096; ++i) pts[i / 2][i % 2] = (float)(i % 100);
        std::vector<std::array<float, 2>> c = {{1, 1}, {10, 10}, {20, 20}, {30, 30}, {50, 50}, {60, 60}, {70, 70}, {80, 80}};
        ecc::Context ctx(0);
        ecc::KMeans km(ctx, 8, 20, 50.f, 10.f);  // the reference stops when error_max <= 10 (:545)
        int iters = 0;
        const std::vector<uint8_t> lab = km.fit(pts, c, &iters);
        std::vector<int> cnt(8, 0);
        for (uint8_t l : lab) if (l < 8) cnt[l]++;
        std::printf("updated centroids (%d iterations)\n", iters);
        for (int j = 0; j < 8; ++j) std::printf("(%f, %f, %d) ", c[j][0], c[j][1], cnt[j]);
        std::printf("\n");
    } catch (const ecc::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
