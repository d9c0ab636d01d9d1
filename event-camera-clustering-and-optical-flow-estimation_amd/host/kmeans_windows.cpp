// k-means per downsample window on the host side: the reference's per-id displacement of a slice's
// cluster centroids against the previous slice (TWE/…opencl_store.cpp:396-448: diff = cen -
// centroid_prev[id], drawn only where the id had a previous centroid; unscaled here), and the C++
// layer over ecc_kmeans_windows_xy16.
#include <cstdint>
#include <vector>

#include "../../include/ecc.hpp"

extern "C" __attribute__((visibility("default"))) int ecc_kmeans_windows_flow_host(const float *centroids,
                                                                                   const int32_t *sizes, int64_t n_segs,
                                                                                   int32_t k, float *diff,
                                                                                   uint8_t *has_prev) {
    if (!centroids || !sizes || !diff || !has_prev || k < 1 || n_segs < 0) return ECC_ERR_INVALID;
    for (int64_t w = 0; w < n_segs; ++w)
        for (int32_t c = 0; c < k; ++c) {
            const bool hp = w > 0 && sizes[(w - 1) * k + c] > 0 && sizes[w * k + c] > 0;
            has_prev[w * k + c] = hp ? 1 : 0;
            for (int d = 0; d < 2; ++d) {
                const int64_t i = w * 2 * k + 2 * c + d;
                diff[i] = hp ? centroids[i] - centroids[i - 2 * k] : 0.f;
            }
        }
    return ECC_OK;
}

namespace ecc {

static void check(int rc, const char *what) {
    if (rc != ECC_OK) throw Error(rc, what);
}

KMeans::Windows KMeans::fit_windows(const std::vector<uint32_t> &xy, int64_t stride, const std::vector<int32_t> &counts,
                                    const std::vector<std::array<float, 2>> &init) {
    if ((int)init.size() != cfg_.k) throw Error(ECC_ERR_INVALID, "KMeans::fit_windows: init.size() != k");
    if (stride < 1 || xy.size() % (size_t)stride) throw Error(ECC_ERR_INVALID, "KMeans::fit_windows: xy.size() % stride");
    Windows r;
    r.n_windows = (int64_t)(xy.size() / (size_t)stride);
    if (!counts.empty() && (int64_t)counts.size() != r.n_windows)
        throw Error(ECC_ERR_INVALID, "KMeans::fit_windows: counts.size() != windows");
    const size_t nw = (size_t)r.n_windows, k = (size_t)cfg_.k;
    r.centroids.assign(nw * 2 * k, 0.f);
    r.labels.assign(xy.size(), 255);
    r.sizes.assign(nw * k, 0);
    r.iters.assign(nw, 0);
    ecc_stream_t s = ctx_.stream();
    DeviceBuffer d_xy, d_cnt, d_init, d_c(r.centroids.size() * 4), d_l, d_sz(r.sizes.size() * 4), d_it(nw * 4);
    d_xy.upload(xy.data(), xy.size() * 4, s);
    if (!counts.empty()) d_cnt.upload(counts.data(), counts.size() * 4, s);
    d_init.upload(init.data(), k * 8, s);
    d_l.upload(r.labels.data(), r.labels.size(), s);  // labels past a count stay 255
    check(ecc_kmeans_windows_xy16(ctx_.get(), d_xy.as<uint32_t>(), r.n_windows, stride,
                                  counts.empty() ? nullptr : d_cnt.as<int32_t>(), &cfg_, d_init.as<float>(),
                                  d_c.as<float>(), d_l.as<uint8_t>(), d_sz.as<int32_t>(), d_it.as<int32_t>(), s),
          "ecc_kmeans_windows_xy16");
    d_c.download(r.centroids.data(), r.centroids.size() * 4, s);
    d_l.download(r.labels.data(), r.labels.size(), s);
    d_sz.download(r.sizes.data(), r.sizes.size() * 4, s);
    d_it.download(r.iters.data(), nw * 4, s);
    ctx_.sync();
    return r;
}

WindowFlow window_centroid_flow(const std::vector<float> &centroids, const std::vector<int32_t> &sizes, int k) {
    if (k < 1 || sizes.size() % (size_t)k || centroids.size() != 2 * sizes.size())
        throw Error(ECC_ERR_INVALID, "window_centroid_flow: array sizes");
    WindowFlow f;
    f.diff.assign(centroids.size(), 0.f);
    f.has_prev.assign(sizes.size(), 0);
    if (sizes.empty()) return f;
    check(ecc_kmeans_windows_flow_host(centroids.data(), sizes.data(), (int64_t)(sizes.size() / (size_t)k), k,
                                       f.diff.data(), f.has_prev.data()),
          "ecc_kmeans_windows_flow_host");
    return f;
}

}  // namespace ecc
