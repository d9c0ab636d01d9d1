// Stand-alone probe of csrc/grid_geometry.hpp (the cloud cell grid's arithmetic) for
// tests/test_cloud_grid_geometry.py: its own main, only that header, no HIP, no libecc.
// It prints what it computed as `key=value` text lines; the Python test does the asserting.
//
//   term   hostile bounding boxes through grid_geometry() and through the sizing loop as it was
//          before it got a bound (restated below, with an iteration cap so that this program
//          cannot spin where that loop did)
//   same   random finite boxes: the new function against the old loop, bit for bit
//   claim  the one-cell claim on geometries chosen to be worst for it, >= 10^6 pairs each
#include "grid_geometry.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>

using ecc::rgrid::Grid;

// ---- the sizing loop of grid_setup_kernel before the bound, verbatim but for the cap --------
static bool old_grid(const double *mn, const double *mx, int dim, double eps, int64_t max_cells, int cap, Grid &out,
                     int &doublings) {
    Grid r{};
    r.dim = dim;
    double cs = eps > 0.0 ? eps * (1.0 + 1e-6) : 1.0;
    double span[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < dim; ++d) {
        r.mn[d] = mn[d];
        span[d] = mx[d] - r.mn[d];
        if (!(span[d] >= 0.0)) span[d] = 0.0;  // no finite point at all: one cell
    }
    for (doublings = 0;; ++doublings) {
        if (doublings == cap) return false;
        int64_t cells = 1;
        bool ok = true;
        for (int d = 0; d < dim; ++d) {
            const double c = floor(span[d] / cs) + 1.0;
            if (!(c < 4.0e18)) { ok = false; break; }
            r.dims[d] = (int64_t)c;
            if (cells > max_cells / r.dims[d] + 1) { ok = false; break; }
            cells *= r.dims[d];
        }
        if (ok && cells <= max_cells) {
            r.n_cells = cells;
            break;
        }
        cs *= 2.0;
    }
    for (int d = dim; d < 3; ++d) r.dims[d] = 1;
    r.cs = cs;
    out = r;
    return true;
}

static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}
static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

static bool same_grid(const Grid &a, const Grid &b) {
    bool s = bits_of(a.cs) == bits_of(b.cs) && a.n_cells == b.n_cells && a.dim == b.dim;
    for (int d = 0; d < 3; ++d) s = s && a.dims[d] == b.dims[d];
    for (int d = 0; d < a.dim; ++d) s = s && bits_of(a.mn[d]) == bits_of(b.mn[d]);
    return s;
}

constexpr int kOldCap = 5000;
constexpr int64_t kCellsSmall = 4096, kCellsMax = (int64_t)INT32_MAX - 1;

// ---- term ------------------------------------------------------------------------------------
static void run_term() {
    // what bbox_init_kernel's keys stand for when no finite point was seen
    const double no_mn = from_bits(0x7fffffffffffffffull), no_mx = from_bits(0xffffffffffffffffull);
    const double boxes[][2] = {
        {-1e308, 1e308}, {-8.9e307, 8.9e307}, {0.0, 1.7e308}, {-DBL_MAX, DBL_MAX}, {-1e308, DBL_MAX},
        {5.0, 5.0}, {0.0, 0.0}, {-0.0, 0.0}, {no_mn, no_mx},
        {1.0, nextafter(1.0, 2.0)}, {1e15, nextafter(1e15, 2e15)}, {0.0, 5e-324}, {-1e300, nextafter(-1e300, 0.0)},
        {0.0, 1000.0}, {-1e15, 1e15}, {-3.0, 2147483644.5},
    };
    const double epss[] = {0.0, 5e-324, 1e-300, 1.0, 1e200, DBL_MAX};
    const int64_t caps[] = {kCellsSmall, kCellsMax};
    int id = 0;
    for (const auto &b : boxes)
        for (double eps : epss)
            for (int dim = 1; dim <= 3; ++dim)
                for (int every_axis = 0; every_axis <= (dim > 1 ? 1 : 0); ++every_axis)
                    for (int64_t max_cells : caps) {
                        // the hostile box on axis 0 (or on every axis), a friendly [0, 10] elsewhere
                        double mn[3] = {0.0, 0.0, 0.0}, mx[3] = {10.0, 10.0, 10.0};
                        for (int d = 0; d < (every_axis ? dim : 1); ++d) mn[d] = b[0], mx[d] = b[1];
                        int nd = -1, od = -1;
                        const Grid g = ecc::rgrid::grid_geometry(mn, mx, dim, eps, max_cells, &nd);
                        Grid o{};
                        const bool ended = old_grid(mn, mx, dim, eps, max_cells, kOldCap, o, od);
                        std::printf("term id=%d dim=%d max_cells=%" PRId64 " eps=%a mn=%a,%a,%a mx=%a,%a,%a "
                                    "doublings=%d cs=%a dims=%" PRId64 ",%" PRId64 ",%" PRId64 " n_cells=%" PRId64
                                    " old_ended=%d old_doublings=%d same_as_old=%d\n",
                                    id++, dim, max_cells, eps, mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], nd, g.cs,
                                    g.dims[0], g.dims[1], g.dims[2], g.n_cells, ended ? 1 : 0, od,
                                    ended && same_grid(g, o) ? 1 : 0);
                    }
}

// ---- same ------------------------------------------------------------------------------------
struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t seed) : g(seed) {}
    uint64_t u64() { return g(); }
    double unit() { return (double)(g() >> 11) * 0x1.0p-53; }  // [0, 1)
    double range(double a, double b) { return a + (b - a) * unit(); }
    int64_t below(int64_t n) { return (int64_t)(g() % (uint64_t)n); }
};

static void run_same() {
    Rng rng(20240611);
    int boxes = 0, mismatches = 0, not_ended = 0, doubled = 0, most = 0;
    for (int i = 0; i < 6000; ++i) {
        const int dim = 1 + (int)rng.below(3);
        const int64_t max_cells = (i & 1) ? kCellsMax : (int64_t)4096 << rng.below(12);
        // eps and extents log-uniform over scales whose squares and differences stay finite
        const double eps = (i % 50 == 0) ? 0.0 : pow(10.0, rng.range(i % 3 ? -6.0 : -300.0, i % 3 ? 4.0 : 150.0));
        double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) {
            const double ext = (i % 7 == 0 && d == 0) ? 0.0 : pow(10.0, rng.range(i % 3 ? -4.0 : -300.0, i % 3 ? 9.0 : 300.0));
            const double at = (rng.u64() & 1 ? 1.0 : -1.0) * pow(10.0, rng.range(-5.0, i % 3 ? 15.0 : 300.0));
            mn[d] = (i % 5 == 0) ? -ext * rng.unit() : at;
            mx[d] = mn[d] + ext;
        }
        int nd = -1, od = -1;
        const Grid g = ecc::rgrid::grid_geometry(mn, mx, dim, eps, max_cells, &nd);
        Grid o{};
        const bool ended = old_grid(mn, mx, dim, eps, max_cells, kOldCap, o, od);
        ++boxes;
        if (!ended) { ++not_ended; continue; }
        if (!same_grid(g, o) || nd != od) {
            if (mismatches++ < 5)
                std::printf("same_mismatch i=%d dim=%d eps=%a mn=%a mx=%a cs=%a old_cs=%a\n", i, dim, eps, mn[0], mx[0],
                            g.cs, o.cs);
        }
        doubled += nd > 0;
        most = nd > most ? nd : most;
    }
    std::printf("same boxes=%d old_not_ended=%d mismatches=%d doubled=%d most_doublings=%d\n", boxes, not_ended,
                mismatches, doubled, most);
}

// ---- claim -----------------------------------------------------------------------------------
// The reference's test in coordinate type T: the per-axis difference in T, widened, squared and
// summed left to right in double, `<= eps * eps`.
template <typename T>
static bool accepts(const T *p, const T *q, int dim, double eps2) {
    double s = 0.0;
    for (int d = 0; d < dim; ++d) {
        const volatile T diff = q[d] - p[d];  // rounded to T (no excess precision)
        const double dd = (double)diff;
        s = s + dd * dd;
    }
    return s <= eps2;
}

// One geometry: the box [lo, hi]^dim holds every point drawn; base points come from
// [near_lo, near_hi] on every axis.
template <typename T>
static void run_claim(const char *name, const char *tname, int dim, double lo, double hi, double near_lo, double near_hi,
                      double eps, int64_t max_cells, int64_t pairs, uint64_t seed) {
    // the box as the device sees it: min / max of the coordinates, as T values widened
    const double mn[3] = {(double)(T)lo, (double)(T)lo, (double)(T)lo};
    const double mx[3] = {(double)(T)hi, (double)(T)hi, (double)(T)hi};
    int nd = -1;
    const Grid g = ecc::rgrid::grid_geometry(mn, mx, dim, eps, max_cells, &nd);
    const double eps2 = eps * eps;
    const double ulp1 = sizeof(T) == 4 ? 0x1.0p-23 : 0x1.0p-52;
    Rng rng(seed);
    int64_t accepted = 0, adjacent = 0, violations = 0, drawn = 0, rounded_in = 0;
    double worst = 0.0;
    for (int64_t it = 0; it < pairs; ++it) {
        T p[3] = {0, 0, 0}, q[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) p[d] = (T)rng.range(near_lo, near_hi);
        const int kind = (int)(it & 3);
        if (kind <= 1) {  // q = p +- eps * (1 + k ulps) on one axis, equal on the others
            const int ax = (int)rng.below(dim);
            if (kind == 0) {  // p within three steps of a cell border: q then sits at the next border
                const double c = floor(((double)p[ax] - g.mn[ax]) / g.cs + 0.5);
                p[ax] = (T)(g.mn[ax] + c * g.cs);
                const int64_t j = rng.below(7) - 3;
                for (int64_t s = 0; s < (j < 0 ? -j : j); ++s) p[ax] = std::nextafter(p[ax], j < 0 ? (T)-INFINITY : (T)INFINITY);
            }
            const double k = (double)(rng.below(17) - 8);
            const double off = (rng.u64() & 1 ? 1.0 : -1.0) * eps * (1.0 + k * ulp1);
            for (int d = 0; d < dim; ++d) q[d] = p[d];
            q[ax] = (T)((double)p[ax] + off);
            // ... and up to two representable steps either way (where p is large, an ulp of eps
            // is lost in p + off, and the values next to the boundary are steps of p's own ulp)
            const int64_t j = rng.below(5) - 2;
            for (int64_t s = 0; s < (j < 0 ? -j : j); ++s) q[ax] = std::nextafter(q[ax], j < 0 ? (T)-INFINITY : (T)INFINITY);
        } else if (kind == 2) {  // a random offset below eps on every axis
            for (int d = 0; d < dim; ++d) q[d] = (T)((double)p[d] + eps * rng.range(-1.0, 1.0));
        } else {  // a random direction at distance eps * (1 + k ulps)
            double v[3], s = 0.0;
            for (int d = 0; d < dim; ++d) v[d] = rng.range(-1.0, 1.0), s += v[d] * v[d];
            const double r = eps * (1.0 + (double)(rng.below(17) - 8) * ulp1) / sqrt(s > 0.0 ? s : 1.0);
            for (int d = 0; d < dim; ++d) q[d] = (T)((double)p[d] + v[d] * r);
        }
        bool inside = true;
        for (int d = 0; d < dim; ++d)
            inside = inside && (double)p[d] >= mn[d] && (double)p[d] <= mx[d] && (double)q[d] >= mn[d] && (double)q[d] <= mx[d];
        if (!inside) continue;  // the grid was not built for it
        ++drawn;
        if (!accepts<T>(p, q, dim, eps2)) continue;
        ++accepted;
        bool adj = false, exact_out = false;
        for (int d = 0; d < dim; ++d) {
            const int64_t cp = ecc::rgrid::cell_coord((double)p[d], g.mn[d], g.cs, g.dims[d]);
            const int64_t cq = ecc::rgrid::cell_coord((double)q[d], g.mn[d], g.cs, g.dims[d]);
            const int64_t dc = cp > cq ? cp - cq : cq - cp;
            if (dc > 1) {
                if (violations++ < 5) std::printf("claim_violation name=%s axis=%d p=%a q=%a cp=%" PRId64 " cq=%" PRId64 "\n", name, d, (double)p[d], (double)q[d], cp, cq);
            }
            adj = adj || dc == 1;
            const double qd = fabs(((double)p[d] - g.mn[d]) / g.cs - ((double)q[d] - g.mn[d]) / g.cs);
            worst = qd > worst ? qd : worst;
            exact_out = exact_out || fabs((double)q[d] - (double)p[d]) > eps;  // the exact difference (dim 1)
        }
        adjacent += adj;
        rounded_in += (dim == 1 && exact_out);
    }
    std::printf("claim name=%s type=%s dim=%d eps=%a doublings=%d cs=%a dims=%" PRId64 ",%" PRId64 ",%" PRId64
                " drawn=%" PRId64 " accepted=%" PRId64 " adjacent=%" PRId64 " rounded_in=%" PRId64 " violations=%" PRId64
                " max_quotient_diff=%.17g margin=%.6e\n",
                name, tname, dim, eps, nd, g.cs, g.dims[0], g.dims[1], g.dims[2], drawn, accepted, adjacent, rounded_in,
                violations, worst, 1.0 - worst);
}

static void run_claims() {
    const int64_t P = 1200000;
    const double cs1 = 1.0 * (1.0 + 1e-6);
    // as many cells on one axis as an int32 cell id allows, not one doubling: pairs at the top
    const double top = 2147483645.5 * cs1;
    run_claim<double>("f64_1d_2^31_cells_top", "f64", 1, 0.0, top, top - 64.0, top, 1.0, kCellsMax, P, 1);
    run_claim<double>("f64_1d_2^31_cells_eps_0.1", "f64", 1, 0.0, 214748364.0, 214748364.0 - 8.0, 214748364.0, 0.1, kCellsMax, P, 2);
    run_claim<double>("f64_1d_mn_1e15", "f64", 1, 1e15, 1e15 + 2147483645.0, 1e15 + 2147483645.0 - 64.0, 1e15 + 2147483645.0, 1.0, kCellsMax, P, 3);
    run_claim<double>("f64_1d_mn_1e15_low", "f64", 1, 1e15, 1e15 + 2147483645.0, 1e15, 1e15 + 64.0, 1.0, kCellsMax, P, 4);
    run_claim<double>("f64_1d_negative_mn", "f64", 1, -2147483645.0, 0.25, -60.0, 0.25, 1.0, kCellsMax, P, 5);
    run_claim<double>("f64_1d_negative_mn_eps_0.3", "f64", 1, -644245093.0, 7.0, -7.0, 7.0, 0.3, kCellsMax, P, 6);
    run_claim<double>("f64_2d_mn_1e15_doubled", "f64", 2, 1e15, 1e15 + 1000.0, 1e15, 1e15 + 1000.0, 1.0, kCellsSmall, P, 7);
    run_claim<double>("f64_3d_negative_mn_doubled", "f64", 3, -1000.0, 24.0, -1000.0, 24.0, 0.7, kCellsSmall, P, 8);
    // float coordinates, the float-difference test: fine float spacing exists only near 0, so the
    // largest cell coordinates with near pairs come from a far negative mn
    run_claim<float>("f32_1d_negative_mn_2^31_cells", "f32", 1, -2147483520.0, 4.0, -4.0, 4.0, 1.0, kCellsMax, P, 9);
    run_claim<float>("f32_1d_negative_mn_eps_0.3", "f32", 1, -644245056.0, 2.0, -2.0, 2.0, 0.3, kCellsMax, P, 10);
    run_claim<float>("f32_1d_mn_2^22", "f32", 1, 4194304.0, 4194304.0 + 4096.0, 4194304.0, 4194304.0 + 4096.0, 1.5, kCellsMax, P, 11);
    run_claim<float>("f32_1d_top_2^24", "f32", 1, 0.0, 16777216.0, 16777216.0 - 4096.0, 16777216.0, 1.0, kCellsMax, P, 12);
    run_claim<float>("f32_2d_negative_mn_doubled", "f32", 2, -3000.0, 64.0, -3000.0, 64.0, 1.5, kCellsSmall, P, 13);
    run_claim<float>("f32_3d_offset_doubled", "f32", 3, 1000.0, 1100.0, 1000.0, 1100.0, 0.37, kCellsSmall, P, 14);
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "all";
    const bool all = !std::strcmp(mode, "all");
    if (all || !std::strcmp(mode, "term")) run_term();
    if (all || !std::strcmp(mode, "same")) run_same();
    if (all || !std::strcmp(mode, "claim")) run_claims();
    std::printf("done mode=%s max_doublings=%d\n", mode, ecc::rgrid::kMaxDoublings);
    return 0;
}
