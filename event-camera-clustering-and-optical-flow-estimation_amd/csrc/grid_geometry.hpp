// The pure arithmetic of the cloud cell grid (radius_grid.hpp): how the cell size and the cell
// counts per axis follow from a bounding box, and which cell a coordinate lands in.  No HIP
// include: the same functions run in grid_setup_kernel / cell_count_kernel / for_runs on the
// device and in a host program (tests/cloud_grid_probe.cpp), with IEEE double +, -, *, / and
// floor only, so both give the same bits.
//
// The claim everything built on the grid rests on: two points that pass the reference's test
// (per-axis difference in the coordinate type T, widened, squared and summed in double,
// `<= eps * eps`) land at most one cell apart on every axis under floor((v - mn) / cs), for
// cs = eps * (1 + 1e-6) * 2^k.  With |p - q| <= eps * (1 + 2^-24) (the rounding of a float
// difference; 2^-53 for double) the exact quotients differ by at most (1 + 6e-8) / (1 + 1e-6)
// < 1 - 9.4e-7 cells.  The two roundings of (v - mn) / cs move a quotient x by at most
// x * 2^-53 (the subtraction) plus half an ulp of x (the division): below the largest cell
// coordinate there is, 2^31 (cell ids are int32), that is less than 2^-22 + 2^-23 = 3.6e-7
// cells per point, 7.2e-7 for a pair.  So the computed quotients differ by less than 1 and
// their floors by at most 1 (tests/cloud_grid_probe.cpp measures the margin that is left).
// Clamping a coordinate into [0, dims - 1] is monotone and never moves two cells further apart.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ECC_GEOM_FN __host__ __device__ __forceinline__
#else
#define ECC_GEOM_FN inline
#endif

namespace ecc {
namespace rgrid {

struct Grid {
    double mn[3];
    double cs;
    int64_t dims[3];
    int64_t n_cells;
    int dim;
};

// The sizing loop doubles cs at most this often.  The smallest cs it can start from is the
// smallest subnormal, 2^-1074 (eps * (1 + 1e-6) rounds to no less for eps > 0), and a span is at
// most DBL_MAX < 2^1024: after 1074 + 1024 = 2098 doublings cs >= 2^1024 exceeds every span (it
// has become +inf), floor(span / cs) is 0 on every axis and the one-cell grid fits any
// max_cells >= 1.  2100 leaves the two spare rounds for the first test and the last.
constexpr int kMaxDoublings = 2100;

// Extent of one axis of the bounding box [mn, mx].
//   * no finite point at all (mn, mx are the NaNs bbox_init_kernel's keys stand for): 0;
//   * mx - mn overflows (finite ends, e.g. -1e308 and 1e308): DBL_MAX.  The grid is then sized
//     for DBL_MAX; a point whose v - mn overflows gets +inf from the division and is clamped
//     into the last cell by cell_coord, together with everything beyond DBL_MAX from mn.
//     Merging cells at the far end loses nothing (the clamp is monotone), and no pair is asked
//     to be found across it that the reference finds: a per-axis difference that overflows has
//     d^2 = +inf, which is `<= eps * eps` only where eps * eps is +inf too, and that case gets
//     one cell below.  Clamping was chosen over mx / 2 - mn / 2 because it leaves every finite
//     span, and with it every grid that was built before, bit for bit as it was.
ECC_GEOM_FN double axis_span(double mn, double mx) {
    double s = mx - mn;
    if (!(s >= 0.0)) s = 0.0;
    if (s > DBL_MAX) s = DBL_MAX;
    return s;
}

// Grid over the box [mn, mx] (dim axes): cells of eps * (1 + 1e-6), or 1.0 for eps == 0 (and
// +inf where eps * eps overflows), doubled until floor(span / cs) + 1 cells per axis give at most max_cells cells in all.
// `doublings`, when not null, receives the number of doublings taken.
ECC_GEOM_FN Grid grid_geometry(const double *mn, const double *mx, int dim, double eps, int64_t max_cells,
                               int *doublings = nullptr) {
    Grid r{};
    r.dim = dim;
    double cs = eps > 0.0 ? eps * (1.0 + 1e-6) : 1.0;
    // eps * eps = +inf: `d2 <= eps * eps` holds for every pair of finite points, however far
    // apart, so cells of any finite size would separate neighbours: one unbounded cell
    if (eps * eps > DBL_MAX) cs = INFINITY;
    double span[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < dim; ++d) {
        r.mn[d] = mn[d];
        span[d] = axis_span(mn[d], mx[d]);
    }
    bool done = false;
    int it = 0;
    for (; it <= kMaxDoublings; ++it) {
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
            done = true;
            break;
        }
        cs *= 2.0;
    }
    if (!done) {  // not reached for max_cells >= 1 (see kMaxDoublings): one cell holds everything
        for (int d = 0; d < dim; ++d) r.dims[d] = 1;
        r.n_cells = 1;
    }
    for (int d = dim; d < 3; ++d) r.dims[d] = 1;
    r.cs = cs;
    if (doublings) *doublings = it;
    return r;
}

// Cell of coordinate v on an axis of `dims` cells: clamped into [0, dims - 1]; NaN (a NaN
// coordinate, or mn of a box without finite points, or inf / inf) goes to cell 0.
ECC_GEOM_FN int64_t cell_coord(double v, double mn, double cs, int64_t dims) {
    const double f = floor((v - mn) / cs);
    if (!(f >= 0.0)) return 0;  // also NaN
    return f >= (double)dims ? dims - 1 : (int64_t)f;
}

}  // namespace rgrid
}  // namespace ecc
