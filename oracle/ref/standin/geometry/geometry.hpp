// Stand-in for CrikeeIP Geometry <geometry/geometry.hpp>: the three names that the reference's
// OPTICS spans compiled by oracle/ref/ref_optics.cpp use.  Our code; TEST INFRASTRUCTURE ONLY.
// The library's own text is not in the reference tree, so these are readings, not copies:
//   * square_dist / dist: the sum of squared coordinate differences in double, and its double
//     square root.  Every fixture has INTEGER coordinates, for which the differences, squares and
//     the sum are exact, so any reading that returns the double square root of the exact integer
//     sum gives the same bits.  Float or double inputs with fractions are NOT pinned by this: there
//     the library's operation order (or a hypot) could differ in the last bit.
//   * in_range(a, b, range): |a - b| <= range, the reading of quirk Q25; the pins do
//     not test it against the library, only against our own other forms.
#pragma once

#include <array>
#include <cmath>
#include <cstddef>

namespace geom {

template <typename T, std::size_t N>
double square_dist(const std::array<T, N> &a, const std::array<T, N> &b) {
    double s = 0.0;
    for (std::size_t i = 0; i < N; ++i) {
        const double d = static_cast<double>(a[i]) - static_cast<double>(b[i]);
        s += d * d;
    }
    return s;
}

template <typename T, std::size_t N>
double dist(const std::array<T, N> &a, const std::array<T, N> &b) {
    return std::sqrt(square_dist<T, N>(a, b));
}

template <typename T>
bool in_range(const T &a, const T &b, const T &range) {
    return std::abs(a - b) <= range;
}

}  // namespace geom
