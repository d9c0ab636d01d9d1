// Stand-in for FunctionalPlus <fplus/fplus.hpp>: the eleven names that the reference's OPTICS code
// (OPT/include/optics/optics.hpp, tree.hpp, kdTree.hpp) uses in the spans oracle/ref/ref_optics.cpp
// compiles.  Our code, written from the names' documented meaning; TEST INFRASTRUCTURE ONLY.
//
// Decisions a reader of the pins must know:
//   * nth_element_on(f, n, xs) returns SOME element of xs whose key f(x) is the n-th smallest
//     (0-based).  Which of several elements with equal keys is not pinned: compute_core_dist
//     (optics.hpp:286-299) uses only the returned element's distance, so ties cannot change a result.
//   * transform and keep_if keep the input order; justs keeps the order of the filled slots.
#pragma once

#include <algorithm>
#include <cstddef>
#include <set>
#include <utility>
#include <vector>

namespace fplus {

template <typename T>
class maybe {
public:
    maybe() : has_(false), value_() {}
    maybe(const T &v) : has_(true), value_(v) {}
    bool is_just() const { return has_; }
    bool is_nothing() const { return !has_; }
    const T &unsafe_get_just() const { return value_; }

private:
    bool has_;
    T value_;
};

template <typename T>
maybe<T> just(const T &v) {
    return maybe<T>(v);
}

template <typename T>
maybe<T> nothing() {
    return maybe<T>();
}

template <typename T>
std::vector<T> justs(const std::vector<maybe<T>> &xs) {
    std::vector<T> out;
    out.reserve(xs.size());
    for (const auto &x : xs)
        if (x.is_just()) out.push_back(x.unsafe_get_just());
    return out;
}

template <typename T>
T max(const T &a, const T &b) {
    return a < b ? b : a;
}

template <typename Pred, typename T>
std::vector<T> keep_if(Pred pred, const std::vector<T> &xs) {
    std::vector<T> out;
    for (const auto &x : xs)
        if (pred(x)) out.push_back(x);
    return out;
}

template <typename F, typename T>
auto transform(F f, const std::vector<T> &xs) -> std::vector<decltype(f(xs.front()))> {
    std::vector<decltype(f(xs.front()))> out;
    out.reserve(xs.size());
    for (const auto &x : xs) out.push_back(f(x));
    return out;
}

template <typename F, typename T>
T nth_element_on(F f, std::size_t n, std::vector<T> xs) {
    std::nth_element(xs.begin(), xs.begin() + static_cast<std::ptrdiff_t>(n), xs.end(),
                     [&f](const T &a, const T &b) { return f(a) < f(b); });
    return xs[n];
}

template <typename T>
bool all_unique(const std::vector<T> &xs) {
    return std::set<T>(xs.begin(), xs.end()).size() == xs.size();
}

template <typename T>
T maximum(const std::vector<T> &xs) {
    return *std::max_element(xs.begin(), xs.end());
}

template <typename T>
T sum(const std::vector<T> &xs) {
    T s = T();
    for (const auto &x : xs) s += x;
    return s;
}

}  // namespace fplus
