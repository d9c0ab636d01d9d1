// Stand-alone check of csrc/run_bitmap.hpp (only that header; no HIP, no libecc): the half-width
// table, the box geometry, ranks and the row-run count against brute force over the pixel list.
// Prints "OK queries=<n>" and returns 0, or says what failed and returns 1.
#include "run_bitmap.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

using namespace ecc::runbm;

namespace {

int fails = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++fails <= 20) {                          \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

struct Px {
    int x, y;
};

void check_half_widths() {
    const double epss[] = {0.0, 0.5, 1.0, 1.01, std::sqrt(2.0), 10.0, 31.9, 32.0, 37.9, 400.0, 511.9};
    for (double eps : epss) {
        const uint32_t r2i = (uint32_t)std::floor(eps * eps);
        const int e_int = (int)std::floor(eps);
        for (int a = 0; a <= e_int; ++a) {
            const uint64_t v = (uint64_t)r2i - (uint64_t)a * a;
            uint64_t h = 0;
            while ((h + 1) * (h + 1) <= v) ++h;
            CHECK(half_width(r2i, a) == h, "eps %g a %d: %u, expected %llu", eps, a, half_width(r2i, a),
                  (unsigned long long)h);
        }
    }
}

// The device's prefix pass, sequentially: wd[w].y = set bits of wd[0 .. w).
void prefix_words_host(std::vector<Word> &wd, int64_t words) {
    uint32_t off = 0;
    for (int64_t w = 0; w < words; ++w) {
        wd[w].y = off;
        off += (uint32_t)__builtin_popcount(wd[w].x);
    }
}

long long check_window(const std::vector<Px> &pts, int W, int Hh, int x0, int y0) {
    int xmn = 0x7fffffff, ymn = 0x7fffffff, xmx = -1, ymx = -1;
    for (const Px &p : pts) {
        xmn = std::min(xmn, p.x), ymn = std::min(ymn, p.y);
        xmx = std::max(xmx, p.x), ymx = std::max(ymx, p.y);
    }
    const Box b((int)pts.size(), xmn, ymn, xmx, ymx);
    CHECK(b.xmn == x0 && b.ymn == y0 && b.Wb == W && b.H == Hh && b.WW == (W >> 5) + 1 &&
              b.words() == (int64_t)Hh * ((W >> 5) + 1),
          "box %d x %d: xmn %d ymn %d Wb %d H %d WW %d", W, Hh, b.xmn, b.ymn, b.Wb, b.H, b.WW);
    const int zero_word = (int)b.words();
    std::vector<Word> wd(b.words() + 1, Word{0u, 0u});
    for (const Px &p : pts) {
        const int x = p.x - b.xmn, y = p.y - b.ymn;
        CHECK(word_of(b, x, y) >= 0 && word_of(b, x, y) < zero_word, "word_of(%d, %d) = %d", x, y, word_of(b, x, y));
        CHECK(!(wd[word_of(b, x, y)].x & bit_of(x)), "pixel (%d, %d) twice", x, y);
        wd[word_of(b, x, y)].x |= bit_of(x);
    }
    prefix_words_host(wd, b.words());
    // raster ranks
    std::vector<Px> ras = pts;
    std::sort(ras.begin(), ras.end(), [](const Px &a, const Px &c) { return a.y != c.y ? a.y < c.y : a.x < c.x; });
    for (size_t r = 0; r < ras.size(); ++r)
        CHECK(rank_at(wd.data(), b, ras[r].x - b.xmn, ras[r].y - b.ymn) == (int)r, "rank of (%d, %d)", ras[r].x,
              ras[r].y);
    // counts: every set pixel, each eps
    long long queries = 0;
    bool edge[4] = {false, false, false, false};
    const double epss[] = {0.0, 0.5, 1.01, 3.7, 10.0, 31.9, 37.9, 70.0};
    for (double eps : epss) {
        const uint32_t r2i = (uint32_t)std::floor(eps * eps);
        const int e_int = (int)std::floor(eps);
        std::vector<uint16_t> hwt(e_int + 1);
        for (int a = 0; a <= e_int; ++a) hwt[a] = (uint16_t)half_width(r2i, a);
        const int amax = std::min(e_int, b.H - 1);
        for (const Px &p : pts) {
            int want = 0;
            for (const Px &q : pts) {
                const long long dx = q.x - p.x, dy = q.y - p.y;
                want += dx * dx + dy * dy <= (long long)r2i;
            }
            const int x = p.x - b.xmn, y = p.y - b.ymn;
            const int got = chord_count(wd.data(), zero_word, b, hwt.data(), x, y, amax);
            CHECK(got == want, "box %d x %d eps %g (%d, %d): %d, expected %d", W, Hh, eps, x, y, got, want);
            edge[0] |= x == 0, edge[1] |= x == b.Wb - 1, edge[2] |= y == 0, edge[3] |= y == b.H - 1;
            ++queries;
        }
    }
    CHECK(edge[0] && edge[1] && edge[2] && edge[3], "box %d x %d: no query on some edge", W, Hh);
    return queries;
}

}  // namespace

int main() {
    check_half_widths();

    {  // no points: one pixel, one word
        const Box b(0, 0x7fffffff, 0x7fffffff, -1, -1);
        CHECK(b.Wb == 1 && b.H == 1 && b.WW == 1 && b.words() == 1, "empty box: Wb %d H %d WW %d", b.Wb, b.H, b.WW);
    }
    long long queries = check_window({Px{123, 45}}, 1, 1, 123, 45);  // one point

    std::mt19937 rng(20240607u);
    const int widths[] = {1, 31, 32, 33, 63, 64, 65}, heights[] = {1, 40};
    const double occ[] = {0.05, 0.5, 1.0};
    const int x0 = 7, y0 = 3;  // the box does not start at the origin
    for (int W : widths)
        for (int Hh : heights)
            for (double p : occ) {
                std::vector<Px> pts;
                std::bernoulli_distribution set(p);
                for (int y = 0; y < Hh; ++y)
                    for (int x = 0; x < W; ++x) {
                        const bool corner = (x == 0 && y == 0) || (x == W - 1 && y == Hh - 1);  // pins the box
                        if (corner || p >= 1.0 || set(rng)) pts.push_back(Px{x0 + x, y0 + y});
                    }
                std::shuffle(pts.begin(), pts.end(), rng);
                queries += check_window(pts, W, Hh, x0, y0);
            }

    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("OK queries=%lld\n", queries);
    return 0;
}
