// The xi-cluster hierarchy of every segment in one launch: optics::flat_clusters_to_tree
// (OPT/include/optics/optics.hpp:948-995) over the flat pairs ecc_optics_xi leaves on the device,
// as (sorted, parent, level) arrays that determine the reference's forest exactly.
//
// A workgroup per segment (about 415 pairs per downsample window: two trips of 256 threads; a
// wave per segment would walk the same scans in seven).  Both of the reference's steps are
// "the first later entry that ...", which a thread per entry scans for, four entries a trip:
//   * placement (:950-966).  run(i) ends at nge(i), the first j > i with second[j] > second[i]
//     (or P).  The runs nest, the literal loop's slot is the post-order of that nesting:
//       slot(i) = i + run(i) - #{a < i : nge(a) > i} = nge(i) - i - 1 + #{a : nge(a) <= i},
//     and the last term is a histogram of nge followed by an inclusive prefix sum.
//   * parents (:974-992): the first j > k in the placed list whose interval holds k's.
//   * level: parent(k) > k, so blocks of kNT positions are finished from the top down; inside a
//     block a thread climbs at most kNT parents before it meets a finished position or a root.
// Nothing in LDS grows with pair_cap: of every per-segment array the first kLdsPairs entries live
// in LDS and the rest in the segment's own output rows, which double as scratch until their final
// values are written (nge and slot in `parent`, the histogram in the even words of `sorted`).
// A segment of at most kLdsPairs pairs runs the same text with the global branch compiled out.
// Pair values are only ever compared, never used as an index.
#include "ecc_internal.hpp"

namespace {

constexpr int kNT = 256;
constexpr int kLdsPairs = 512;  // entries of each per-segment array held in LDS (12 KiB per workgroup)
constexpr int64_t kMaxBlocks = int64_t(1) << 30;  // segments (workgroups) per launch

// One per-segment int array: entry k in LDS for k < kLdsPairs, else word k * kStep of a global row.
// kSpill = false: the segment has at most kLdsPairs entries.
template <int kStep, bool kSpill>
struct Arr {
    int32_t *lds;
    int32_t *row;
    __device__ __forceinline__ int ld(int k) const { return !kSpill || k < kLdsPairs ? lds[k] : row[(int64_t)k * kStep]; }
    __device__ __forceinline__ void st(int k, int v) const {
        if (!kSpill || k < kLdsPairs) lds[k] = v;
        else row[(int64_t)k * kStep] = v;
    }
    __device__ __forceinline__ void add1(int k) const {
        if (!kSpill || k < kLdsPairs) atomicAdd(&lds[k], 1);
        else atomicAdd(&row[(int64_t)k * kStep], 1);
    }
};

// {first, second} pairs: LDS for k < kLdsPairs, else words 2k, 2k + 1 of a global row.
template <bool kSpill, class Row>
struct Pairs {
    int2 *lds;
    Row *row;
    __device__ __forceinline__ int2 ld(int k) const {
        return !kSpill || k < kLdsPairs ? lds[k] : make_int2(row[(int64_t)k * 2], row[(int64_t)k * 2 + 1]);
    }
    __device__ __forceinline__ int second(int k) const { return !kSpill || k < kLdsPairs ? lds[k].y : row[(int64_t)k * 2 + 1]; }
};

// The first j in (k, P) with hit(j), or P: four independent reads a trip.
template <class Hit>
__device__ __forceinline__ int first_after(int k, int P, Hit hit) {
    int j = k + 1;
    for (; j + 3 < P; j += 4) {
        const bool h0 = hit(j), h1 = hit(j + 1), h2 = hit(j + 2), h3 = hit(j + 3);
        if (h0 | h1 | h2 | h3) return h0 ? j : h1 ? j + 1 : h2 ? j + 2 : j + 3;
    }
    for (; j < P; ++j)
        if (hit(j)) return j;
    return P;
}

// A workgroup barrier; with part of the arrays in global memory, an agent fence on both sides of it.
template <bool kSpill>
__device__ __forceinline__ void sync() {
    if (kSpill) __threadfence();
    __syncthreads();
    if (kSpill) __threadfence();
}

struct Lds {  // 12 KiB
    int2 in[kLdsPairs], sorted[kLdsPairs];
    int32_t a[kLdsPairs], b[kLdsPairs];
    int32_t wave[kNT / 64], roots;
};

// One segment: P pairs at in_row; the segment's rows of the outputs (level_row may be null).
template <bool kSpill>
__device__ __forceinline__ void tree_of_segment(Lds &S, int P, const int32_t *__restrict__ in_row, int32_t *sorted_row,
                                                int32_t *parent_row, int32_t *level_row, int32_t *n_roots) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int in_lds = min(P, kLdsPairs);
    const Pairs<kSpill, const int32_t> in{S.in, in_row};
    const Pairs<kSpill, int32_t> placed{S.sorted, sorted_row};
    const Arr<1, kSpill> A{S.a, parent_row};  // nge, then slot, then parent
    const Arr<2, kSpill> B{S.b, sorted_row};  // histogram of nge, then its prefix sums (dead before `sorted` is written)
    const Arr<1, kSpill> L{S.b, level_row};   // level (after B is dead)

    if (t == 0) S.roots = 0;
    for (int k = t; k < in_lds; k += kNT) S.in[k] = make_int2(in_row[(int64_t)k * 2], in_row[(int64_t)k * 2 + 1]);
    __syncthreads();

    // ---- placement (:950-966)
    for (int i = t; i < P; i += kNT) {
        const int sec = in.second(i);
        A.st(i, first_after(i, P, [&](int j) { return in.second(j) > sec; }));
        B.st(i, 0);
    }
    sync<kSpill>();
    for (int i = t; i < P; i += kNT) {
        const int n = A.ld(i);
        if (n < P) B.add1(n);
    }
    sync<kSpill>();
    int carry = 0;  // B[k] = #{a : nge(a) <= k}
    for (int base = 0; base < P; base += kNT) {
        const int k = base + t;
        const int incl = ecc::wave_incl_scan(k < P ? B.ld(k) : 0);
        if (lane == 63) S.wave[wave] = incl;
        __syncthreads();
        int before = carry, total = carry;
        for (int w = 0; w < kNT / 64; ++w) {
            const int v = S.wave[w];
            if (w < wave) before += v;
            total += v;
        }
        if (k < P) B.st(k, before + incl);
        carry = total;
        __syncthreads();
    }
    sync<kSpill>();
    for (int i = t; i < P; i += kNT) A.st(i, A.ld(i) - i - 1 + B.ld(i));
    sync<kSpill>();  // B is dead: its global words are `sorted`'s
    for (int i = t; i < P; i += kNT) {
        const int slot = A.ld(i);
        const int2 c = in.ld(i);
        if (!kSpill || slot < kLdsPairs) {
            S.sorted[slot] = c;
        } else {
            sorted_row[(int64_t)slot * 2] = c.x;
            sorted_row[(int64_t)slot * 2 + 1] = c.y;
        }
    }
    sync<kSpill>();

    // ---- parents (:974-992)
    int roots = 0;
    for (int k = t; k < P; k += kNT) {
        const int2 c = placed.ld(k);
        const int j = first_after(k, P, [&](int q) {
            const int2 o = placed.ld(q);
            return c.x >= o.x && c.y <= o.y;
        });
        A.st(k, j < P ? j : -1);
        roots += j >= P;
    }
    if (roots) atomicAdd(&S.roots, roots);
    sync<kSpill>();

    // ---- level: blocks of kNT positions from the top down
    if (level_row) {
        for (int hi = P; hi > 0; hi -= kNT) {
            const int k = hi - 1 - t;
            if (k >= 0) {
                int up = 0, a = k, lvl;
                for (;;) {
                    const int p = A.ld(a);
                    if (p < 0) { lvl = up; break; }
                    if (p >= hi) { lvl = up + 1 + L.ld(p); break; }
                    a = p, ++up;
                }
                L.st(k, lvl);
            }
            sync<kSpill>();
        }
    }

    // ---- the LDS part of the rows
    for (int k = t; k < in_lds; k += kNT) {
        const int2 c = S.sorted[k];
        sorted_row[(int64_t)k * 2] = c.x;
        sorted_row[(int64_t)k * 2 + 1] = c.y;
        parent_row[k] = S.a[k];
        if (level_row) level_row[k] = S.b[k];
    }
    if (t == 0) *n_roots = S.roots;
}

__global__ __launch_bounds__(kNT) void optics_xi_tree_kernel(const int32_t *__restrict__ pairs, int64_t cap,
                                                              const int32_t *__restrict__ n_pairs, int64_t s0,
                                                              int32_t *sorted, int32_t *parent, int32_t *level,
                                                              int32_t *n_roots, int32_t *flag) {
    __shared__ Lds S;
    const int64_t s = s0 + blockIdx.x;
    const int raw = n_pairs[s];
    if (raw > cap) {  // a truncated flat list: no tree of it
        if (threadIdx.x == 0) {
            n_roots[s] = -1;
            *flag = 1;
        }
        return;
    }
    const int P = raw < 0 ? 0 : raw;
    int32_t *level_row = level ? level + s * cap : nullptr;
    if (P <= kLdsPairs)
        tree_of_segment<false>(S, P, pairs + s * cap * 2, sorted + s * cap * 2, parent + s * cap, level_row, n_roots + s);
    else
        tree_of_segment<true>(S, P, pairs + s * cap * 2, sorted + s * cap * 2, parent + s * cap, level_row, n_roots + s);
}

}  // namespace

ECC_API int ecc_optics_xi_tree(ecc_ctx *ctx, const int32_t *pairs, int64_t pair_cap, const int32_t *n_pairs,
                               int64_t n_segs, int32_t *sorted, int32_t *parent, int32_t *level, int32_t *n_roots,
                               ecc_stream_t stream) {
    if (!ctx || n_segs < 0 || pair_cap < 0) return ECC_ERR_INVALID;
    if (n_segs > 0 && (!pairs || !n_pairs || !sorted || !parent || !n_roots)) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    ECC_CHECK_HIP(ctx, hipMemsetAsync(&ctx->dev->optics_xi_tree, 0, 4, s), "memset(optics xi tree err)");
    ECC_TIMED(ctx, s, "optics_xi_tree_kernel");
    for (int64_t s0 = 0; s0 < n_segs; s0 += kMaxBlocks) {
        hipLaunchKernelGGL(optics_xi_tree_kernel, dim3((unsigned)std::min(n_segs - s0, kMaxBlocks)), dim3(kNT), 0, s,
                           pairs, pair_cap, n_pairs, s0, sorted, parent, level, n_roots, &ctx->dev->optics_xi_tree);
        ECC_CHECK_LAUNCH(ctx, "optics_xi_tree");
    }
    return ECC_OK;
}

ECC_API int ecc_optics_xi_tree_status(ecc_ctx *ctx, ecc_stream_t stream) {
    if (!ctx) return ECC_ERR_INVALID;
    int32_t f = 0;
    if (int rc = ecc::read_dev_words(ctx, &ctx->dev->optics_xi_tree, 1, &f, ecc::as_stream(stream))) return rc;
    return f ? ECC_ERR_CAPACITY : ECC_OK;
}
