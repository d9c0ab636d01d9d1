// OPTICS ordering and threshold clusters of many independent point segments (downsample windows)
// in one launch ("OPTICS eps 10 / min_pts 2 per 8192-rep window").
//
// Reference: optics::compute_reachability_dists, OPT/include/optics/optics.hpp — core distances
// (:286-299), the reachability update (:315-337), the ordered seed-set expansion (:525-555) — and
// get_cluster_indices (:674-690), as driven by OPT/test/cluster_event_data.cpp:449-454
// (min_pts 2, eps 10, threshold 10).
//
// Integer keys.  Coordinates are integers, so every d^2 is an exact integer below 2^31, and
//   reach = max(core, dist) = sqrt(max(core^2, d^2))
// because sqrt is monotone and correctly rounded; fp64 sqrt is injective on integers below 2^32,
// so the reference's seed order (reach, index) (:67-69) is the integer order (reach^2, index).
// The whole expansion runs on u32 keys; fp64 appears only at the output: sqrt((double)reach2)
// and the `>= threshold` test.
//
// MI355X design: one 1024-lane workgroup per segment (eps_grid.hpp's binning is written for one).
//   1. bin   the points into the LDS cell grid (bin_cells, fine cells);
//   2. core  core2[q] for all points in parallel: the (min_pts-1)-th smallest d^2 of the eps-ball
//            in a register insertion network (eps.hip's rule), 0xffffffff below min_pts points;
//   3. expand  by wave 0 alone, so the step loop has no workgroup barrier (the other 15 waves wait
//            at the barrier after it).  The reference's per-start std::set is exactly the set
//            {unprocessed and reach2 defined}, and it drains before the outer loop moves on, so
//            one member list serves the whole segment: a point enters it when its reach2 becomes
//            defined (once) and leaves it when it is emitted (swap-remove).  The list stores
//            positions only and the key is read from reach2[] at extraction time, so there are
//            no stale entries, the list never holds more than the unprocessed points and nothing
//            can overflow.  Extract-min: the lanes stride over the list, each keeps its best
//            (reach2, index), one DPP wave minimum picks the winner.  The neighbour update walks
//            the candidate cell runs of the emitted point with all 64 lanes (the runs of the up
//            to seven cell rows laid end to end); a candidate belongs to exactly one lane, so
//            reach2[] needs no atomics, and new members are appended by ballot + prefix count.
//            The emitted order grows from the front of the same u16 array whose back holds the
//            member list (emitted + members <= m).
//   4. out   order / reach coalesced; the cluster ids are a block scan over the flags
//            reach < 0 || reach >= threshold, compared in fp64 as the reference does.
// All tables are in cell order (position q); sidx[q] is the segment-local index.
#include "eps_grid.hpp"

#include <algorithm>
#include <cmath>

namespace {

using ecc::epsg::CellGrid;
using ecc::epsg::kCells;
using ecc::epsg::kMaxR;
using ecc::epsg::kNT;

constexpr int kMaxPts = 8192;
constexpr int kPer = kMaxPts / kNT;  // ordered entries per lane in the threshold scan
constexpr uint32_t kUndef = 0xffffffffu;

// Orders this wave's LDS accesses across its lanes (the LDS serves one wave's requests in order;
// this keeps the compiler from moving accesses over the point).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Dynamic LDS bytes of optics_grid_kernel at a stride.
inline size_t optics_lds_bytes(int64_t stride) {
    const size_t bw = (size_t)((stride + 31) >> 5);
    return (size_t)(kCells + 1 + 3 * stride + 2 * bw) * 4 + (size_t)((stride + 1) & ~1ll) * 2 * 2;
}

// The ordered expansion of one binned segment (wave 0, all 64 lanes).  On return ol[0, m) holds
// the positions in emission order and reach2[] the final squared reachabilities.
__device__ __forceinline__ void expand_segment(const CellGrid &g, int m, int bw, int e_int, uint32_t r2i,
                                               const uint32_t *cend, const uint32_t *spt, const uint16_t *sidx,
                                               const uint32_t *core2, uint32_t *reach2, uint32_t *live,
                                               uint32_t *todo, uint16_t *ol) {
    const int lane = threadIdx.x & 63;
    int n_out = 0;   // emitted: ol[0, n_out)
    int n_seed = 0;  // members: ol[m - n_seed, m), member j at ol[m - 1 - j]
    int next_w = 0;  // todo[] words before this one are empty
    for (int step = 0; step < m; ++step) {  // one point is emitted per step
        int q;
        if (n_seed > 0) {  // uniform: the member with the smallest (reach2, index)
            int64_t best = INT64_MAX;
            int bq = 0, bj = 0;
            for (int j = lane; j < n_seed; j += 64) {
                const int qq = ol[m - 1 - j];
                const int64_t key = ((int64_t)reach2[qq] << 32) | (int64_t)((uint32_t)sidx[qq] << 8) | lane;
                if (key < best) {
                    best = key;
                    bq = qq;
                    bj = j;
                }
            }
            const int wl = (int)(ecc::wave_min_i64(best) & 63);  // DPP; the winner's lane
            q = ecc::lane_value(bq, wl);
            const int j = ecc::lane_value(bj, wl);
            if (lane == 0) ol[m - 1 - j] = ol[m - n_seed];  // swap-remove
            --n_seed;
        } else {  // the outer loop's next unprocessed index (:525-526) and its position
            int i = -1;
            for (; next_w < bw; next_w += 64) {
                const int w = next_w + lane;
                const uint32_t bits = w < bw ? todo[w] : 0u;
                const uint64_t bal = __ballot(bits != 0u);
                if (bal) {
                    const int fl = __ffsll((unsigned long long)bal) - 1;
                    i = (next_w + fl) * 32 + __ffs(ecc::lane_value((int)bits, fl)) - 1;
                    break;
                }
            }
            if (i < 0) break;  // (every step finds one: todo holds the m - step unprocessed points)
            q = -1;
            for (int t0 = 0; t0 < m; t0 += 64) {
                const int t = t0 + lane;
                const uint64_t bal = __ballot(t < m && sidx[t] == i);
                if (bal) {
                    q = t0 + __ffsll((unsigned long long)bal) - 1;
                    break;
                }
            }
            if (q < 0) break;
        }
        const int iq = uniform(sidx[q]);
        if (lane == 0) {
            ol[n_out] = (uint16_t)q;
            live[q >> 5] &= ~(1u << (q & 31));
            todo[iq >> 5] &= ~(1u << (iq & 31));
        }
        ++n_out;
        wave_sync();
        const uint32_t c2 = (uint32_t)uniform((int)core2[q]);
        if (c2 == kUndef) continue;  // not a core point: no update (:535, :549)
        // update (:315-337) over the candidate runs of q's cell rows, laid end to end
        const uint32_t v = (uint32_t)uniform((int)spt[q]);
        const int cx = ecc::epsg::cell_x(g, v), cy = ecc::epsg::cell_y(g, v);
        int lo[2 * kMaxR + 1], len[2 * kMaxR + 1], total = 0;
#pragma unroll
        for (int r = 0; r <= 2 * kMaxR; ++r) {
            const int ry = cy + r - kMaxR, kx = g.kx[r];
            lo[r] = 0;
            len[r] = 0;
            if (kx < 0 || ry < 0 || ry >= g.gy) continue;
            const int cl = ry * g.gx + max(cx - kx, 0), ch = ry * g.gx + min(cx + kx, g.gx - 1);
            lo[r] = uniform(cl == 0 ? 0 : (int)cend[cl - 1]);
            len[r] = uniform((int)cend[ch]) - lo[r];
            total += len[r];
        }
        for (int t0 = 0; t0 < total; t0 += 64) {
            int rem = t0 + lane, a = -1;
#pragma unroll
            for (int r = 0; r <= 2 * kMaxR; ++r) {
                if (a < 0) {
                    if (rem < len[r]) a = lo[r] + rem;
                    else rem -= len[r];
                }
            }
            bool fresh = false;
            if (a >= 0) {
                uint32_t d2;
                const uint32_t w = spt[a];
                const bool in = g.narrow ? ecc::epsg::in_eps<true>(v, w, e_int, r2i, &d2)
                                         : ecc::epsg::in_eps<false>(v, w, e_int, r2i, &d2);
                if (in && ((live[a >> 5] >> (a & 31)) & 1u)) {
                    const uint32_t nr = max(c2, d2), old = reach2[a];
                    if (nr < old) {  // undefined (0xffffffff) or larger
                        reach2[a] = nr;
                        fresh = old == kUndef;
                    }
                }
            }
            const uint64_t bal = __ballot(fresh);
            if (fresh) ol[m - 1 - (n_seed + __popcll(bal & ((1ull << lane) - 1ull)))] = (uint16_t)a;
            n_seed += __popcll(bal);
        }
        wave_sync();
    }
}

// K: size of the insertion network, the smallest of 1, 2, 4, ..., 64 that is >= min_pts.
template <int K>
__global__ void __launch_bounds__(kNT)
optics_grid_kernel(const uint32_t *__restrict__ xy, int64_t n_segs, int64_t stride,
                   const int32_t *__restrict__ seg_counts, int e_int, uint32_t r2i, int min_pts, double thr,
                   int32_t *__restrict__ order, double *__restrict__ reach, int32_t *__restrict__ cluster,
                   int32_t *__restrict__ n_clusters) {
    // cend[kCells + 1] | spt[stride] | core2[stride] | reach2[stride] | live[bw] | todo[bw]
    // | sidx[stride] (u16) | ol[stride] (u16)
    extern __shared__ uint32_t lds_o[];
    const int bw = (int)((stride + 31) >> 5);
    uint32_t *cend = lds_o;
    uint32_t *spt = cend + kCells + 1;
    uint32_t *core2 = spt + stride;
    uint32_t *reach2 = core2 + stride;
    uint32_t *live = reach2 + stride;  // bit q: position q not yet emitted
    uint32_t *todo = live + bw;        // bit i: index i not yet emitted
    uint16_t *sidx = reinterpret_cast<uint16_t *>(todo + bw);
    uint16_t *ol = sidx + ((stride + 1) & ~1ll);
    __shared__ int red[64];
    __shared__ int wsum[kNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t s = blockIdx.x; s < n_segs; s += gridDim.x) {
        const int m = ecc::seg_points(seg_counts, stride, s);
        const int64_t base = s * stride;
        const CellGrid g = ecc::epsg::bin_cells(xy, base, m, e_int, r2i, cend, spt, sidx, red, false, true);
        // core distances (:286-299): the (min_pts-1)-th smallest d^2 of the ball, self included
        ecc::epsg::with_narrow(g, [&](auto narrow) {
            constexpr bool kN = decltype(narrow)::value;
            for (int q = tid; q < m; q += kNT) {
                const uint32_t v = spt[q];
                int cnt = 0;
                int best[K];
#pragma unroll
                for (int k = 0; k < K; ++k) best[k] = 0x7fffffff;
                ecc::epsg::for_candidates(g, cend, spt, v, [&](int, uint32_t w, bool ok) {
                    uint32_t d2;
                    const bool in = ecc::epsg::in_eps<kN>(v, w, e_int, r2i, &d2) & ok;
                    cnt += in ? 1 : 0;
                    int val = in ? (int)d2 : 0x7fffffff;  // insertion network: the K smallest, sorted
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int lo2 = min(best[k], val);
                        val = max(best[k], val);
                        best[k] = lo2;
                    }
                });
                uint32_t sel = kUndef;
                if (cnt >= min_pts) {
#pragma unroll
                    for (int k = 0; k < K; ++k) sel = (k == min_pts - 1) ? (uint32_t)best[k] : sel;
                }
                core2[q] = sel;
                reach2[q] = kUndef;
            }
        });
        for (int w = tid; w < bw; w += kNT) {
            const int left = m - w * 32;
            live[w] = todo[w] = left >= 32 ? 0xffffffffu : (left > 0 ? (1u << left) - 1u : 0u);
        }
        __syncthreads();
        if (wave == 0) expand_segment(g, m, bw, e_int, r2i, cend, spt, sidx, core2, reach2, live, todo, ol);
        __syncthreads();
        // threshold clusters (:674-690): a new cluster at every entry with reach < 0 or >= thr
        if (cluster) {  // uniform
            uint32_t fl = 0u;
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int k = tid * kPer + u;
                if (k >= m) continue;
                const uint32_t r2 = reach2[ol[k]];
                fl |= (r2 == kUndef || sqrt((double)r2) >= thr) ? 1u << u : 0u;
            }
            const int cnt = __popc(fl);
            const int inc = ecc::wave_incl_scan(cnt);  // DPP
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            int c = inc - cnt, total = 0;
            for (int w = 0; w < kNT / 64; ++w) {
                c += w < wave ? wsum[w] : 0;
                total += wsum[w];
            }
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int k = tid * kPer + u;
                if (k >= m) continue;
                c += (int)((fl >> u) & 1u);
                cluster[base + k] = c > 0 ? c - 1 : 0;
            }
            if (tid == 0) n_clusters[s] = total;
        }
        for (int k = tid; k < m; k += kNT) {
            const int q = ol[k];
            const uint32_t r2 = reach2[q];
            order[base + k] = sidx[q];
            reach[base + k] = r2 == kUndef ? -1.0 : sqrt((double)r2);  // correctly rounded
        }
        __syncthreads();
    }
}

}  // namespace

ECC_API int ecc_optics_grid(ecc_ctx *ctx, const uint32_t *xy, int64_t n_segs, int64_t seg_stride,
                            const int32_t *seg_counts, double eps, int32_t min_pts, double threshold, int32_t *order,
                            double *reach, int32_t *cluster, int32_t *n_clusters, ecc_stream_t stream) {
    if (!ctx || n_segs < 0 || seg_stride < 1 || seg_stride > kMaxPts || !(eps > 0.0) || eps > 32767.0 || min_pts < 1 ||
        min_pts > 64 || (cluster == nullptr) != (n_clusters == nullptr))
        return ECC_ERR_INVALID;
    if (n_segs > 0 && (!xy || !order || !reach)) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    // d^2 <= eps^2 (fp64) <=> d^2 <= floor(eps^2) for integer d^2; |dx|, |dy| <= floor(eps)
    const int r2i = (int)std::floor(eps * eps), e_int = (int)std::floor(eps);
    using Kern = void (*)(const uint32_t *, int64_t, int64_t, const int32_t *, int, uint32_t, int, double, int32_t *,
                          double *, int32_t *, int32_t *);
    const Kern kern = min_pts <= 1 ? optics_grid_kernel<1> : min_pts <= 2 ? optics_grid_kernel<2>
                    : min_pts <= 4 ? optics_grid_kernel<4> : min_pts <= 8 ? optics_grid_kernel<8>
                    : min_pts <= 16 ? optics_grid_kernel<16> : min_pts <= 32 ? optics_grid_kernel<32>
                    : optics_grid_kernel<64>;
    const size_t lds = optics_lds_bytes(seg_stride);
    static_assert((kCells + 1 + 3 * kMaxPts + 2 * (kMaxPts / 32)) * 4 + kMaxPts * 4 + 64 * 4 + (kNT / 64) * 4 <=
                      160 * 1024,
                  "LDS of optics_grid_kernel at the largest stride");
    if (int rc = ecc::allow_dynamic_lds(ctx, kern, (int)lds, "optics_grid lds")) return rc;
    // one workgroup per segment; beyond 4096 the segments are grid-strided
    const unsigned grid = (unsigned)std::min<int64_t>(n_segs, 4096);
    ECC_TIMED(ctx, s, "optics_grid_kernel");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kNT), lds, s, xy, n_segs, seg_stride, seg_counts, e_int, (uint32_t)r2i,
                       (int)min_pts, threshold, order, reach, cluster, n_clusters);
    ECC_CHECK_LAUNCH(ctx, "optics_grid");
    return ECC_OK;
}

// The member list holds each unprocessed point at most once, so no capacity can overflow.
ECC_API int ecc_optics_grid_status(ecc_ctx *ctx, ecc_stream_t) {
    if (!ctx) return ECC_ERR_INVALID;
    return ECC_OK;
}
