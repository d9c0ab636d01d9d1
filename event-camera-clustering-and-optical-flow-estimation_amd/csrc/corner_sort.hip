// Corner detection, stage 1: the per-slice counting sort by tile (pipeline: corners.hip).
#include "corner_common.hpp"

namespace {

// 1. Per slice, one 1024-lane workgroup: counting sort of the slice's events by tile into the
// slice's own range (keys + group-relative timestamps), the per-slice tile offsets, the
// time-order check (Metavision stream order: t non-decreasing) and, for Q11, the slice's first
// border event.  Slices of <= 16384 events stay in registers (one read); longer ones take a
// counting pass and a placing pass.
// Two 1024-lane workgroups per CU (64 VGPRs: only each event's final key and tile/rank stay in
// registers), so one workgroup's loads overlap the other's LDS phases (one workgroup per CU left
// the CU idle outside its load phase).
#ifndef ECC_SORT_FENCE
#define ECC_SORT_FENCE 4
#endif
constexpr int kSortFence = ECC_SORT_FENCE;  // events whose loads may be in flight together

// Per-slice (slice, pixel) dedup of the keys (groups with 4-byte keys, slices in one chunk, time
// order intact): an arc test reads, per (slice, pixel), only the largest timestamp, i.e. the key
// of the pixel's LAST event in the slice; pair_build takes the maximum of what it receives.  The
// slice's events are taken in kSortEPT rounds from the last (round u = events [1024 u, 1024 u +
// 1024)): an event is dropped when a LATER round already set its tile pixel's bit in an LDS
// bitmap (the staging area, not yet in use).  Events of one round at one pixel all stay (no
// ordering inside a round), so the maximum always survives.  ~46 % of the events remain on the
// bench's stream (40 % are distinct (slice, pixel) pairs), and pair_build reads only those.
#ifndef ECC_SORT_DEDUP_STEP
#define ECC_SORT_DEDUP_STEP 1  // event slots per dedup round (a divisor of kSortEPT)
#endif
constexpr int kSortDedupStep = ECC_SORT_DEDUP_STEP;
#ifndef ECC_SORT_DEDUP
#define ECC_SORT_DEDUP 1
#endif

// Block-wide exclusive scan in place of a[0, n) (kSortThreads threads, each a contiguous run);
// returns the total to every thread.
__device__ __forceinline__ int block_excl_scan_inplace(int32_t *a, int n, int32_t *wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (n + kSortThreads - 1) / kSortThreads;
    const int b0 = min(n, tid * per), b1 = min(n, b0 + per);
    int sum = 0;
    for (int i = b0; i < b1; ++i) sum += a[i];
    const int incl = ecc::wave_incl_scan(sum);  // DPP
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int run = incl - sum, total = 0;
    for (int w = 0; w < kSortThreads / 64; ++w) {
        run += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    for (int i = b0; i < b1; ++i) {
        const int c = a[i];
        a[i] = run;
        run += c;
    }
    return total;
}

template <bool kBorder>  // border_mode 1: the slice's first border event is wanted
__global__ void __launch_bounds__(kSortThreads, 8)  // 8 waves/SIMD: two workgroups per CU
slice_sort_kernel(const uint32_t *__restrict__ xy, const int64_t *__restrict__ t, CornerGeom g, Sorted so,
                  int32_t *__restrict__ first_border, int32_t *__restrict__ err, int32_t tag,
                  uint32_t *__restrict__ zero0, int32_t *__restrict__ zero1, GroupRec *__restrict__ grec) {
    extern __shared__ int32_t hist[];  // [nb + kSortSent]: counts, then offsets, then (long slices) cursors;
                                       // then [kSortChunk] staging (single slices: the keys in
                                       // event order, then in tile order); then the dedup bitmap
    __shared__ int32_t wsum[kSortThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t s = blockIdx.x;
    // the call's counters that later kernels of the call start from (a 4-B memset each was a
    // fill launch on the critical path): arc_kernel's overflow count, the NMS error word.  The
    // sort verdict needs no reset: a workgroup that sees decreasing time writes this call's tag.
    if (s == 0 && tid == 0) {
        if (zero0) *zero0 = 0u;
        if (zero1) *zero1 = 0;
    }
    const int64_t lo = s * g.S;
    const int len = (int)((lo + g.S < g.n ? lo + g.S : g.n) - lo);
    const int64_t grp = s / kGroup;
    const int64_t grp_first = grp * kGroup * (int64_t)g.S;
    // the group's record for the later kernels of the call (rewritten by every sort phase)
    if (s % kGroup == 0 && tid == 0) group_rec_store(t, g, grp, grec);
    int64_t t_first;
    const bool narrow = group_narrow(t, g, grp, &t_first);  // uniform
    const bool fmt4 = group_fmt4(t, g, grp);                // uniform
    const int nb = g.n_tiles + 1;
    const bool single = len <= kSortChunk;
    const bool dedup = ECC_SORT_DEDUP && single && fmt4 && g.dedup_words > 0;  // uniform
    const int nbs = nb + kSortSent;
    const uint32_t sent = (uint32_t)(nb + (lane & (kSortSent - 1))) << 16;  // this lane's sentinel bin
    uint32_t *stage = reinterpret_cast<uint32_t *>(hist + nbs);
    uint32_t *bm = stage + kSortChunk;  // the dedup bitmap
    for (int b = tid; b < nbs; b += kSortThreads) hist[b] = 0;
    if (dedup)
        for (int w = tid; w < g.dedup_words; w += kSortThreads) bm[w] = 0u;
    __syncthreads();
    bool bad = false;
    int fb = 0x7fffffff;
    // per event only tile << 16 | rank stays in registers (single slices: rank < 2^14); the key,
    // formed at load time, waits in the staging area in event order (in registers, it held 16
    // VGPRs through the load phase)
    uint32_t br[kSortEPT];
    const uint32_t *__restrict__ xs = xy + lo;
    const int64_t *__restrict__ ts = t + lo;
    for (int c0 = 0; c0 < len; c0 += kSortChunk) {  // one iteration for single slices
#pragma unroll
        for (int u = 0; u < kSortEPT; ++u) {
            // a compiler fence every kSortFence events keeps later loads from being hoisted above
            // earlier uses (all 16 events' loads in flight would spill)
            if (u > 0 && u % kSortFence == 0) asm volatile("" ::: "memory");
            const int i = c0 + u * kSortThreads + tid;
            const bool ok = i < len;
            const int ic = ok ? i : len - 1;  // clamped: unconditional loads off uniform bases
            const uint32_t v = xs[ic];
            const int64_t tc = ts[ic];
            // the previous event's t: a coalesced load of the neighbouring element (cache hit).  A
            // clamped slot repeats the check of the slice's last event, so the verdict needs no
            // `ok`: no per-slot mask pair is kept alive.
            const int64_t tp = (ic > 0 || lo > 0) ? ts[ic - 1] : INT64_MIN;
            bad |= tp > tc;
            if (single) stage[u * kSortThreads + tid] = tile_key(v, fmt4 ? (uint32_t)(tc - t_first) : (uint32_t)(lo + i - grp_first));
            br[u] = ok ? (uint32_t)tile_of(v, g) << 16 : sent;
            if (kBorder && ok && is_border(ecc::xy_x(v), ecc::xy_y(v), g)) fb = min(fb, i);
        }
        if (dedup && !__syncthreads_or(bad)) {  // uniform (single slices: one pass of this loop)
            // rounds of kSortDedupStep event slots, latest first: an event is dropped when a later
            // round already holds its (slice, pixel); events of one round are not compared with
            // each other (pair_build's atomicMax keeps the last of what remains)
#pragma unroll
            for (int u0 = kSortEPT - 1; u0 >= 0; u0 -= kSortDedupStep) {
                bool drop[kSortDedupStep];
                uint32_t tp[kSortDedupStep];
                bool cand[kSortDedupStep];
#pragma unroll
                for (int d = 0; d < kSortDedupStep; ++d) {
                    const int u = u0 - d;
                    const uint32_t b = br[u] >> 16;  // > n_tiles: no event; n_tiles: outside the sensor (kept)
                    cand[d] = b < (uint32_t)g.n_tiles;
                    tp[d] = b * kTilePix + (stage[u * kSortThreads + tid] & 255u);  // own key
                    drop[d] = u0 < kSortEPT - 1 && cand[d] && ((bm[tp[d] >> 5] >> (tp[d] & 31u)) & 1u);
                }
                if (u0 < kSortEPT - 1) __syncthreads();  // every check of the round before its bits are set
#pragma unroll
                for (int d = 0; d < kSortDedupStep; ++d) {
                    if (drop[d]) br[u0 - d] = sent;
                    else if (cand[d]) atomicOr(&bm[tp[d] >> 5], 1u << (tp[d] & 31u));
                }
                if (u0 - kSortDedupStep >= 0) __syncthreads();  // the round's bits before the next checks
            }
        }
#pragma unroll
        for (int u = 0; u < kSortEPT; ++u) br[u] |= (uint32_t)atomicAdd(&hist[br[u] >> 16], 1) & 0xffffu;
    }
    if (__any(bad) && lane == 0 && !g.any_order) *err = tag;  // pending: published by sae_prefix_kernel
    if (kBorder) {  // (border_mode 0: the flag pass does not read first_border)
        fb = ecc::wave_min_i32(fb);  // DPP
        if (lane == 0) wsum[tid >> 6] = fb;
        __syncthreads();
        if (tid == 0) {
            int m = 0x7fffffff;
            for (int w = 0; w < kSortThreads / 64; ++w) m = min(m, wsum[w]);
            first_border[s] = m;
        }
    }
    __syncthreads();
    block_excl_scan_inplace(hist, nbs, wsum);
    __syncthreads();
    const int kept = hist[nb];  // the first sentinel bin's offset: len, less the dropped events
    int32_t *row = so.toff + s * (int64_t)(nb + 1);
    for (int b = tid; b < nb; b += kSortThreads) row[b] = hist[b];
    if (tid == 0) row[nb] = kept;
    if (single) {  // place keys, then timestamps, in tile order in LDS; write both out contiguously
        uint32_t kv[kSortEPT];
#pragma unroll
        for (int u = 0; u < kSortEPT; ++u) kv[u] = stage[u * kSortThreads + tid];  // own keys
        __syncthreads();  // every key read before the stage is permuted
#pragma unroll
        for (int u = 0; u < kSortEPT; ++u) stage[hist[br[u] >> 16] + (br[u] & 0xffffu)] = kv[u];
        __syncthreads();
        for (int i = tid; i < kept; i += kSortThreads) so.key[lo + i] = stage[i];
        if (fmt4 || !narrow) return;  // (no dedup below: kept == len)
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kSortEPT; ++u)  // rare (groups spanning >= 2^24 ticks): t read again (clamped)
            stage[hist[br[u] >> 16] + (br[u] & 0xffffu)] = (uint32_t)(t[lo + min(u * kSortThreads + tid, len - 1)] - t_first);
        __syncthreads();
        for (int i = tid; i < len; i += kSortThreads) so.t32[lo + i] = stage[i];
        return;
    }
    __syncthreads();  // row written before the offsets turn into cursors
    for (int c0 = 0; c0 < len; c0 += kSortThreads) {
        const int i = c0 + tid;
        if (i >= len) continue;
        const uint32_t vv = xy[lo + i];
        const int64_t pos = lo + atomicAdd(&hist[tile_of(vv, g)], 1);
        if (fmt4) {
            so.key[pos] = tile_key(vv, (uint32_t)(t[lo + i] - t_first));
        } else {
            so.key[pos] = tile_key(vv, (uint32_t)(lo + i - grp_first));
            if (narrow) so.t32[pos] = (uint32_t)(t[lo + i] - t_first);
        }
    }
}

}  // namespace

int ecc::corner::launch_sort(ecc_ctx *ctx, hipStream_t s, const uint32_t *xy, const int64_t *t, const CornerGeom &g,
                             const Sorted &so, int32_t *first_border, int32_t tag, uint32_t *zero0, int32_t *zero1,
                             GroupRec *grec) {
    // > 64 KiB: opt in (gfx950 has 160 KiB); the dedup bitmap only while two workgroups fit a CU
    const int nb = g.n_tiles + 1;
    const size_t lds = ((size_t)nb + kSortSent + kSortChunk + g.dedup_words) * 4;
    constexpr int kLdsCap = (kMaxTiles + 1 + kSortSent + kSortChunk) * 4;
    const auto kern = g.border_mode == 1 ? &slice_sort_kernel<true> : &slice_sort_kernel<false>;
    if (int rc = ecc::allow_dynamic_lds(ctx, kern, kLdsCap, "slice_sort LDS")) return rc;
    ECC_TIMED(ctx, s, "slice_sort_kernel");
    hipLaunchKernelGGL(kern, dim3((unsigned)g.n_slices), dim3(kSortThreads), lds, s, xy, t, g, so, first_border,
                       &ctx->dev->sort_pending, tag, zero0, zero1, grec);
    return ECC_OK;
}
