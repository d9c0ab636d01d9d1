// Corner detection, stage 6: the corner flags in event order, and for the fused detect + NMS
// calls each slice's NMS candidate list (pipeline: corners.hip).
#include "corner_common.hpp"
#include "flag_decode.hpp"

namespace {

// 6. Corner flags in event order: one workgroup per slice.  Event i of slice s (group g, slice j
// of the group) is a corner iff its (slice, pixel) pair's bit is set in the result words of its
// (g, tile) item.  The workgroup first stages slice j's 196-bit segment of every tile's result
// vector in LDS (7 words per tile), so each event's lookup is an LDS read (word and bit from
// flag_decode.hpp, for every event alike: no branch and no wait per event); every flag is then
// written, 0 or 1, four per lane and store.  The per-event eligibility of the reference loop: the
// first-detect rule (Q15) and, in ref_compat mode (Q11), "before the slice's first border event";
// corner pairs are never border pixels.
#ifndef ECC_FLAG_THREADS
#define ECC_FLAG_THREADS 256
#endif
constexpr int kFlagThreads = ECC_FLAG_THREADS;  // 256: every slice's workgroup resident at once (5 per CU)
#ifndef ECC_FLAG_QUADS
#define ECC_FLAG_QUADS 8
#endif
constexpr int kFlagQuads = ECC_FLAG_QUADS;  // 4-event quads a lane has in flight per batch
constexpr int kFlagBatch = kFlagQuads * kFlagThreads;  // quads per batch

// Quads whose LDS reads are issued together, before the first of them is consumed (all 8 of a
// batch would take 124 VGPRs: four workgroups per CU, and the slices no longer resident at once).
#ifndef ECC_FLAG_GROUP
#define ECC_FLAG_GROUP 4
#endif
constexpr int kFlagGroup = ECC_FLAG_GROUP;
static_assert(kFlagQuads % kFlagGroup == 0, "a batch is whole read groups");
static_assert(kFlagTile == (uint32_t)kTile && kFlagSegWords == (uint32_t)kSegWords, "flag_decode.hpp's tile");

// kStaged: word `w` of the slice's result segments from LDS; otherwise (sensors whose segments
// exceed the LDS) straight from the group's result words.  w <= last_word: inside both.
template <bool kStaged>
__device__ __forceinline__ uint32_t seg_word(uint32_t w, const uint32_t *sb, const uint32_t *__restrict__ rg) {
    return kStaged ? sb[w] : rg[w];
}

// One event's flag (the scalar tails).  Nothing is under a branch: the word index is clamped
// (flag_slot), and an event off the sensor masks the bit it read.
template <bool kStaged>
__device__ __forceinline__ uint32_t corner_bit(uint32_t v, const CornerGeom &g, uint32_t last_word, const uint32_t *sb,
                                               const uint32_t *__restrict__ rg) {
    const uint32_t x = (uint32_t)ecc::xy_x(v), y = (uint32_t)ecc::xy_y(v);
    const FlagSlot sl = flag_slot(x, y, (uint32_t)g.tiles_x, last_word);
    return (seg_word<kStaged>(sl.word, sb, rg) >> sl.bit) & flag_on_sensor(x, y, (uint32_t)g.W, (uint32_t)g.H);
}

// 0x01 in byte k for k < r (r of any sign): the events of a quad before an end r events away
__device__ __forceinline__ uint32_t first_bytes(int r) {
    const int rc = min(max(r, 0), 4);
    return rc >= 4 ? 0x01010101u : (0x01010101u & ((1u << (8 * (rc & 3))) - 1u));
}

// kCand (ecc_fast_detect_nms): the pass also writes each slice's NMS candidate list — the
// flagged events' xy in event order at cand[s * S ...], their count in n_cand[s] — which is
// what nms_compact_kernel would rebuild from the flags (the host takes this form only for
// slices of at most kFlagCandMax events, a multiple of 4, with 4-B aligned flags: every slice then
// runs in quads).
// 256-lane workgroups, one per slice, so that all 1221 slices of the bench batch are resident at
// once (five per CU at the kernel's 90 VGPRs, which 1221 / 256 = 4.8 needs; 512-lane ones left a
// second round of 197 workgroups as a tail).  A slice's
// quads are taken in batches of kFlagQuads per lane: the first batch's loads are issued before
// the staging of the result segments, so the two latencies overlap.
template <bool kStaged, bool kCand>
__global__ void __launch_bounds__(kFlagThreads)
flags_event_kernel(const uint32_t *__restrict__ xy, CornerGeom g, const uint32_t *__restrict__ res,
                   const int32_t *__restrict__ first_border, uint8_t *__restrict__ flags, uint32_t *__restrict__ cand,
                   int32_t *__restrict__ n_cand) {
    extern __shared__ uint32_t sb[];  // [n_tiles][kSegWords]: bit lp of tile = pair (j, lp)
    __shared__ int ctot[kFlagQuads][kFlagThreads / 64];
    const int64_t s = blockIdx.x;
    const int64_t lo = s * g.S;
    const int len = (int)((lo + g.S < g.n ? lo + g.S : g.n) - lo);
    const uint32_t last_word = (uint32_t)(g.n_tiles * kSegWords - 1);  // of the slice's segments
    // events [0, live_end) of the slice can be corners
    const int live_end = s < g.first_detect ? 0 : (g.border_mode == 1 ? min(len, max(first_border[s], 0)) : len);
    const uint32_t *rg = res + s * g.seg_stride;  // slice s's segment of every tile (16-B aligned)
    // 4-event quads (16-B loads through the view, which need 4 B; 4-B flag stores, taken by the
    // store's ADDRESS: the slice's first event plus the flags pointer's own offset)
    const bool vec = ((lo + (int64_t)(reinterpret_cast<uintptr_t>(flags) & 3)) & 3) == 0;  // uniform
    const int n4 = vec ? len / 4 : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // all loads unconditional through a buffer view of the slice's whole quads (0 past them): a
    // load under a per-lane condition made each quad wait for the previous one
    const __amdgpu_buffer_rsrc_t vq = ecc::buffer_view(xy + lo, (uint32_t)n4 * 16u);
    uint4 pre[kFlagQuads];
    auto load_batch = [&](int q0) {
#pragma unroll
        for (int u = 0; u < kFlagQuads; ++u)
            pre[u] = ecc::buffer_load_u128(vq, threadIdx.x * 16u, (uint32_t)(q0 + u * kFlagThreads) * 16u);
        __builtin_amdgcn_sched_barrier(0);
    };
    load_batch(0);
    if (kStaged && live_end > 0) {
        // the slice's words of every tile are one contiguous run: 16-B loads, four per lane per
        // trip, unconditional through a buffer view (0 past the run)
        const int total = g.n_tiles * kSegWords;
        const __amdgpu_buffer_rsrc_t vr = ecc::buffer_view(rg, (uint32_t)total * 4u);
        for (int k0 = 0; k0 < total; k0 += 16 * kFlagThreads) {
            uint4 a[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) a[b] = ecc::buffer_load_u128(vr, (uint32_t)(k0 + 4 * (b * kFlagThreads + (int)threadIdx.x)) * 4u);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = k0 + 4 * (b * kFlagThreads + (int)threadIdx.x);
                if (k + 3 < total) {
                    *reinterpret_cast<uint4 *>(sb + k) = a[b];
                } else {
                    if (k < total) sb[k] = a[b].x;
                    if (k + 1 < total) sb[k + 1] = a[b].y;
                    if (k + 2 < total) sb[k + 2] = a[b].z;
                }
            }
        }
    }
    __syncthreads();
    // No event is under a branch.  Every slot of a batch is decoded and looked up, whatever it
    // holds: a quad past the slice's quads loads zeros (pixel (0, 0): in bounds), an event off the
    // sensor reads a clamped word; what must not count is masked out of the packed quad word
    // afterwards: the on-sensor bytes, and the bytes before `live_q` (live_end, held to the
    // slice's whole quads).  The flag store goes through a buffer view of the slice's whole quads
    // (dropped past them; when `vec`, flags + lo is 4-B aligned).  A read group's LDS reads are
    // all issued before the first is consumed.
    const int live_q = min(live_end, 4 * n4);
    const __amdgpu_buffer_rsrc_t vf = ecc::buffer_view(flags + lo, (uint32_t)n4 * 4u);
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int base = 0;  // candidates written so far (uniform)
    uint32_t *dst = cand + lo;
    for (int q0 = 0; q0 < n4; q0 += kFlagBatch) {  // uniform
        if (q0 > 0) load_batch(q0);
        uint32_t f[kFlagQuads];
        int pfx[kFlagQuads];
#pragma unroll
        for (int u0 = 0; u0 < kFlagQuads; u0 += kFlagGroup) {
            uint32_t wd[kFlagGroup][4], sh[kFlagGroup], ok[kFlagGroup];  // words; bit numbers, on-sensor: a byte each
#pragma unroll
            for (int u = 0; u < kFlagGroup; ++u) {
                const uint32_t ev[4] = {pre[u0 + u].x, pre[u0 + u].y, pre[u0 + u].z, pre[u0 + u].w};
                sh[u] = ok[u] = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t x = (uint32_t)ecc::xy_x(ev[k]), y = (uint32_t)ecc::xy_y(ev[k]);
                    const FlagSlot sl = flag_slot(x, y, (uint32_t)g.tiles_x, last_word);
                    wd[u][k] = seg_word<kStaged>(sl.word, sb, rg);
                    sh[u] |= sl.bit << (8 * k);
                    ok[u] |= flag_on_sensor(x, y, (uint32_t)g.W, (uint32_t)g.H) << (8 * k);
                }
            }
#pragma unroll
            for (int u = 0; u < kFlagGroup; ++u) {
                const int i = 4 * (q0 + (u0 + u) * kFlagThreads + (int)threadIdx.x);
                uint32_t bits = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) bits |= ((wd[u][k] >> ((sh[u] >> (8 * k)) & 31u)) & 1u) << (8 * k);
                f[u0 + u] = bits & ok[u] & first_bytes(live_q - i);
                ecc::buffer_store_u32(f[u0 + u], vf, threadIdx.x * 4u, (uint32_t)(q0 + (u0 + u) * kFlagThreads) * 4u);
            }
        }
#pragma unroll
        for (int u = 0; u < kFlagQuads; ++u) {
            if constexpr (kCand) {
                // quad u of lane tid holds events 4 (q0 + u * T + tid) .. + 3: event order is u,
                // then lane; a quad has <= 4 flags, so three ballots give each lane its prefix
                const int c = __popc(f[u]);  // flag bytes are 0 or 1
                const uint64_t b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
                pfx[u] = __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
                if (lane == 0) ctot[u][wave] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
            }
        }
        if constexpr (kCand) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kFlagQuads; ++u) {
                int off = base + pfx[u];
#pragma unroll
                for (int w = 0; w < kFlagThreads / 64; ++w) {
                    const int tw = ctot[u][w];
                    off += w < wave ? tw : 0;
                    base += tw;
                }
                if (f[u]) {
                    if (f[u] & 0x1u) dst[off++] = pre[u].x;
                    if (f[u] & 0x100u) dst[off++] = pre[u].y;
                    if (f[u] & 0x10000u) dst[off++] = pre[u].z;
                    if (f[u] & 0x1000000u) dst[off++] = pre[u].w;
                }
            }
            __syncthreads();  // ctot is rewritten by the next batch
        }
    }
    if constexpr (kCand) {
        if (threadIdx.x == 0) {
            for (int i = 4 * n4; i < len; ++i) {  // the batch's last < 4 events, in order
                const uint32_t v = xy[lo + i];
                const uint32_t fb = corner_bit<kStaged>(v, g, last_word, sb, rg) & (i < live_end ? 1u : 0u);
                flags[lo + i] = (uint8_t)fb;
                if (fb) dst[base++] = v;
            }
            n_cand[s] = base;
        }
    } else {
        for (int i = 4 * n4 + threadIdx.x; i < len; i += kFlagThreads)  // last < 4 events, or unaligned slices
            flags[lo + i] = (uint8_t)(corner_bit<kStaged>(xy[lo + i], g, last_word, sb, rg) & (i < live_end ? 1u : 0u));
    }
}

}  // namespace

int ecc::corner::launch_flags(ecc_ctx *ctx, hipStream_t s, const uint32_t *xy, const CornerGeom &g, const GroupImages &gi,
                              const int32_t *first_border, uint8_t *corner_flags, uint32_t *cand, int32_t *n_cand) {
    ECC_TIMED(ctx, s, "flags_kernel");
    constexpr size_t kLdsMax = kFlagDynLdsMax;
    const size_t lds = (size_t)g.n_tiles * kSegWords * sizeof(uint32_t);
    if (lds <= kLdsMax) {
        const auto fn = cand ? &flags_event_kernel<true, true> : &flags_event_kernel<true, false>;
        if (lds > 65536)
            if (int rc = ecc::allow_dynamic_lds(ctx, fn, (int)kLdsMax, "flags LDS")) return rc;
        if (cand)
            hipLaunchKernelGGL((flags_event_kernel<true, true>), dim3((unsigned)g.n_slices), dim3(kFlagThreads), lds, s,
                               xy, g, (const uint32_t *)gi.res, first_border, corner_flags, cand, n_cand);
        else
            hipLaunchKernelGGL((flags_event_kernel<true, false>), dim3((unsigned)g.n_slices), dim3(kFlagThreads), lds,
                               s, xy, g, (const uint32_t *)gi.res, first_border, corner_flags, nullptr, nullptr);
    } else {
        if (cand) return ECC_ERR_INVALID;  // the caller checks ecc_fast_detect_nms' conditions
        hipLaunchKernelGGL((flags_event_kernel<false, false>), dim3((unsigned)g.n_slices), dim3(kFlagThreads), 0, s,
                           xy, g, (const uint32_t *)gi.res, first_border, corner_flags, nullptr, nullptr);
    }
    return ECC_OK;
}
