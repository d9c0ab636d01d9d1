// Corner detection, stage 6: the corner flags in event order, and for the fused detect + NMS
// calls each slice's NMS candidate list (pipeline: corners.hip).
#include "corner_common.hpp"
#include "flag_decode.hpp"
#include "flag_raster.hpp"

namespace {

// 6. Corner flags in event order: one workgroup per slice.  Event i of slice s (group g, slice j
// of the group) is a corner iff its (slice, pixel) pair's bit is set in the result words of its
// (g, tile) item.  The flag depends on (slice, x, y) alone, so the workgroup first turns slice j's
// 196-bit segment of every tile's result vector (7 words per tile) into a raster bitmap of the
// sensor in LDS, bit y * W + x (flag_raster.hpp): the tile arithmetic runs once per corner pixel
// of the slice, and each event's lookup is a multiply-add, a clamp and an LDS read, for every
// event alike (no branch and no wait per event); every flag is then
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

// Quads whose LDS reads are issued together, before the first of them is consumed (all 8 of an
// unpipelined batch take 117 VGPRs: four workgroups per CU, the slices no longer resident at
// once, and the kernel 3 us slower; a pipelined batch is 4 quads, one read group).
#ifndef ECC_FLAG_GROUP
#define ECC_FLAG_GROUP 4
#endif
constexpr int kFlagGroup = ECC_FLAG_GROUP;
static_assert(kFlagQuads % kFlagGroup == 0, "a batch is whole read groups");
// 1: the staged variants look events up in a raster bitmap of the slice's corners; 0: in the tile
// segments themselves, copied to LDS (flag_slot per event, as the unstaged variant always does).
#ifndef ECC_FLAG_RASTER
#define ECC_FLAG_RASTER 1
#endif
constexpr bool kFlagRaster = ECC_FLAG_RASTER != 0;
// 1: a lane's candidate ranks from one DPP scan of its quad counts, packed two to a word; 0: from
// three ballots and six 64-bit bit counts per quad.
#ifndef ECC_FLAG_SCAN
#define ECC_FLAG_SCAN 1
#endif
constexpr bool kFlagScan = ECC_FLAG_SCAN != 0;
// 1: the staged variants take a batch in two halves with a register buffer each, the loads of a
// half in flight while the other is decoded, ranked and written out; 0: one buffer, each batch
// loaded when the one before it is finished.
#ifndef ECC_FLAG_PIPE
#define ECC_FLAG_PIPE 1
#endif
constexpr bool kFlagPipe = ECC_FLAG_PIPE != 0;
static_assert(kFlagQuads % 2 == 0, "the quad counts are packed in pairs");
constexpr int kFlagWaves = kFlagThreads / 64;
constexpr int kFlagTotWords = kFlagScan ? 2 * kFlagWaves * (kFlagQuads / 2) : kFlagQuads * kFlagWaves;
static_assert(kFlagTotWords * 4 + 4 <= 160 * 1024 - (int)kFlagDynLdsMax, "the static LDS kFlagDynLdsMax leaves room for");

// Dynamic LDS of the staged variants, in words.  Raster form: the bitmap (never more than the
// tile segments' n_tiles * 7 words, flag_raster.hpp) and behind it the list of the segments'
// non-zero words that the staging pass collects, in what the segments' size leaves over plus, where
// the limit allows, kFlagListExtra words (a list entry is 6 B; a word that finds the list full is
// rastered by the lane that loaded it).
constexpr uint32_t kFlagListExtra = 384;
__host__ __device__ inline uint32_t flag_lds_words(uint32_t n_tiles) {
    const uint32_t seg = n_tiles * (uint32_t)kSegWords;
    if (!kFlagRaster) return seg;
    const uint32_t most = (uint32_t)(kFlagDynLdsMax / 4), want = ((seg + 3u) & ~3u) + kFlagListExtra;
    return want < most ? want : most;
}
static_assert(kFlagTile == (uint32_t)kTile && kFlagSegWords == (uint32_t)kSegWords, "flag_decode.hpp's tile");

// kStaged: word `w` of the slice's result segments from LDS; otherwise (sensors whose segments
// exceed the LDS) straight from the group's result words.  w <= last_word: inside both.
template <bool kStaged>
__device__ __forceinline__ uint32_t seg_word(uint32_t w, const uint32_t *sb, const uint32_t *__restrict__ rg) {
    return kStaged ? sb[w] : rg[w];
}

// An event's word and bit.  kRaster: of the raster bitmap (`last` = its last bit, W * H - 1);
// otherwise of the slice's result segments (`last` = their last word).  Clamped either way.
template <bool kRaster>
__device__ __forceinline__ FlagSlot flag_look(uint32_t x, uint32_t y, const CornerGeom &g, uint32_t last) {
    if constexpr (kRaster) {
        const uint32_t idx = flag_raster_index(x, y, (uint32_t)g.W, last);
        return FlagSlot{idx >> 5, idx & 31u};
    } else {
        return flag_slot(x, y, (uint32_t)g.tiles_x, last);
    }
}

// One event's flag (the scalar tails).  Nothing is under a branch: the index is clamped
// (flag_look), and an event off the sensor masks the bit it read.
template <bool kStaged>
__device__ __forceinline__ uint32_t corner_bit(uint32_t v, const CornerGeom &g, uint32_t last, const uint32_t *sb,
                                               const uint32_t *__restrict__ rg) {
    const uint32_t x = (uint32_t)ecc::xy_x(v), y = (uint32_t)ecc::xy_y(v);
    const FlagSlot sl = flag_look<kStaged && kFlagRaster>(x, y, g, last);
    return (seg_word<kStaged>(sl.word, sb, rg) >> sl.bit) & flag_on_sensor(x, y, (uint32_t)g.W, (uint32_t)g.H);
}

// Staging, raster form: ORs the pixels of the set bits of `w`, word `i` of the slice's
// [n_tiles][kSegWords] run, into the raster bitmap `sb` (LDS atomics: raster neighbours belong to
// different tiles, hence to different lanes).  A loop over the set bits: they are rare.
__device__ __forceinline__ void raster_or_word(uint32_t *sb, uint32_t i, uint32_t w, const CornerGeom &g) {
    const FlagStageWord sw = flag_stage_word(i, (uint32_t)g.tiles_x, g.tx_mul, g.tx_sh);
    while (w) {
        const uint32_t b = (uint32_t)__builtin_ctz(w);
        w &= w - 1u;
        const FlagStagePixel px = flag_stage_pixel(sw, b, (uint32_t)g.W, (uint32_t)g.H);
        if (px.set) {
            const uint32_t idx = __umul24(px.y, (uint32_t)g.W) + px.x;  // < W * H
            atomicOr(sb + (idx >> 5), 1u << (idx & 31u));
        }
    }
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
// once (five per CU at the kernel's 80 VGPRs, which 1221 / 256 = 4.8 needs; 512-lane ones left a
// second round of 197 workgroups as a tail).  A slice's
// quads are taken in batches (kFlagQuads per lane, or half that with the next half loading):
// the first batch's loads are issued before the staging of the result segments, so the two
// latencies overlap.
template <bool kStaged, bool kCand>
__global__ void __launch_bounds__(kFlagThreads)
flags_event_kernel(const uint32_t *__restrict__ xy, CornerGeom g, const uint32_t *__restrict__ res,
                   const int32_t *__restrict__ first_border, uint8_t *__restrict__ flags, uint32_t *__restrict__ cand,
                   int32_t *__restrict__ n_cand) {
    constexpr bool kRaster = kStaged && kFlagRaster;
    // kRaster: bit y * W + x = pixel (x, y) is a corner of slice j, then the staging list;
    // otherwise [n_tiles][kSegWords]: bit lp of tile = pair (j, lp)
    extern __shared__ uint32_t sb[];
    __shared__ uint32_t ctot[kFlagTotWords];  // the waves' candidate counts of a batch
    __shared__ uint32_t n_list;               // non-zero segment words the staging pass met
    const int64_t s = blockIdx.x;
    const int64_t lo = s * g.S;
    const int len = (int)((lo + g.S < g.n ? lo + g.S : g.n) - lo);
    // the lookups' clamp: the raster's last bit, or the last word of the slice's segments
    const uint32_t last = kRaster ? (uint32_t)(g.W * g.H - 1) : (uint32_t)(g.n_tiles * kSegWords - 1);
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
    // kPipe: the lane's kFlagQuads quad registers are two halves, `pre` the half batch being
    // worked on and `nxt` the one after it, whose loads are in flight meanwhile (a batch past
    // the slice loads zeros).  A batch starts by moving `nxt` to `pre`: the one wait for loads
    // issued a whole batch earlier, where the compiler can count (with the two halves as
    // alternating buffers of a loop unrolled twice it waited for the loads it had just issued).
    constexpr bool kPipe = kStaged && kFlagPipe;
    constexpr int kQ = kPipe ? kFlagQuads / 2 : kFlagQuads;  // quads of a lane per batch
    constexpr int kBatch = kQ * kFlagThreads;
    static_assert(kQ % kFlagGroup == 0 && kQ % 2 == 0, "a batch is whole read groups and whole pairs");
    uint4 pre[kQ], nxt[kPipe ? kQ : 1];
    auto load_batch = [&](uint4(&to)[kQ], int q0) {
#pragma unroll
        for (int u = 0; u < kQ; ++u)
            to[u] = ecc::buffer_load_u128(vq, threadIdx.x * 16u, (uint32_t)(q0 + u * kFlagThreads) * 16u);
        __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (kPipe)
        load_batch(reinterpret_cast<uint4(&)[kQ]>(nxt), 0);
    else
        load_batch(pre, 0);
    if (kStaged && live_end > 0) {
        // the slice's words of every tile are one contiguous run: 16-B loads, four per lane per
        // trip, unconditional through a buffer view (0 past the run)
        const int total = g.n_tiles * kSegWords;
        const __amdgpu_buffer_rsrc_t vr = ecc::buffer_view(rg, (uint32_t)total * 4u);
        // raster form: the bitmap zeroed (whole 16 B: inside the LDS by flag_lds_words), then the
        // list of the run's non-zero words behind it, 4-B words and 2-B indices (below 2^16:
        // kMaxTiles * kSegWords)
        const uint32_t ras4 = (flag_raster_words((uint32_t)g.W, (uint32_t)g.H) + 3u) & ~3u;
        const uint32_t cap = kRaster ? (flag_lds_words((uint32_t)g.n_tiles) - ras4) * 4u / 6u : 0u;
        uint32_t *const list_w = sb + ras4;
        uint16_t *const list_i = reinterpret_cast<uint16_t *>(list_w + cap);
        if constexpr (kRaster) {
            for (uint32_t k = 4u * threadIdx.x; k < ras4; k += 4u * kFlagThreads)
                *reinterpret_cast<uint4 *>(sb + k) = make_uint4(0u, 0u, 0u, 0u);
            if (threadIdx.x == 0) n_list = 0u;
            __syncthreads();
        }
        for (int k0 = 0; k0 < total; k0 += 16 * kFlagThreads) {
            uint4 a[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) a[b] = ecc::buffer_load_u128(vr, (uint32_t)(k0 + 4 * (b * kFlagThreads + (int)threadIdx.x)) * 4u);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (kRaster) {
                // Words past the run load as 0, like the many without a corner: a word costs its
                // test.  The non-zero ones are spread thinly over the lanes, so they are first
                // collected (a wave's places from one scan and one atomic) and then rastered one
                // per lane, instead of every wave looping over the bits of each of its 16 slots.
                uint32_t nz = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    nz += (a[b].x != 0u) + (a[b].y != 0u) + (a[b].z != 0u) + (a[b].w != 0u);
                const uint32_t incl = (uint32_t)ecc::wave_incl_scan((int)nz);
                uint32_t first = 0u;
                if (lane == 63 && incl) first = atomicAdd(&n_list, incl);
                const uint32_t pos0 = (uint32_t)ecc::lane_value((int)first, 63) + incl - nz;
                uint32_t pos = pos0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t k = (uint32_t)(k0 + 4 * (b * kFlagThreads + (int)threadIdx.x));
                    const uint32_t wv[4] = {a[b].x, a[b].y, a[b].z, a[b].w};
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c)
                        if (wv[c]) {
                            if (pos < cap) {
                                list_w[pos] = wv[c];
                                list_i[pos] = (uint16_t)(k + c);
                            }
                            ++pos;
                        }
                }
                if (pos > cap) {
                    // the list is full (a slice with thousands of corner pixels, or a sensor whose
                    // segments leave it no room): this lane rasters the words it could not place,
                    // read again, in one rolled loop
                    pos = pos0;
#pragma unroll 1
                    for (uint32_t e = 0; e < 16u; ++e) {
                        const uint32_t k = (uint32_t)k0 + 4u * ((e >> 2) * kFlagThreads + threadIdx.x) + (e & 3u);
                        const uint32_t w = k < (uint32_t)total ? rg[k] : 0u;
                        if (w) {
                            if (pos >= cap) raster_or_word(sb, k, w, g);
                            ++pos;
                        }
                    }
                }
            } else {
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
        if constexpr (kRaster) {
            __syncthreads();
            const uint32_t nl = n_list < cap ? n_list : cap;
            for (uint32_t e = threadIdx.x; e < nl; e += kFlagThreads) raster_or_word(sb, list_i[e], list_w[e], g);
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
    auto run_batch = [&](int q0) {  // quads q0 .. q0 + kBatch - 1, in `pre`
        const uint4(&pq)[kQ] = pre;
        uint32_t f[kQ];
        int pfx[kQ];
#pragma unroll
        for (int u0 = 0; u0 < kQ; u0 += kFlagGroup) {
            uint32_t wd[kFlagGroup][4], sh[kFlagGroup], ok[kFlagGroup];  // words; bit numbers, on-sensor: a byte each
#pragma unroll
            for (int u = 0; u < kFlagGroup; ++u) {
                const uint32_t ev[4] = {pq[u0 + u].x, pq[u0 + u].y, pq[u0 + u].z, pq[u0 + u].w};
                sh[u] = ok[u] = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t x = (uint32_t)ecc::xy_x(ev[k]), y = (uint32_t)ecc::xy_y(ev[k]);
                    const FlagSlot sl = flag_look<kRaster>(x, y, g, last);
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
        // quad u of lane tid holds events 4 (q0 + u * T + tid) .. + 3: event order is u, then wave,
        // then lane
        auto write_quad = [&](int u, int off) {
            if (f[u]) {
                if (f[u] & 0x1u) dst[off++] = pq[u].x;
                if (f[u] & 0x100u) dst[off++] = pq[u].y;
                if (f[u] & 0x10000u) dst[off++] = pq[u].z;
                if (f[u] & 0x1000000u) dst[off++] = pq[u].w;
            }
        };
        if constexpr (kCand && kFlagScan) {
            // A quad has <= 4 flags and a wave <= 256 per quad slot, the workgroup <= 64 *
            // kFlagThreads / 16: two counts to a word in 16-bit fields (the four waves' total
            // reaches 1024, past a 10-bit field), each word one DPP scan; lane 63's words are the
            // wave's totals.  The totals are double-buffered by the batch's parity: batch b + 2
            // writes a buffer only behind batch b + 1's barrier, which every read of batch b precedes.
            static_assert(4 * kFlagThreads < 65536, "a quad slot's flags fit a 16-bit field");
            constexpr int kPairs = kQ / 2;
            uint32_t *const tot = ctot + (((q0 / kBatch) & 1) ? kFlagWaves * kPairs : 0);
            uint32_t cw[kPairs], sc[kPairs];
#pragma unroll
            for (int j = 0; j < kPairs; ++j) {
                cw[j] = (uint32_t)__popc(f[2 * j]) | ((uint32_t)__popc(f[2 * j + 1]) << 16);  // flag bytes are 0 or 1
                sc[j] = (uint32_t)ecc::wave_incl_scan((int)cw[j]);
            }
            if (lane == 63) {
#pragma unroll
                for (int j = 0; j < kPairs; ++j) tot[wave * kPairs + j] = sc[j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kPairs; ++j) {
                uint32_t below = 0u, all = 0u;  // packed: the waves before this one, and every wave
#pragma unroll
                for (int w = 0; w < kFlagWaves; ++w) {
                    const uint32_t tw = tot[w * kPairs + j];
                    below += w < wave ? tw : 0u;
                    all += tw;
                }
                const uint32_t ex = sc[j] - cw[j] + below;  // field by field: no borrow, no carry
                write_quad(2 * j, base + (int)(ex & 0xffffu));
                base += (int)(all & 0xffffu);
                write_quad(2 * j + 1, base + (int)(ex >> 16));
                base += (int)(all >> 16);
            }
        } else if constexpr (kCand) {
#pragma unroll
            for (int u = 0; u < kQ; ++u) {
                // a quad has <= 4 flags, so three ballots give each lane its prefix
                const int c = __popc(f[u]);  // flag bytes are 0 or 1
                const uint64_t b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
                pfx[u] = __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
                if (lane == 0) ctot[u * kFlagWaves + wave] = (uint32_t)(__popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2));
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kQ; ++u) {
                int off = base + pfx[u];
#pragma unroll
                for (int w = 0; w < kFlagWaves; ++w) {
                    const int tw = (int)ctot[u * kFlagWaves + w];
                    off += w < wave ? tw : 0;
                    base += tw;
                }
                write_quad(u, off);
            }
            __syncthreads();  // ctot is rewritten by the next batch
        }
    };
    for (int q0 = 0; q0 < n4; q0 += kBatch) {  // uniform
        if constexpr (kPipe) {
#pragma unroll
            for (int u = 0; u < kQ; ++u) pre[u] = nxt[u];
            __builtin_amdgcn_sched_barrier(0);
            load_batch(reinterpret_cast<uint4(&)[kQ]>(nxt), q0 + kBatch);
        } else {
            if (q0 > 0) load_batch(pre, q0);
        }
        run_batch(q0);
    }
    if constexpr (kCand) {
        if (threadIdx.x == 0) {
            for (int i = 4 * n4; i < len; ++i) {  // the batch's last < 4 events, in order
                const uint32_t v = xy[lo + i];
                const uint32_t fb = corner_bit<kStaged>(v, g, last, sb, rg) & (i < live_end ? 1u : 0u);
                flags[lo + i] = (uint8_t)fb;
                if (fb) dst[base++] = v;
            }
            n_cand[s] = base;
        }
    } else {
        for (int i = 4 * n4 + threadIdx.x; i < len; i += kFlagThreads)  // last < 4 events, or unaligned slices
            flags[lo + i] = (uint8_t)(corner_bit<kStaged>(xy[lo + i], g, last, sb, rg) & (i < live_end ? 1u : 0u));
    }
}

}  // namespace

int ecc::corner::launch_flags(ecc_ctx *ctx, hipStream_t s, const uint32_t *xy, const CornerGeom &g, const GroupImages &gi,
                              const int32_t *first_border, uint8_t *corner_flags, uint32_t *cand, int32_t *n_cand) {
    ECC_TIMED(ctx, s, "flags_kernel");
    constexpr size_t kLdsMax = kFlagDynLdsMax;
    // staged wherever the tile segments fit, in either form (the raster bitmap is the smaller)
    const bool staged = (size_t)g.n_tiles * kSegWords * sizeof(uint32_t) <= kLdsMax;
    const size_t lds = (size_t)flag_lds_words((uint32_t)g.n_tiles) * sizeof(uint32_t);
    if (staged) {
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
