// Corner detection, stage 5: the arc tests of every (group, tile) item (pipeline and the arc
// test's branch-free form: corners.hip).  arc_kernel takes the common case on compact window
// lists and clamped 32-bit keys; arc_dense_kernel redoes what it leaves (heavy windows, wide
// groups, ties the clamp may have merged) on dense per-slice planes with the exact int64 tests.
#include "arc_select.hpp"
#include "corner_common.hpp"

namespace {

constexpr int kArcThreads = 512;  // 8 waves: one lane per window pixel (484) when staging

__constant__ constexpr int8_t c3dy[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__constant__ constexpr int8_t c3dx[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
__constant__ constexpr int8_t c4dy[20] = {0, 1, 2, 3, 4, 4, 4, 3, 2, 1, 0, -1, -2, -3, -4, -4, -4, -3, -2, -1};
__constant__ constexpr int8_t c4dx[20] = {4, 4, 3, 2, 1, 0, -1, -2, -3, -4, -4, -4, -3, -2, -1, 0, 1, 2, 3, 4};

// arc_streak (the count form, used by the exact tests), sort_desc, the selection networks and
// arc_keys (the fast test on clamped 32-bit keys) are in arc_select.hpp, which the host compiles too.

// The corner pairs leave the arc kernels SLICE-major: res[group][j][tile][kSegWords], bit lp of
// word w = pair (j, pixel 32 w + lp), so that the flag pass of slice j stages its segment of every
// tile as one contiguous run (item-major words put one 4-B read of each tile in its own 128-B
// line, and the 32 slices of a group, on 8 XCDs, fetched every line ~8 times: ~90 MB per step).
// Lane w < 32 * 7 of an item's workgroup writes word w from the item's LDS bits `bits`
// (pair j * 196 + lp); neighbouring tiles' words are adjacent, so the writes combine in L2.
__device__ __forceinline__ void store_res_slice_major(const uint32_t *bits, int64_t grp, int tile, const CornerGeom &g,
                                                      uint32_t *__restrict__ res, int tid) {
    if (tid >= kGroup * kSegWords) return;
    const int j = tid / kSegWords, w = tid % kSegWords;
    const int b0 = j * kTilePix + 32 * w, w0 = b0 >> 5, sh = b0 & 31;
    uint32_t v = bits[w0] >> sh;
    if (sh && w0 + 1 < kPairWords) v |= bits[w0 + 1] << (32 - sh);
    if (w == kSegWords - 1) v &= (1u << (kTilePix - 32 * (kSegWords - 1))) - 1u;  // 4 bits of the last word
    res[(grp * kGroup + j) * g.seg_stride + tile * kSegWords + w] = v;
}
constexpr int kWaves = kArcThreads / 64;
constexpr int kQ4Cap = 1024;  // two 8-wave workgroups per CU fit the 160 KiB LDS

// Staged neighbourhood of one (group, tile) item (arc_dense_kernel).  T[j][wp] holds the value set
// at window pixel wp by slice j of the group — v' = t - L (narrow groups, exact) or the event
// index + 1 (wide groups) — and is valid only where bit j of mb[wp].mask is set; mb[wp].bc is the
// clamped B_g.  The value an event of slice j sees at wp is T[j*][wp] with j* the highest set bit
// of mask & ((2 << j) - 1), else bc: no forward fill, and T is never cleared.
struct MaskB {
    uint32_t mask;
    uint32_t bc;
};

struct ArcLds {
    uint32_t T[kGroup][kWinPix];      // 60.5 KiB
    MaskB mb[kWinPix];
    uint32_t res[kPairWords];         // corner (slice, pixel) pairs of the tile
    uint16_t tasks[kGroup * kTilePix]; // the tile's eligible pairs (j << 9 | window pixel)
    uint16_t q4[kQ4Cap];               // circle-3 survivors (beyond the cap: tested inline)
    int64_t wave_min[16];  // per wave (up to 16 waves: arc_dense_kernel's workgroup size is a switch)
    int32_t exact_only;  // a value above t_last: clamped keys unusable
    int32_t mixed;       // clamped values not all equal to the window minimum of B
    int32_t q4n;
    int32_t n_exact;      // some task needs the exact int64 test
    int32_t wave_own[16];  // the wave's own-tile pixels have pairs
    int32_t wave_tasks[16];  // the wave's eligible pairs (task-list offsets by a scan)
};

// The clamped B_g values (at or below L) are "mixed" when not all equal: ties among their keys may
// then be artefacts of the clamp.  Per wave: its first clamped value c0 and flags cf (bit 1: it has
// one, bit 0: another differs), by ballots and readlanes (no 64-bit reductions); bq = INT64_MAX
// outside the sensor (never at or below Lt).
__device__ __forceinline__ int64_t readlane_i64(int64_t v, int l) {
    return (int64_t)((uint64_t)__builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), l) << 32 |
                     (uint64_t)__builtin_amdgcn_readlane((uint32_t)v, l));
}
__device__ __forceinline__ void clamp_wave_flags(int64_t bq, int64_t Lt, int64_t &c0, int &cf) {
    const bool clp = bq <= Lt;
    const uint64_t cball = __ballot(clp);
    c0 = 0;
    cf = 0;
    if (cball) {  // uniform
        c0 = readlane_i64(bq, __ffsll((unsigned long long)cball) - 1);
        cf = 2 | (__ballot(clp && bq != c0) != 0ull ? 1 : 0);
    }
}
// Wave 0 after the barrier: lane w takes wave w's (c0, cf); the window's "mixed" flag.
template <int W>
__device__ __forceinline__ bool clamp_mixed(const int64_t *wc0, const int32_t *wcf, int lane) {
    const int wf = lane < W ? wcf[lane] : 0;
    const int64_t wv = lane < W ? wc0[lane] : 0;
    const uint64_t has = __ballot(wf & 2);
    bool mixed = __ballot(wf & 1) != 0ull;
    if (has) {  // uniform
        const int64_t v0 = readlane_i64(wv, __ffsll((unsigned long long)has) - 1);
        mixed = mixed || __ballot((wf & 2) && wv != v0) != 0ull;
    }
    return mixed;
}
// (arc_clamp_value and arc_clamp_rel, the maps to clamped keys, are in arc_select.hpp: the host runs them
// over the int64 edges)

// slices 0 .. j (arc_select.hpp: the host checks it with the compact list's index arithmetic)
__device__ __forceinline__ uint32_t below_mask(int j) { return arc_below_mask(j); }

// Clamped value at window pixel wp for slice j (fast path).
__device__ __forceinline__ uint32_t win_value(const ArcLds &L, int wp, uint32_t below) {
    const MaskB m = L.mb[wp];
    const uint32_t mk = m.mask & below;
    return mk ? L.T[31 - __clz(mk)][wp] : m.bc;
}

// Exact arc test of one circle around window pixel wp0 (global pixel q0) for slice j, on the
// reference's own ordering of the int64 values (double_key):
// V = the group value (v' + L, or the timestamp of the stored event index) where a slice <= j of
// the group touched the pixel, else B_g.  Rare fallback; out of line so its registers do not
// raise the pressure of the main kernel body.
struct ExactCtx {
    const int64_t *Bg;  // B_g image of the group
    const int64_t *t;
    int64_t grp_first, Lt;
    int W;
    bool narrow;
};

// Order key of (double)v: k(a) > k(b) <=> (double)a > (double)b.  The reference's arc scan takes
// its minimum and its `>=` on (double)t (:977-990, :1024-1036), and a streak passes exactly when
// every value of the arc is greater IN DOUBLE than every value outside it (which implies the two
// int64 neighbour comparisons, :968/:972), so arc_streak on these keys is the reference's test.
// Below 2^53 in magnitude the conversion is exact and the order is the int64 one.  The bits of a
// non-negative double order as integers; a negative one's magnitude bits are flipped (an int64
// never converts to -0.0 or NaN).
__device__ __forceinline__ int64_t double_key(int64_t v) {
    const int64_t b = __builtin_bit_cast(int64_t, (double)v);
    return b ^ ((b >> 63) & INT64_MAX);
}

template <int N>
__device__ __forceinline__ void exact_values(const ArcLds *L, int wp0, int64_t q0, uint32_t below,
                                             const int8_t *dy, const int8_t *dx, const ExactCtx &c, int64_t (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        // four neighbours' loads in flight at a time: all of them at once spilled (rare path)
        if (k > 0 && k % 4 == 0) __builtin_amdgcn_sched_barrier(0);
        const int wp = wp0 + dy[k] * kWin + dx[k];
        const uint32_t mk = L->mb[wp].mask & below;
        const uint32_t tv = mk ? L->T[31 - __clz(mk)][wp] : 0u;
        v[k] = double_key(!mk        ? c.Bg[q0 + (int64_t)dy[k] * c.W + dx[k]]
                          : c.narrow ? c.Lt + (int64_t)tv
                                     : c.t[c.grp_first + tv - 1u]);
    }
}


// Both circles exactly (circle 3 skipped when it already passed on keys).  Out of line, called
// only from arc_dense_item's exact phase, where nothing else is live.
__device__ __noinline__ bool exact_pair_test(const ArcLds *L, int wp0, int64_t q0, uint32_t below, bool c3_passed,
                                             const int64_t *Bg, const int64_t *t, int64_t grp_first, int64_t Lt, int W,
                                             bool narrow) {
    const ExactCtx c{Bg, t, grp_first, Lt, W, narrow};  // scalars in registers, not a by-value struct on the stack
    if (!c3_passed) {
        int64_t v3[16];
        exact_values<16>(L, wp0, q0, below, c3dy, c3dx, c, v3);
        if (!arc_streak<16, 3, 6>(v3)) return false;
    }
    int64_t v4[20];
    exact_values<20>(L, wp0, q0, below, c4dy, c4dx, c, v4);
    return arc_streak<20, 4, 8>(v4);
}

// 5. Arc test of one (group, tile) item, all items of all groups in one launch.  The item's
// corner pairs go to res (slice-major, store_res_slice_major); flags_event_kernel applies them.
//
// Staging: window pixel wp of the item (lane wp < 484) reads its slice mask, its value record and
// its B_g from fixed per-pixel addresses (pair_build's gmask / pv images, sae_prefix's B), three
// independent loads in flight together; only a pixel with more than four values reads the rest
// of them from the overflow array, at the address its record names.

// The slices of group grp whose pairs are tested (Q15: slices before first_detect are not).
__device__ __forceinline__ uint32_t eligible_slices(const CornerGeom &g, int64_t grp) {
    const int gs = (int)grp * kGroup;  // the group's first slice (n_slices < 2^31: host check)
    if (g.first_detect <= gs) return 0xffffffffu;
    const int j0 = g.first_detect - gs;  // > 0 with gs >= 0: no overflow
    return j0 >= kGroup ? 0u : (0xffffffffu << j0);
}

// The values v3 .. v_{p-1} (p > 4) of a pixel whose record is r, from the overflow array:
// the run starts 16-B aligned at line r.w, so line l holds
// v_{3 + 4l} .. v_{6 + 4l}.  Lines l0 .. of the run, four lines (16 values) in flight per trip
// (clamped to the last line, no load under a lane condition): a pixel with 32 values costs two
// dependent round trips instead of seven 4-value ones.
template <class Put>
__device__ __forceinline__ void overflow_lines(const uint32_t *__restrict__ ovf, const uint4 &r, int l0, int p, Put put) {
    const uint4 *__restrict__ x4 = reinterpret_cast<const uint4 *>(ovf) + r.w;
    const int nl = (p - (kRecVals - 1) + 3) >> 2;
    for (; l0 < nl; l0 += 4) {
        uint4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = x4[min(l0 + u, nl - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = (kRecVals - 1) + 4 * (l0 + u);
            if (k < p) put(k, a[u].x);
            if (k + 1 < p) put(k + 1, a[u].y);
            if (k + 2 < p) put(k + 2, a[u].z);
            if (k + 3 < p) put(k + 3, a[u].w);
        }
    }
}

#ifndef ECC_ARC_PROFILE
#define ECC_ARC_PROFILE 0
#endif
#if ECC_ARC_PROFILE
// profiling builds: arc_dense_kernel's per-item phases summed (thread 0), [5] = the longest item,
// [6] = tasks, [7] = items
__device__ unsigned long long g_dense_prof[8];
#define DENSE_MARK(k)                                                                \
    do {                                                                             \
        if (tid == 0) {                                                              \
            const unsigned long long now_ = wall_clock64();                          \
            atomicAdd(&g_dense_prof[k], now_ - dense_t_);                            \
            dense_t_ = now_;                                                         \
        }                                                                            \
    } while (0)
#else
#define DENSE_MARK(k) do { } while (0)
#endif

template <int NT>
__device__ __forceinline__ void arc_dense_item(ArcLds &L, int64_t item, const int64_t *__restrict__ t, const CornerGeom &g,
                                               const uint32_t *__restrict__ ovf, const uint4 *__restrict__ pv,
                                               const int64_t *__restrict__ gB, const uint32_t *__restrict__ gmask,
                                               uint32_t *__restrict__ res, const GroupRec *__restrict__ grec) {
    int64_t grp;
    int tile;
    item_decode(g, item, grp, tile);
    if ((int)grp < (g.first_detect >> 5)) return;  // (grp + 1) * 32 <= first_detect: every slice precedes detection
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#if ECC_ARC_PROFILE
    const unsigned long long dense_t0_ = wall_clock64();
    unsigned long long dense_t_ = dense_t0_;
#endif
    const int64_t HW = (int64_t)g.H * g.W;
    int tx, ty;
    tile_origin_xy(g, tile, tx, ty);
    const int x0 = tx * kTile, y0 = ty * kTile;
    const GroupRef gr = group_ref_of(grec[grp]);  // uniform: one scalar load
    const int64_t grp_first = gr.first, Lt = gr.Lt;
    const bool narrow = gr.narrow;
    const int64_t *Bg = gB + grp * HW;

    // (a) window pixel wp (lane wp < 484): its B_g, slice mask and value record, three loads in
    //     flight together; its values go to the dense planes T[j][wp], the own tile's eligible
    //     pairs (slice and pixel; the per-event cut of border mode 1 is applied when flagging)
    //     are the test tasks
    static_assert(NT >= kWinPix, "one lane per window pixel");
    const int wp = tid;
    const bool win_lane = wp < kWinPix;
    const int ox = wp % kWin - kHalo, oy = wp / kWin - kHalo;  // pixel relative to the tile origin
    const int wx = x0 + ox, wy = y0 + oy;
    const bool in = win_lane && wx >= 0 && wy >= 0 && wx < g.W && wy < g.H;
    const int64_t q = grp * HW + (int64_t)wy * g.W + wx;
    int64_t bq = INT64_MAX;  // outside: never read (the window minimum skips it; `in` tells it from a real INT64_MAX)
    uint32_t mk = 0u;
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (in) {
        bq = gB[q];
        mk = gmask[q];
        rec = pv[q];
    }
    for (int w = tid; w < kPairWords; w += NT) L.res[w] = 0u;
    if (tid == 0) {
        L.exact_only = narrow ? 0 : 1;  // wide groups: every test exact
        L.mixed = 0;
        L.q4n = 0;
        L.n_exact = 0;
    }
    const bool own = win_lane && ox >= 0 && oy >= 0 && ox < kTile && oy < kTile;
    const uint64_t own_pairs = __ballot(own && mk != 0u);
    if (lane == 0) L.wave_own[wave] = own_pairs != 0ull;
    // the own tile's eligible pairs, placed by a scan (one returning LDS atomic per pair on one
    // counter serialised a heavy item's ~3 000 tasks)
    const uint32_t tm0 = (own && !is_border(wx, wy, g)) ? (mk & eligible_slices(g, grp)) : 0u;
    const int tcnt = __popc(tm0);
    const int tincl = ecc::wave_incl_scan(tcnt);  // DPP
    if (lane == 63) L.wave_tasks[wave] = tincl;
    __syncthreads();
    if (win_lane) {
        L.mb[wp].mask = mk;
        const int p = __popc(mk);
        uint32_t mm = mk;
        for (int k = 0; mm && k < kRecVals - 1; ++k, mm &= mm - 1u)
            L.T[__ffs(mm) - 1][wp] = k == 0 ? rec.x : (k == 1 ? rec.y : rec.z);
        if (mm && p == kRecVals) {
            L.T[__ffs(mm) - 1][wp] = rec.w;
        } else if (mm) {  // v3.. from the overflow array, ascending j as the bits
            overflow_lines(ovf, rec, 0, p, [&](int, uint32_t v) {
                L.T[__ffs(mm) - 1][wp] = v;
                mm &= mm - 1u;
            });
        }
    }
    int toff = tincl - tcnt, n_tasks = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const int c = L.wave_tasks[w];
        toff += w < wave ? c : 0;
        n_tasks += c;
    }
    for (uint32_t tm = tm0; tm; tm &= tm - 1u) L.tasks[toff++] = (uint16_t)((__ffs(tm) - 1) << 9 | wp);  // j << 9 | window pixel
    const int64_t bmin = ecc::wave_min_i64(bq);  // DPP
    if (lane == 0) L.wave_min[wave] = bmin;
    __syncthreads();
    DENSE_MARK(0);  // (a) staging
    {
        int any = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) any |= L.wave_own[w];
        if (!any) return;  // uniform: no events in the tile, nothing to flag
    }
    DENSE_MARK(1);

    // (c) clamped B_g per window pixel
    if (win_lane) {
        int64_t vz = INT64_MAX;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) vz = L.wave_min[w] < vz ? L.wave_min[w] : vz;
        L.mb[wp].bc = (!narrow || !in) ? 0u : arc_clamp_rel(bq, Lt, vz, kVMax, &L.exact_only, &L.mixed);
    }
    __syncthreads();
    DENSE_MARK(2);  // (c)

    // (d) each eligible pair of the tile is tested once, in three phases so that no phase holds
    //     another's registers (and no call): circle 3 on clamped keys, its survivors queued so
    //     that circle 4 runs on as few waves as possible; circle 4 on clamped keys; then the
    //     exact int64 tests of whatever the keys could not decide, marked in the task list
    //     itself (bit 14: circle 3 undecided; bit 15: circle 3 passed, circle 4 still open).
    //     Wide groups and values above t_last (exact_only) take every task exactly.
    const bool fast = !L.exact_only;
    const bool ties_exact = !L.mixed;
    constexpr uint16_t kOpen3 = 0x4000, kOpen4 = 0x8000;
    if (fast) {
        for (int ti = tid; ti < n_tasks; ti += NT) {
            const int pi = L.tasks[ti];  // j << 9 | window pixel
            const int wp0 = pi & 511;
            const uint32_t below = below_mask(pi >> 9);
            uint32_t k3[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) k3[k] = (win_value(L, wp0 + c3dy[k] * kWin + c3dx[k], below) << 5) | k;
            const int r3 = arc_keys<16, 5, 3, 6>(k3, ties_exact);
            if (r3 > 0) {
                const int qi = atomicAdd(&L.q4n, 1);
                if (qi < kQ4Cap) L.q4[qi] = (uint16_t)ti;
                else { L.tasks[ti] = (uint16_t)(pi | kOpen4); L.n_exact = 1; }  // queue full (rare)
            } else if (r3 < 0) {
                L.tasks[ti] = (uint16_t)(pi | kOpen3);
                L.n_exact = 1;
            }
        }
    }
    __syncthreads();
    DENSE_MARK(3);  // circle 3
    const int n4 = min(L.q4n, kQ4Cap);
    for (int qi = tid; qi < n4; qi += NT) {
        const int ti = L.q4[qi];
        const int pi = L.tasks[ti];
        const int j = pi >> 9, wp0 = pi & 511;
        const uint32_t below = below_mask(j);
        uint32_t k4[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) k4[k] = (win_value(L, wp0 + c4dy[k] * kWin + c4dx[k], below) << 5) | k;
        const int r4 = arc_keys<20, 5, 4, 8>(k4, ties_exact);
        if (r4 > 0) {  // the pair's bit: slice j, tile pixel (wp0's row and column less the halo)
            const int rb = j * kTilePix + (wp0 / kWin - kHalo) * kTile + (wp0 % kWin - kHalo);
            atomicOr(&L.res[rb >> 5], 1u << (rb & 31));
        } else if (r4 < 0) {
            L.tasks[ti] = (uint16_t)(pi | kOpen4);
            L.n_exact = 1;
        }
    }
    __syncthreads();
    DENSE_MARK(4);  // circle 4
    if (!fast || L.n_exact) {  // uniform; rare: the exact int64 tests
        for (int ti = tid; ti < n_tasks; ti += NT) {
            const int e = L.tasks[ti], pi = e & 0x3fff;
            if (fast && !(e & (kOpen3 | kOpen4))) continue;
            const int j = pi >> 9, wp0 = pi & 511;
            const int ly = wp0 / kWin - kHalo, lx = wp0 % kWin - kHalo;
            const int64_t q0 = (int64_t)(y0 + ly) * g.W + (x0 + lx);
            const uint32_t below = below_mask(j);
            if (exact_pair_test(&L, wp0, q0, below, (e & kOpen4) != 0, Bg, t, grp_first, Lt, g.W, narrow)) {
                const int rb = j * kTilePix + ly * kTile + lx;
                atomicOr(&L.res[rb >> 5], 1u << (rb & 31));
            }
        }
        __syncthreads();
    }
#if ECC_ARC_PROFILE
    if (tid == 0) {
        atomicMax(&g_dense_prof[5], wall_clock64() - dense_t0_);
        atomicAdd(&g_dense_prof[6], (unsigned long long)n_tasks);
        atomicAdd(&g_dense_prof[7], 1ull);
    }
#endif
    store_res_slice_major(L.res, grp, tile, g, res, tid);
}

// ---- compact window values (the common case) -------------------------------------------------
// Window pixel wp keeps its clamped B_g followed by the values of the slices that touched it,
// ascending j, from byte pix[wp].off of vals; the value an event of slice j sees is the word at
// byte off + 4 * popc(mask & ((2 << j) - 1)) (arc_value_byte) — the B_g slot when no slice <= j
// touched the pixel, so a lookup is one 8-B pixel read and one value read, no select.  ~34 KB of LDS
// instead of the dense planes' ~80 KB: four 8-wave workgroups per CU.  Windows with more than
// kValCap values go to the overflow list (arc_dense_kernel).
#ifndef ECC_ARC_VALCAP
#define ECC_ARC_VALCAP 4096
#endif
constexpr int kValCap = ECC_ARC_VALCAP;

struct PixInfo {
    uint32_t mask;  // slices of the group that touched the pixel
    uint32_t off;   // its B_g slot in vals[], in BYTES (4 * the word index); the slice values follow
};

// pix stands first: a task's circle pixels are then all read off ONE address register, the
// record of the window pixel four rows up and four columns left of the task's (circle_base),
// with each pixel's displacement in the read's offset field.  ds_read2_b64's two offsets count
// 8-B units up to 255; in the middle of the struct the compiler rounded the address down to
// what those fields reach and needed five registers per circle-3 trip for it.
struct SparseLds {
    PixInfo pix[kWinPix];               // 3.8 KiB
    uint32_t vals[kValCap + kWinPix];   // 17.9 KiB: the pairs + one B_g slot per window pixel
    uint32_t res[kPairWords];
    uint16_t tasks[kValCap];  // the tile's eligible pairs (j << 9 | window pixel): at most the window's pairs
    uint16_t q4[kQ4Cap];
    int64_t wave_c0[kWaves];    // the wave's first B_g at or below L (clamped to 0) ...
    int32_t wave_cf[kWaves];    // ... bit 1: it has one, bit 0: another differs from it
    int32_t wave_tot[kWaves];   // the wave's counts and its own-tile flag, packed (arc_item)
    int32_t exact_only, mixed, q4n, redo;
};

// Branch-free by layout: one 8-B pixel read and one value read (a conditional read compiles to
// an exec-mask branch per circle pixel: scalar-unit bookkeeping, serialised LDS round trips).
static_assert(sizeof(PixInfo) == 8, "one 8-B LDS read per pixel");
__device__ __forceinline__ uint32_t sparse_value(const SparseLds &L, const uint2 *pix, int d, uint32_t below) {
    const uint2 p = pix[d];  // {mask, off in bytes}
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(L.vals) +
                                               arc_value_byte_below(p.x, below, p.y));
}

// The circles' pixel reads are relative to the window pixel kHalo rows up and kHalo columns left
// of the task's: displacement (dy + kHalo) * kWin + dx + kHalo, never negative, and small
// enough for the paired 8-B read's offset field whatever the task pixel.
// The byte offset passes through an empty asm so that it stays one value in one register: left
// to itself the compiler folds the constant back into the displacements, half of them negative
// again, and forms a register per negative one (seven adds per circle-3 trip).
__device__ __forceinline__ const uint2 *circle_base(const SparseLds &L, int wp0) {
    uint32_t b = (uint32_t)(wp0 - kHalo * kWin - kHalo) * (uint32_t)sizeof(PixInfo);
    asm("" : "+v"(b));
    return reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(L.pix) + b);
}
constexpr int circle_disp(int dy, int dx) { return (dy + kHalo) * kWin + dx + kHalo; }
template <int N>
constexpr bool circle_disps_fit(const int8_t (&dy)[N], const int8_t (&dx)[N]) {
    for (int k = 0; k < N; ++k)
        if (circle_disp(dy[k], dx[k]) < 0 || circle_disp(dy[k], dx[k]) > 255) return false;
    return true;
}
static_assert(circle_disps_fit(c3dy, c3dx) && circle_disps_fit(c4dy, c4dx),
              "every circle pixel within ds_read2_b64's offset field (8-B units, 8 bits: below 2040 B)");
static_assert(offsetof(SparseLds, pix) == 0, "the circle base is 8 * task pixel less a constant: no struct offset to add");

#ifndef ECC_ARC_SKIP_OVF
#define ECC_ARC_SKIP_OVF 0  // timing experiments only (wrong results): 1 = no overflow loads past the first line
#endif
#ifndef ECC_ARC_WAVES
#define ECC_ARC_WAVES 8
#endif

#if ECC_ARC_PROFILE
// profiling builds: per-workgroup wall-clock of arc_kernel's phases, summed (thread 0); [7] = items
// per item (no global atomics on shared words: 18 K workgroups adding to 8 words serialised at
// the memory side and distorted the very phases they timed); summed on the host
constexpr int kProfItems = 1 << 15;
__device__ unsigned long long g_arc_items[kProfItems][8];
#define ARC_MARK(k)                                                                  \
    do {                                                                             \
        if (tid == 0) {                                                              \
            const unsigned long long now_ = wall_clock64();                          \
            arc_ph_[k] = now_ - arc_t_;                                              \
            arc_t_ = now_;                                                           \
        }                                                                            \
    } while (0)
#else
#define ARC_MARK(k) do { } while (0)
#endif

// One item's phase-A loads: window pixel `tid`'s B_g, slice mask and value record, from fixed
// per-pixel addresses (no offset table in between), so the three are in flight together.
struct ArcPre {
    int64_t bq;   // B_g (INT64_MAX outside the sensor / past the window)
    uint32_t mk;  // slices of the group that touched the pixel
    uint4 rec;    // its values (pair_build's record)
};

__device__ __forceinline__ void arc_prefetch(ArcPre &p, int64_t item, const CornerGeom &g, const uint4 *__restrict__ pv,
                                             const int64_t *__restrict__ gB, const uint32_t *__restrict__ gmask) {
    const int tid = threadIdx.x;
    p.bq = INT64_MAX;
    p.mk = 0u;
    p.rec = make_uint4(0u, 0u, 0u, 0u);
    const int64_t HW = (int64_t)g.H * g.W;
    int64_t grp;
    int tile, tx, ty;
    item_decode(g, item, grp, tile);
    tile_origin_xy(g, tile, tx, ty);
    const int wx = tx * kTile - kHalo + tid % kWin, wy = ty * kTile - kHalo + tid / kWin;
    if (tid < kWinPix && wx >= 0 && wy >= 0 && wx < g.W && wy < g.H) {
        const int64_t q = grp * HW + (int64_t)wy * g.W + wx;
        p.bq = gB[q];
        p.mk = gmask[q];
        p.rec = pv[q];
    }
}

// The arc tests of one (group, tile) item from its phase-A loads `pre`.
//   A: wave scans of the value counts and task counts, wave minimum of B_g    -> barrier 1
//   B: pixel records, clamped B_g slots, values (overflow loads), tasks       -> barrier 2
//   circle 3 -> barrier 3 -> circle 4 -> barrier 4
// Every lane knows its own pixel's values, so the list offsets, the task offsets and the window
// minimum of B_g are all wave scans before the first barrier, and each lane writes its pixel's
// list and tasks itself (no scatter, no LDS atomics).
__device__ __forceinline__ void arc_item(SparseLds &L, int64_t item, const ArcPre &pre,
                                         const GroupRec *__restrict__ grec, const CornerGeom &g,
                                         const uint32_t *__restrict__ ovf, uint32_t *__restrict__ res,
                                         int64_t *__restrict__ over, uint32_t *__restrict__ n_over) {
    int64_t grp;
    int tile;
    item_decode(g, item, grp, tile);
    if ((int)grp < (g.first_detect >> 5)) return;  // (grp + 1) * 32 <= first_detect: every slice precedes detection
    static_assert(kGroup == 32, "first_detect >> 5");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);  // in a scalar register: uniform selects
#if ECC_ARC_PROFILE
    unsigned long long arc_t_ = wall_clock64(), arc_ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    int tx, ty;
    tile_origin_xy(g, tile, tx, ty);
    const int x0 = tx * kTile, y0 = ty * kTile;
    const GroupRec rec = grec[grp];  // uniform: one scalar load
    const int64_t Lt = rec.Lt;
    const bool narrow = (rec.bits & kRecNarrow) != 0u;
    const int wp = tid;
    const bool win_lane = wp < kWinPix;
    const int64_t bq = pre.bq;
    const uint32_t mk_w = pre.mk;
    const int ox = wp % kWin - kHalo, oy = wp / kWin - kHalo;  // pixel relative to the tile origin
    const bool own = win_lane && ox >= 0 && oy >= 0 && ox < kTile && oy < kTile;
    // on the sensor (a lane mask, taken here where ox and oy are live; arc_clamp_value reads it after barrier 1)
    const bool inside = (unsigned)(x0 + ox) < (unsigned)g.W && (unsigned)(y0 + oy) < (unsigned)g.H;
    for (int w = tid; w < kPairWords; w += kArcThreads) L.res[w] = 0u;
    if (tid == 0) {
        L.exact_only = narrow ? 0 : 1;  // wide groups: every test exact
        L.q4n = 0;
        L.redo = 0;
    }
    // the own tile's eligible pairs of this pixel (Q15 slices; border pixels are never corners)
    const uint32_t tm = (own && !is_border(x0 + ox, y0 + oy, g)) ? (mk_w & eligible_slices(g, grp)) : 0u;
    const int cnt = win_lane ? __popc(mk_w) + 1 : 0;  // the pixel's values + its B_g slot
    const int tcnt = __popc(tm);
    // wave scans and the wave minimum of B_g by DPP moves
    // one scan of both counts, packed (task count << kTaskShift | value count: a workgroup's sums
    // are at most 484 * 33 < 2^14 values and 196 * 32 < 2^13 tasks); the wave's word for the
    // others adds its "own-tile pixels have pairs" flag above them (eight of them sum below 2^4),
    // so the packed words are summed as they are and unpacked once
    constexpr int kTaskShift = 14, kOwnShift = 27;
    constexpr int kCntMask = (1 << kTaskShift) - 1, kTaskMask = (1 << (kOwnShift - kTaskShift)) - 1;
    const int both = ecc::wave_incl_scan(tcnt << kTaskShift | cnt);
    const int incl = both & kCntMask, tincl = both >> kTaskShift;
    const uint64_t own_pairs = __ballot(own && mk_w != 0u);
    int64_t c0;
    int cf;
    clamp_wave_flags(bq, Lt, c0, cf);  // the window's "mixed" clamp, per wave
    // a pixel with more than 4 values: v3 .. v6 as one 16-B load, issued now (its address is in
    // the record) so that it flies during the scans and the barrier; the other lanes of the wave
    // load the first line of ovf (no per-lane branch around the load)
    const int p = cnt - 1;
#ifndef ECC_ARC_XPF
#define ECC_ARC_XPF 1  // 16-B overflow lines loaded before barrier 1 (0: none, after it)
#endif
    constexpr int kXpf = ECC_ARC_XPF > 0 ? ECC_ARC_XPF : 1;
    uint4 xs[kXpf];
#pragma unroll
    for (int u = 0; u < kXpf; ++u) xs[u] = make_uint4(0u, 0u, 0u, 0u);
    if (ECC_ARC_XPF && __ballot(p > kRecVals)) {  // uniform
        const bool o = p > kRecVals;
        const uint4 *x4 = reinterpret_cast<const uint4 *>(ovf) + (o ? pre.rec.w : 0u);
        const int nl = o ? (p - (kRecVals - 1) + 3) >> 2 : 1;  // lines of the lane's run
#pragma unroll
        for (int u = 0; u < kXpf; ++u) xs[u] = x4[min(u, nl - 1)];  // no load past the run
    }
    if (lane == 63) L.wave_tot[wave] = both | (own_pairs != 0ull ? 1 << kOwnShift : 0);
    if (lane == 0) {
        L.wave_c0[wave] = c0;
        L.wave_cf[wave] = cf;
    }
    __syncthreads();  // 1
    ARC_MARK(0);  // A
    int sum = 0, before = 0;  // packed: all waves, the waves ahead of this one
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {  // uniform reads, in flight together
        const int wb = L.wave_tot[w];
        sum += wb;
        before += w < wave_s ? wb : 0;
    }
    const int total = sum & kCntMask, any_own = sum >> kOwnShift;
    int n_tasks = (sum >> kTaskShift) & kTaskMask;
    const int off = incl - cnt + (before & kCntMask);
    int toff = tincl - tcnt + ((before >> kTaskShift) & kTaskMask);
    if (wave == 0) {  // L.mixed is read after barrier 2
        const bool mixed = clamp_mixed<kWaves>(L.wave_c0, L.wave_cf, lane);
        if (lane == 0) L.mixed = mixed;
    }
    if (!any_own || total > kValCap + kWinPix) {  // uniform
        // no events in the tile: nothing to flag; too many values for the compact list: the
        // dense kernel takes it
        if (any_own && tid == 0) over[atomicAdd(n_over, 1u)] = item;
        return;
    }
    if (win_lane) {
        const uint32_t bcv = arc_clamp_value(bq, Lt, kVMax, narrow, inside, &L.exact_only);  // above the range: the exact kernel
        reinterpret_cast<uint2 *>(L.pix)[wp] = make_uint2(mk_w, 4u * (uint32_t)off);  // bytes; dst keeps the word offset
        uint32_t *dst = L.vals + off;
        dst[0] = bcv;
        if (p > 0) dst[1] = pre.rec.x;
        if (p > 1) dst[2] = pre.rec.y;
        if (p > 2) dst[3] = pre.rec.z;
        if (p == kRecVals) {
            dst[4] = pre.rec.w;
        } else if (!ECC_ARC_XPF && p > kRecVals) {
            overflow_lines(ovf, pre.rec, 0, p, [&](int k, uint32_t v) { dst[1 + k] = v; });
        } else if (p > kRecVals) {  // v3 .. v6 from the prefetched line, the rest loaded now
            // v_k goes to dst[1 + k] for k < p (here p >= 5); line u holds v_{3+4u} .. v_{6+4u}
#pragma unroll
            for (int u = 0; u < kXpf; ++u) {
                const int k = (kRecVals - 1) + 4 * u;
                if (k < p) dst[1 + k] = xs[u].x;
                if (k + 1 < p) dst[2 + k] = xs[u].y;
                if (k + 2 < p) dst[3 + k] = xs[u].z;
                if (k + 3 < p) dst[4 + k] = xs[u].w;
            }
            if (!ECC_ARC_SKIP_OVF && p > kRecVals + 4 * ECC_ARC_XPF - 1)
                overflow_lines(ovf, pre.rec, ECC_ARC_XPF, p, [&](int k, uint32_t v) { dst[1 + k] = v; });
        }
        // a task is (slice j, window pixel) as j << 9 | wp: the tests decode it with a shift and
        // a mask (no division by the tile and window widths)
        for (uint32_t m = tm; m; m &= m - 1u) L.tasks[toff++] = (uint16_t)((__ffs(m) - 1) << 9 | wp);
    }
    __syncthreads();  // 2
    ARC_MARK(1);  // B
    if (L.exact_only) {  // uniform: a wide group or a value above t_last — the exact kernel takes it
        if (tid == 0) over[atomicAdd(n_over, 1u)] = item;
        return;
    }
    // Tests through the compact lists, on clamped 32-bit keys only.  No exact int64 path and no
    // call: an item its keys cannot decide (a wide group, a value above t_last, a tie the clamping
    // may have merged) or whose circle-3 survivors overflow the queue goes whole to
    // arc_dense_kernel, which redoes it exactly.  So the kernel fits 64 VGPRs without spills.
#ifndef ECC_ARC_SKIP
#define ECC_ARC_SKIP 0  // timing experiments only (wrong results): 1 = no circle 4, 2 = no tests
#endif
    if (ECC_ARC_SKIP >= 2) n_tasks = 0;
    const bool ties_exact = !L.mixed;
    for (int ti = tid; ti < n_tasks; ti += kArcThreads) {
        const int pi = L.tasks[ti];  // j << 9 | window pixel
        const int wp0 = pi & 511;
        const uint32_t below = below_mask(pi >> 9);
        uint32_t k3[16];
        const uint2 *pb = circle_base(L, wp0);
#pragma unroll
        for (int k = 0; k < 16; ++k) k3[k] = (sparse_value(L, pb, circle_disp(c3dy[k], c3dx[k]), below) << 5) | k;
        const int r3 = arc_keys<16, 5, 3, 6>(k3, ties_exact);
        if (r3 > 0) {
            const int qi = atomicAdd(&L.q4n, 1);
            if (qi < kQ4Cap) L.q4[qi] = (uint16_t)pi;
            else L.redo = 1;
        } else if (r3 < 0) {
            L.redo = 1;
        }
    }
    __syncthreads();  // 3
    ARC_MARK(3);  // circle 3
    if (L.redo) {  // uniform
        if (tid == 0) over[atomicAdd(n_over, 1u)] = item;
        return;
    }
    const int n4 = ECC_ARC_SKIP >= 1 ? 0 : L.q4n;
#if ECC_ARC_PROFILE
    if (tid == 0) {
        arc_ph_[5] = (unsigned long long)n_tasks;
        arc_ph_[6] = (unsigned long long)n4;
    }
#endif
    for (int qi = tid; qi < n4; qi += kArcThreads) {
        const int pt = L.q4[qi];  // j << 9 | window pixel
        const int j = pt >> 9, wp0 = pt & 511;
        const uint32_t below = below_mask(j);
        uint32_t k4[20];
        const uint2 *pb = circle_base(L, wp0);
#pragma unroll
        for (int k = 0; k < 20; ++k) k4[k] = (sparse_value(L, pb, circle_disp(c4dy[k], c4dx[k]), below) << 5) | k;
        const int r4 = arc_keys<20, 5, 4, 8>(k4, ties_exact);
        if (r4 > 0) {  // the pair's bit: slice j, tile pixel (wp0's row and column less the halo)
            const int pi = j * kTilePix + (wp0 / kWin - kHalo) * kTile + (wp0 % kWin - kHalo);
            atomicOr(&L.res[pi >> 5], 1u << (pi & 31));
        } else if (r4 < 0) {
            L.redo = 1;
        }
    }
    __syncthreads();  // 4
    ARC_MARK(4);  // circle 4
#if ECC_ARC_PROFILE
    if (tid == 0 && item < kProfItems) {
        arc_ph_[7] = 1ull;
        for (int k = 0; k < 8; ++k) g_arc_items[item][k] = arc_ph_[k];
    }
#endif
    if (L.redo) {  // uniform: a circle-4 tie the clamped keys cannot decide
        if (tid == 0) over[atomicAdd(n_over, 1u)] = item;
        return;
    }
    store_res_slice_major(L.res, grp, tile, g, res, tid);
}

// One workgroup per item, all items of all groups in one launch, in XCD-aware order: workgroup b
// runs on XCD b % 8, so XCD x takes the contiguous item range [x * per, (x + 1) * per) —
// neighbouring tiles of one group share that XCD's L2.
__global__ void __launch_bounds__(kArcThreads, ECC_ARC_WAVES)  // waves/SIMD: 8 = four 8-wave workgroups per CU
arc_kernel(const GroupRec *__restrict__ grec, CornerGeom g, int64_t n_items, const uint32_t *__restrict__ ovf,
           const uint4 *__restrict__ pv, const int64_t *__restrict__ gB, const uint32_t *__restrict__ gmask,
           uint32_t *__restrict__ res, int64_t *__restrict__ over, uint32_t *__restrict__ n_over) {
    __shared__ SparseLds L;
    const int per = (int)(gridDim.x / 8);
    const int64_t item = (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
    if (item >= n_items) return;
    ArcPre pre;
    arc_prefetch(pre, item, g, pv, gB, gmask);
    arc_item(L, item, pre, grec, g, ovf, res, over, n_over);
}


// The windows above the compact list's capacity (arc_kernel's overflow list), each with the
// dense per-slice planes.
#ifndef ECC_DENSE_THREADS
#define ECC_DENSE_THREADS 512  // arc_dense_kernel's workgroup: 512 = two per CU, 1024 = one per CU
#endif
constexpr int kDenseThreads = ECC_DENSE_THREADS;
__global__ void __launch_bounds__(kDenseThreads, 4)  // 4 waves/SIMD (128 VGPRs)
arc_dense_kernel(const int64_t *__restrict__ t, CornerGeom g, const int64_t *__restrict__ over,
                 const uint32_t *__restrict__ n_over, const uint32_t *__restrict__ ovf, const uint4 *__restrict__ pv,
                 const int64_t *__restrict__ gB, const uint32_t *__restrict__ gmask, uint32_t *__restrict__ res,
                 const GroupRec *__restrict__ grec) {
    __shared__ ArcLds L;
    const uint32_t n = *n_over;
    for (uint32_t li = blockIdx.x; li < n; li += gridDim.x) {
        arc_dense_item<kDenseThreads>(L, over[li], t, g, ovf, pv, gB, gmask, res, grec);
        __syncthreads();
    }
}

}  // namespace

void ecc::corner::launch_arc(ecc_ctx *ctx, hipStream_t s, const CornerGeom &g, int64_t n_items, const GroupImages &gi) {
    ECC_TIMED(ctx, s, "arc_kernel");
    const unsigned grid = (unsigned)(8 * ((n_items + 7) / 8));  // multiple of 8 (XCD-aware order)
    hipLaunchKernelGGL(arc_kernel, dim3(grid), dim3(kArcThreads), 0, s, (const GroupRec *)gi.grec, g, n_items,
                       (const uint32_t *)gi.ovf, (const uint4 *)gi.pv, (const int64_t *)gi.B, (const uint32_t *)gi.mask, gi.res, gi.over, gi.n_over);
}

void ecc::corner::launch_arc_dense(ecc_ctx *ctx, hipStream_t s, const int64_t *t, const CornerGeom &g,
                                   const GroupImages &gi) {
    ECC_TIMED(ctx, s, "arc_dense_kernel");  // the items arc_kernel left: dense planes, exact tests
    hipLaunchKernelGGL(arc_dense_kernel, dim3(kDenseThreads == 512 ? 512 : ctx->n_cu), dim3(kDenseThreads), 0, s, t, g, (const int64_t *)gi.over,
                       (const uint32_t *)gi.n_over, (const uint32_t *)gi.ovf, (const uint4 *)gi.pv,
                       (const int64_t *)gi.B, (const uint32_t *)gi.mask, gi.res, (const GroupRec *)gi.grec);
}

#if ECC_ARC_PROFILE
// Profiling builds only (make ARC_PROFILE=1): arc_kernel's summed per-workgroup phase ticks
// since the last call (reset after reading); out[7] = items timed; ticks_per_us from the device.
ECC_API int ecc_arc_dense_profile(unsigned long long *out8, double *ticks_per_us) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_dense_prof), 8 * sizeof(unsigned long long)) != hipSuccess) return ECC_ERR_HIP;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipMemcpyToSymbol(HIP_SYMBOL(g_dense_prof), z, sizeof(z));
    int khz = 0;
    hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0);
    *ticks_per_us = khz / 1000.0;
    return ECC_OK;
}

ECC_API int ecc_arc_profile(unsigned long long *out8, double *ticks_per_us) {
    std::vector<unsigned long long> h((size_t)kProfItems * 8);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_arc_items), h.size() * 8) != hipSuccess) return ECC_ERR_HIP;
    for (int k = 0; k < 8; ++k) out8[k] = 0;
    for (size_t it = 0; it < (size_t)kProfItems; ++it)
        if (h[it * 8 + 7])
            for (int k = 0; k < 8; ++k) out8[k] += h[it * 8 + k];
    std::fill(h.begin(), h.end(), 0ull);
    hipMemcpyToSymbol(HIP_SYMBOL(g_arc_items), h.data(), h.size() * 8);
    int khz = 0;
    hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0);
    *ticks_per_us = khz / 1000.0;
    return ECC_OK;
}
#endif
