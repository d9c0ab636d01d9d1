// Corner detection: what the stage files (corner_sort.hip, corner_pairs.hip, corner_arc.hip,
// corner_flags.hip) and the host driver (corners.hip) share: the constants, the geometry and the
// batch layout that travel from launch to launch, the group records, the tile and group helpers
// and the stages' launch functions.  The types the launch functions take are in ecc::corner (one
// type across the translation units); every device helper has internal linkage.
#pragma once

#include "corner_decode.hpp"
#include "ecc_internal.hpp"

namespace ecc {
namespace corner {

constexpr int kThreads = 256;
// the flag pass's dynamic LDS limit: 160 KiB less its static LDS (ctot[kFlagQuads][4], 128 B)
constexpr size_t kFlagDynLdsMax = 160 * 1024 - 256;
constexpr int kFlagCandMax = 16384;  // slices up to this many events take the candidate-list form
constexpr int kGroup = 32;         // slices per group (mask bits)
constexpr int kTile = 14;          // tile edge (pixels): the 22x22 window fits one 8-wave workgroup
constexpr int kTilePix = kTile * kTile;
constexpr int kHalo = 4;           // circle radius
constexpr int kWin = kTile + 2 * kHalo;  // 22
constexpr int kWinPix = kWin * kWin;     // 484
constexpr int kMaxTiles = 8191;          // bins per group = n_tiles + 1 (8192 fit an LDS histogram)
constexpr int kMaxSlice = 1 << 19;       // group-local event index must fit 24 bits

static_assert(kWin == kTile + 2 * kHalo, "window = tile + halo on both sides");
static_assert(kHalo >= 4, "the circles reach 4 px from the pixel under test");

// slice_sort_kernel's workgroup shape (corner_sort.hip); the host sizes its dedup bitmap
// (CornerGeom::dedup_words) and its dynamic LDS from it.
constexpr int kSortThreads = 1024;
constexpr int kSortEPT = 16;
constexpr int kSortChunk = kSortThreads * kSortEPT;
// Event slots without an event (past the slice's end, or dropped by the dedup) are data, not a
// saved exec mask per unrolled slot: they count into kSortSent sentinel bins after the real ones
// (one per LDS bank, so the lanes of a wave do not pile on one address).  The scan runs over the
// sentinel bins too, so they start at `kept` and a chunk's 16384 slots fill the staging area
// exactly: the histogram add and the placement run unpredicated, the sentinel slots landing
// past the kept keys, where nothing reads them.
constexpr int kSortSent = 32;

constexpr int kRecVals = 4;  // values a pixel record holds inline (pair_build_kernel)
constexpr int kPairWords = kGroup * kTilePix / 32;  // 196: one bit per (slice, tile pixel)
constexpr int kSegWords = (kTilePix + 31) / 32;     // 7: one slice's 196 bits of a tile

struct CornerGeom {
    int W, H, S, margin, border_mode, first_detect;
    int any_order;         // timestamps in any order: every group wide (index values, exact tests)
    int dedup_words;       // slice_sort's dedup bitmap: n_tiles * 196 bits (0: off, too large)
    int tiles_x, n_tiles;  // bin n_tiles of each group holds the events outside the sensor
    int seg_stride;        // words per slice of the slice-major corner pairs: n_tiles * 7, to 16 B
    float inv_S;
    // item -> (group, tile) and tile -> (row, column) without a runtime division (MagicDiv)
    uint32_t nt_mul, nt_sh, tx_mul, tx_sh;
    int64_t n, n_slices;
};

// Batch sorted per slice by tile: slice s keeps its own range [s*S, s*S + len_s), and tile b of
// slice s is [s*S + toff[s][b], s*S + toff[s][b+1]) (row length n_tiles + 2: the outside-sensor
// bin n_tiles, then len_s).  A (group, tile) item's events are the 32 segments of its slices.
struct Sorted {
    uint32_t *key;   // (event index - first event of the group) << 8 | pixel in tile
    uint32_t *t32;   // t - t(first event of the group), written for groups spanning < 2^32 - 1
    int32_t *toff;   // [n_slices][n_tiles + 2]
};

// The group's constants, written once per call by slice_sort's workgroup of the group's first
// slice (which holds every input) and read by pair_build and the arc kernels with one scalar
// load (each of their waves used to rebuild them from two dependent loads of t).  slice_sort
// itself computes its own verdicts: its other workgroups may run before the writer.
struct GroupRec {
    int64_t first, t_first, Lt;
    uint32_t dlt;
    uint32_t bits;  // kRecNarrow: GroupRef::narrow; kRecFmt4: group_fmt4.  kRecNarrow32 (group_narrow)
                    // and kRecBeyond (beyond_double) complete the record but have no reader yet:
                    // only slice_sort needs them, and it computes its own (one thread per group pays)
};
static_assert(sizeof(GroupRec) == 32, "one 32-B scalar load");
constexpr uint32_t kRecNarrow = 1u, kRecFmt4 = 2u, kRecNarrow32 = 4u, kRecBeyond = 8u;

struct GroupImages {
    uint32_t *mask;       // [n_groups][H*W] slices of the group that touched the pixel
    int64_t *B;           // [n_groups][H*W] last t of the group, then (in place) B_g
    uint32_t *res;        // [n_groups][32][n_tiles][kSegWords] corner (slice, pixel) pairs, slice-major
    uint4 *pv;            // [n_groups][H*W] value record of each (group, pixel) (pair_build)
    uint32_t *ovf;        // [n] the values past a record's first three, in each item's part of the range
    int64_t *over;        // [n_items] items arc_kernel leaves to arc_dense_kernel (heavy or undecidable)
    uint32_t *n_over;     // [0]: their count
    GroupRec *grec;       // [n_groups] the groups' constants (slice_sort writes, the later kernels read)
};

// One host function per launch, each in the file that defines its kernel; the driver
// (fast_detect_phases) calls them in pipeline order on one stream.  Those that may have to raise
// a kernel's dynamic LDS limit return a status.
int launch_sort(ecc_ctx *ctx, hipStream_t s, const uint32_t *xy, const int64_t *t, const CornerGeom &g,
                const Sorted &so, int32_t *first_border, int32_t tag, uint32_t *zero0, int32_t *zero1,
                GroupRec *grec);
void launch_pair_build(ecc_ctx *ctx, hipStream_t s, const int64_t *t, const CornerGeom &g, int64_t n_items,
                       const Sorted &so, const GroupImages &gi);
void launch_sae_local_last(ecc_ctx *ctx, hipStream_t s, const CornerGeom &g, int64_t n_groups, const GroupImages &gi,
                           int64_t *local_last);
void launch_sae_prefix(ecc_ctx *ctx, hipStream_t s, const CornerGeom &g, int64_t n_groups, const GroupImages &gi,
                       int64_t *sae, int32_t tag, uint32_t *zero0, int32_t *zero1);
void launch_arc(ecc_ctx *ctx, hipStream_t s, const CornerGeom &g, int64_t n_items, const GroupImages &gi);
void launch_arc_dense(ecc_ctx *ctx, hipStream_t s, const int64_t *t, const CornerGeom &g, const GroupImages &gi);
int launch_flags(ecc_ctx *ctx, hipStream_t s, const uint32_t *xy, const CornerGeom &g, const GroupImages &gi,
                 const int32_t *first_border, uint8_t *corner_flags, uint32_t *cand, int32_t *n_cand);

}  // namespace corner
}  // namespace ecc

namespace {

using namespace ecc::corner;

// item = group * n_tiles + tile (n_items < 2^31: host check)
__device__ __forceinline__ void item_decode(const CornerGeom &g, int64_t item, int64_t &grp, int &tile) {
    const uint32_t q = magic_quot((uint32_t)item, g.nt_mul, g.nt_sh);
    grp = q;
    tile = (int)((uint32_t)item - q * (uint32_t)g.n_tiles);
}

__device__ __forceinline__ bool is_border(int x, int y, const CornerGeom &g) {
    return x < g.margin || x >= g.W - g.margin || y < g.margin || y >= g.H - g.margin;
}

__device__ __forceinline__ int tile_of(uint32_t v, const CornerGeom &g) {
    const int x = ecc::xy_x(v), y = ecc::xy_y(v);
    // a select, not a branch; y / 14 and tiles_x are below 2^13: a 24-bit multiply
    const int tl = (int)__umul24((uint32_t)(y / kTile), (uint32_t)g.tiles_x) + x / kTile;
    return (x >= g.W || y >= g.H) ? g.n_tiles : tl;
}

__device__ __forceinline__ uint32_t tile_key(uint32_t v, uint32_t e_local) {
    return (e_local << 8) | (uint32_t)((ecc::xy_y(v) % kTile) * kTile + ecc::xy_x(v) % kTile);
}

// tile = ty * tiles_x + tx
__device__ __forceinline__ void tile_origin_xy(const CornerGeom &g, int tile, int &tx, int &ty) {
    ty = (int)magic_quot((uint32_t)tile, g.tx_mul, g.tx_sh);
    tx = tile - ty * g.tiles_x;
}
__device__ __forceinline__ void tile_origin(const CornerGeom &g, int tile, int &x0, int &y0) {
    int tx, ty;
    tile_origin_xy(g, tile, tx, ty);
    x0 = tx * kTile;
    y0 = ty * kTile;
}

// The reference compares the two streak-end neighbours as int64 but scans the arc in double
// (FCT/…group_track.cpp:977-990, :1024-1036).  Below 2^53 ticks the conversion is exact and the
// whole test is an integer one; from 2^53 upward neighbouring timestamps round together and
// `tj >= min_t` can hold in double where it does not in int64.  A group that reaches that range is
// therefore never narrow: every test of it takes the exact path, which orders the values as the
// reference's doubles do (double_key).  No stream below 2^53 changes path.
constexpr int64_t kDoubleExact = (int64_t)1 << 53;
__device__ __forceinline__ bool beyond_double(int64_t t_first, int64_t t_last) {
    return t_last >= kDoubleExact || t_first <= -kDoubleExact;
}

// The group's events span < 2^32 - 1 ticks: t - t(first event) fits a u32 (+1 still fits).
__device__ __forceinline__ bool group_narrow(const int64_t *__restrict__ t, const CornerGeom &g, int64_t grp,
                                             int64_t *t_first) {
    const int64_t first = grp * kGroup * (int64_t)g.S;
    const int64_t end = (grp + 1) * kGroup * (int64_t)g.S;
    *t_first = t[first];
    if (g.any_order) return false;
    return (uint64_t)(t[(end < g.n ? end : g.n) - 1] - *t_first) < 0xffffffffull;
}

// Groups spanning < 2^24 - 1 ticks (the common case: 524288 events in under 16.7 s) are sorted
// into ONE 4-byte key per event, (t - t(first event of the group)) << 8 | pixel in tile: the
// slice an event belongs to is the slice segment it is read from.  Other groups keep the event
// index in the key and the relative timestamp in t32.
__device__ __forceinline__ bool group_fmt4(const int64_t *__restrict__ t, const CornerGeom &g, int64_t grp) {
    const int64_t first = grp * kGroup * (int64_t)g.S;
    const int64_t end = (grp + 1) * kGroup * (int64_t)g.S;
    if (g.any_order) return false;
    const int64_t t_first = t[first], t_last = t[(end < g.n ? end : g.n) - 1];
    if (beyond_double(t_first, t_last)) return false;  // wide (group_ref): the keys keep the event index
    return (uint64_t)(t_last - t_first) < 0xFFFFFFull;
}

// floor(el / S) for el < 2^24 (float estimate, then exact correction).
__device__ __forceinline__ int slice_in_group(uint32_t el, const CornerGeom &g) {
    uint32_t q = (uint32_t)((float)el * g.inv_S);
    const uint32_t S = (uint32_t)g.S;
    q = (q * S > el) ? q - 1 : q;
    q = ((q + 1) * S <= el) ? q + 1 : q;
    return (int)q;
}

// The 32 slice segments of one (group, tile) item, built by wave 0 into LDS (caller syncs):
// segment r = slice grp*32 + r; events are addressed by a flattened index i in [0, pref[32]).
// base = sum over the slices of toff[s][tile] = the item's offset inside the group's range when
// the group's items are laid out in tile order (used for its pair entries).
struct TileSegs {
    int64_t start[kGroup];
    int32_t pref[kGroup + 1];
    int64_t base;
};

__device__ __forceinline__ void tile_segs(const CornerGeom &g, const Sorted &so, int64_t grp, int tile, TileSegs &T) {
    const int tid = threadIdx.x;
    if (tid >= 64) return;
    const int64_t s = grp * kGroup + tid;
    int a = 0, len = 0;
    if (tid < kGroup && s < g.n_slices) {
        const int32_t *row = so.toff + s * (int64_t)(g.n_tiles + 2);
        a = row[tile];
        len = row[tile + 1] - a;
    }
    const int incl = ecc::wave_incl_scan(len);         // DPP (wave 0: all 64 lanes)
    const int asum = ecc::wave_sum_i32(a);  // < 32 * S <= 2^24: a 32-bit sum
    if (tid < kGroup) {
        T.start[tid] = s * g.S + a;
        T.pref[tid + 1] = incl;
    }
    if (tid == 0) {
        T.pref[0] = 0;
        T.base = asum;
    }
}

__device__ __forceinline__ int64_t seg_at(const TileSegs &T, int i, int &r) {
    r = 0;
#pragma unroll
    for (int step = kGroup / 2; step > 0; step >>= 1)
        if (T.pref[r + step] <= i) r += step;
    return T.start[r] + (i - T.pref[r]);
}

// Group time reference: L = t_last(group) - (2^27 - 1).  In a narrow group (span < 2^27 - 1
// ticks) every value v of the group maps exactly to v' = v - L in [1, 2^27 - 1]; in a wide group
// the stored value is the event index within the group + 1 (the exact test gathers t).
constexpr int kVBits = 27;
constexpr uint32_t kVMax = (1u << kVBits) - 1u;

struct GroupRef {
    int64_t first, t_first, Lt;
    bool narrow;
    uint32_t dlt;  // t32 + dlt = t - Lt (narrow)
};

__device__ __forceinline__ GroupRef group_ref(const int64_t *__restrict__ t, const CornerGeom &g, int64_t grp) {
    GroupRef r;
    r.first = grp * kGroup * (int64_t)g.S;
    const int64_t end = (grp + 1) * kGroup * (int64_t)g.S;
    r.t_first = t[r.first];
    const int64_t t_last = t[(end < g.n ? end : g.n) - 1];
    // (in uint64: a group that ends within 2^27 of INT64_MIN is beyond double and never reads Lt, but
    // the subtraction must not overflow a signed type)
    r.Lt = (int64_t)((uint64_t)t_last - (uint64_t)kVMax);
    // any order: the span of the first and last timestamps says nothing about the others
    // (the span is taken only below 2^53 in magnitude: no overflow)
    r.narrow = !g.any_order && !beyond_double(r.t_first, t_last) && t_last - r.t_first < (int64_t)kVMax;
    r.dlt = r.narrow ? (uint32_t)(r.t_first - r.Lt) : 0u;
    return r;
}

__device__ __forceinline__ GroupRec group_rec_make(const int64_t *__restrict__ t, const CornerGeom &g, int64_t grp) {
    const GroupRef r = group_ref(t, g, grp);
    int64_t t_first;
    GroupRec rec;
    rec.first = r.first;
    rec.t_first = r.t_first;
    rec.Lt = r.Lt;
    rec.dlt = r.dlt;
    rec.bits = (r.narrow ? kRecNarrow : 0u) | (group_fmt4(t, g, grp) ? kRecFmt4 : 0u) |
               (group_narrow(t, g, grp, &t_first) ? kRecNarrow32 : 0u) |
               (beyond_double(r.t_first, (int64_t)((uint64_t)r.Lt + (uint64_t)kVMax)) ? kRecBeyond : 0u);
    return rec;
}

__device__ __forceinline__ void group_rec_store(const int64_t *__restrict__ t, const CornerGeom &g, int64_t grp,
                                                GroupRec *__restrict__ grec) {
    grec[grp] = group_rec_make(t, g, grp);
}

__device__ __forceinline__ GroupRef group_ref_of(const GroupRec &rec) {
    GroupRef r;
    r.first = rec.first;
    r.t_first = rec.t_first;
    r.Lt = rec.Lt;
    r.narrow = (rec.bits & kRecNarrow) != 0u;
    r.dlt = rec.dlt;
    return r;
}

}  // namespace
