// Greedy box NMS per slice.
//
// Reference: CornerFilter::filterCorners, FCT/…group_track.cpp:81-152 — a H×W u8 mask
// (cv::Mat::zeros per call), corners visited in detection order, a corner is kept iff no mask
// pixel inside its clipped box [x±7]×[y±7] is set, and a kept corner paints its box
// (cv::rectangle filled).  Called once per 16384-event slice (:832-837).
//
// MI355X design: one workgroup per slice, every slice of a batch in ONE launch.  The slice's
// corner flags (16 KiB) are read with 16-B loads and compacted in event order into LDS; the
// greedy pass then runs on one wave without any mask image: "box touches a painted pixel"
// == "box intersects the box of an earlier kept corner" (kept boxes are the painted set).
// Candidates are processed 64 at a time: each lane tests its candidate against the kept list
// (LDS broadcast reads), then the within-chunk order dependency is resolved on a 64x64
// overlap bitmask with scalar bit logic.  Output label = rank in the kept list (:140).
//
// Grid form (used whenever the grid fits LDS): two boxes [c±h] overlap iff their centres are
// within Chebyshev distance 2h (clipping to the image never separates two boxes whose centres
// lie inside it), so kept boxes are pairwise disjoint and a grid of (2h+1)-pixel cells holds at
// most ONE kept centre per cell.  "Overlaps an earlier kept box" is then 9 LDS probes.  A
// parallel compaction kernel (256 lanes per slice) first lists each slice's flagged events in
// event order; one wave per slice then takes them 64 at a time, and within a chunk the kept ones
// are found by a scalar loop over the surviving lanes (each kept lane's centre is broadcast and
// kills the later lanes it overlaps).  ~4 KiB of LDS per slice at the bench's sizes (grid and
// kept list), so many slices run per CU.
#include "ecc_internal.hpp"
#include "nms_cell.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCand = 16384;  // LDS candidate list (64 KiB)
constexpr int kMaxKept = 8192;   // LDS kept list (boxes are disjoint => <= W*H/144)

struct Box { int16_t x0, x1, y0, y1; };

__device__ __forceinline__ Box make_box(uint32_t v, int half, int W, int H) {
    const int x = ecc::xy_x(v), y = ecc::xy_y(v);
    Box b;
    b.x0 = (int16_t)max(0, x - half);     // :114-117
    b.x1 = (int16_t)min(W - 1, x + half);
    b.y0 = (int16_t)max(0, y - half);
    b.y1 = (int16_t)min(H - 1, y + half);
    return b;
}

__device__ __forceinline__ bool overlap(const Box &a, const Box &b) {
    return a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1;
}

__global__ void __launch_bounds__(kThreads)
nms_kernel(const uint32_t *__restrict__ xy, const uint8_t *__restrict__ flags, int64_t n, int S,
           int W, int H, int half, int cap, ecc_corner *__restrict__ out,
           int32_t *__restrict__ out_count, int32_t *__restrict__ err) {
    __shared__ uint32_t cand[kMaxCand];
    __shared__ Box kept[kMaxKept];
    __shared__ int wave_tot[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = blockIdx.x;
    const int64_t lo = s * (int64_t)S;
    const int64_t hi = (lo + S < n) ? lo + S : n;
    const int64_t len = hi - lo;

    // 1. compaction of flagged events in event order, in chunks of 256*16 events
    int n_cand = 0;
    // 16-B flag loads where the slice's first ADDRESS is 16-B aligned (my0 is a multiple of 16)
    const bool vec = ((reinterpret_cast<uintptr_t>(flags) + lo) & 15) == 0;  // uniform
    for (int64_t c0 = 0; c0 < len; c0 += kThreads * 16) {
        const int64_t my0 = c0 + (int64_t)tid * 16;
        uint32_t bits = 0;
        if (my0 + 15 < len && vec) {
            const uint4 q = *reinterpret_cast<const uint4 *>(flags + lo + my0);
            const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) bits |= (((w4[k >> 2] >> (8 * (k & 3))) & 0xffu) ? 1u : 0u) << k;
        } else {
            for (int k = 0; k < 16; ++k)
                if (my0 + k < len && flags[lo + my0 + k]) bits |= 1u << k;
        }
        const int cntv = __popc(bits);
        // wave inclusive scan of cntv
        const int incl = ecc::wave_incl_scan(cntv);  // DPP
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int off = n_cand + incl - cntv, tot = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wave) off += wave_tot[w];
            tot += wave_tot[w];
        }
        while (bits) {
            const int k = __ffs(bits) - 1;
            bits &= bits - 1;
            if (off < kMaxCand) cand[off] = xy[lo + my0 + k];
            ++off;
        }
        n_cand += tot;
        __syncthreads();
    }
    if (n_cand > kMaxCand) n_cand = kMaxCand;  // cannot happen when S <= kMaxCand
    __syncthreads();
    // 2. greedy NMS on wave 0 (the other waves only keep the barriers uniform)
    int n_kept = 0;
    bool overflow = false;
    for (int c0 = 0; c0 < n_cand; c0 += 64) {
        if (wave == 0) {
            const int ci = c0 + lane;
            const bool valid = ci < n_cand;
            const uint32_t v = valid ? cand[ci] : 0u;
            const Box b = make_box(v, half, W, H);
            bool alive = valid;
            for (int k = 0; k < n_kept && alive; ++k)
                if (overlap(b, kept[k])) alive = false;
            // within-chunk dependency: ov = lanes j < lane whose box overlaps mine
            uint64_t ov = 0;
            for (int j = 0; j < 64; ++j) {
                const int x0 = __shfl((int)b.x0, j), x1 = __shfl((int)b.x1, j);
                const int y0 = __shfl((int)b.y0, j), y1 = __shfl((int)b.y1, j);
                const bool o = (j < lane) && x0 <= b.x1 && b.x0 <= x1 && y0 <= b.y1 && b.y0 <= y1;
                ov |= (uint64_t)o << j;
            }
            uint64_t alive_m = __ballot(alive);
            uint64_t acc = 0;
            while (alive_m) {
                const int i = __ffsll((unsigned long long)alive_m) - 1;
                alive_m &= alive_m - 1;
                const uint64_t ov_i = __shfl(ov, i);
                if ((ov_i & acc) == 0) acc |= 1ull << i;
            }
            const bool keep = (acc >> lane) & 1ull;
            const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
            const int rank = n_kept + __popcll(acc & lt);
            if (keep) {
                if (rank < kMaxKept) kept[rank] = b;
                else overflow = true;
                if (rank < cap) out[s * (int64_t)cap + rank] = ecc_corner{ecc::xy_x(v), ecc::xy_y(v), rank};
                else overflow = true;
            }
            n_kept += __popcll(acc);
            if (n_kept > kMaxKept) n_kept = kMaxKept;
        }
        __syncthreads();  // orders the kept[] LDS writes before the next chunk's reads
    }
    if (wave != 0) return;
    overflow = __any(overflow);
    if (lane == 0) {
        out_count[s] = n_kept < cap ? n_kept : cap;
        if (overflow) atomicOr(err, 1);
    }
}


constexpr int kGridMaxCells = 16384;  // 64 KiB of LDS

__device__ __forceinline__ bool near_centre(uint32_t a, uint32_t b, int reach) {
    return abs(ecc::xy_x(a) - ecc::xy_x(b)) <= reach && abs(ecc::xy_y(a) - ecc::xy_y(b)) <= reach;
}

// Two-kernel grid form (bench sizes): candidates first, greedy second.
// nms_compact_kernel: one 256-lane workgroup per slice (chunks of 4096 events): 16-B flag loads,
// a block scan of the per-lane flag counts, and the flagged events' xy gathered into the slice's
// candidate list in event order (cand[s*S ...], count n_cand[s]).
constexpr int kCompactThreads = 256;

__global__ void __launch_bounds__(kCompactThreads)
nms_compact_kernel(const uint32_t *__restrict__ xy, const uint8_t *__restrict__ flags, int64_t n, int S,
                   uint32_t *__restrict__ cand, int32_t *__restrict__ n_cand) {
    __shared__ int wtot[kCompactThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = blockIdx.x;
    const int64_t lo = s * (int64_t)S;
    const int64_t len = ((lo + S < n) ? lo + S : n) - lo;
    int run = 0;
    // 16-B aligned slices: one unconditional 16-B load per lane through a buffer view of the
    // slice rounded up to 16 B (the slice starts on a 16-B boundary in this arm, so the round-up ends
    // with the 16-B block of its last byte; bytes past len are masked) -- a per-lane choice of load
    // form waited for every load
    const bool vec = ((reinterpret_cast<uintptr_t>(flags) + lo) & 15) == 0;  // uniform
    const __amdgpu_buffer_rsrc_t vf = ecc::buffer_view(flags + lo, (uint32_t)((len + 15) & ~15ll));
    for (int64_t c0 = 0; c0 < len; c0 += kCompactThreads * 16) {
        const int64_t my0 = c0 + (int64_t)tid * 16;
        uint32_t bits = 0;
        if (vec) {
            const uint4 q = ecc::buffer_load_u128(vf, (uint32_t)my0);
            const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                bits |= (((w4[k >> 2] >> (8 * (k & 3))) & 0xffu) && my0 + k < len ? 1u : 0u) << k;
        } else {
            for (int k = 0; k < 16; ++k)
                if (my0 + k < len && flags[lo + my0 + k]) bits |= 1u << k;
        }
        const int cnt = __popc(bits);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int off = run + incl - cnt, tot = 0;
#pragma unroll
        for (int w = 0; w < kCompactThreads / 64; ++w) {
            off += w < wave ? wtot[w] : 0;
            tot += wtot[w];
        }
        while (bits) {
            const int k = __ffs(bits) - 1;
            bits &= bits - 1;
            cand[lo + off++] = xy[lo + my0 + k];
        }
        run += tot;
        __syncthreads();
    }
    if (tid == 0) n_cand[s] = run;
}

// ---- the greedy pass over the candidate lists ---------------------------------------------------
// One workgroup per slice takes its list in batches of 64 x waves (the next batch is requested
// before this one is decided); the kept-centre grid as described at the top of the file.
// Build switches (measured alone and together, profiles/nms_batch_ab.txt):
//   ECC_NMS_WAVES  waves per slice.  1: a batch is one chunk of 64, probed and decided by the one
//                  wave.  More: every lane probes one candidate of the batch against the grid as it
//                  stood before the batch, the survivors are listed in candidate order, and wave 0
//                  alone runs the greedy chunk code over that list.  On the bench stream a slice's
//                  first 256 candidates meet an empty grid and all survive, so 2, 4 and 8 waves
//                  measured slower than one: 1 is the default.
//   ECC_NMS_LEAN   1: cell by multiply-high, nine unguarded probes and the keep loop's reach test
//                  as one unsigned compare (nms_cell.hpp), the first batch's loads issued beside
//                  the n_cand load, kept centres listed in LDS and written out after the loop.
//                  0: the divisions, guarded probes and in-loop stores of the pass as it was.
#ifndef ECC_NMS_WAVES
#define ECC_NMS_WAVES 1
#endif
#ifndef ECC_NMS_LEAN
#define ECC_NMS_LEAN 1
#endif
constexpr int kNmsWaves = ECC_NMS_WAVES;
constexpr bool kNmsLean = ECC_NMS_LEAN != 0;
static_assert(kNmsWaves >= 1 && kNmsWaves <= 16, "ECC_NMS_WAVES: 1 .. 16");

template <bool LEAN>
__device__ __forceinline__ bool cell_free(const uint32_t *grid, int c0, int pw, uint32_t v, int reach) {
    uint32_t kc[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) kc[d] = grid[c0 + (d / 3) * pw + d % 3];
    if constexpr (LEAN) {
        const NmsKey k = nms_key(v, reach);
        uint32_t nearest = UINT32_MAX;  // an empty cell is out of every reach (nms_cell.hpp)
#pragma unroll
        for (int d = 0; d < 9; ++d) nearest = min(nearest, nms_span(k, kc[d]));
        return nearest > 2u * (uint32_t)reach;
    } else {
        bool free_ = true;
#pragma unroll
        for (int d = 0; d < 9; ++d) free_ &= !(kc[d] != kNoCentre && near_centre(kc[d], v, reach));
        return free_;
    }
}

// One workgroup of WAVES waves per slice.  LDS: the padded grid, then (WAVES > 1) the waves'
// survivor lists of 64 {xy, cell} pairs and their counts, then (LDS_OUT) the kept centres in rank
// order, kl <= cap of them (at most one per cell, so gw * gh bound the list), and one word for the
// kept count.  A candidate that the batch probe drops lies within reach of a centre that is final;
// the greedy pass drops it whatever follows and a dropped candidate influences nobody, so wave 0's
// pass over the survivors in unchanged order keeps the same centres at the same ranks.
template <int WAVES, bool LEAN, bool LDS_OUT>
__global__ void __launch_bounds__(64 * WAVES)
nms_batch_kernel(const uint32_t *__restrict__ cand, const int32_t *__restrict__ n_cand, int64_t n, int S, int W, int H,
                 int half, int gw, int gh, int cap, int kl, uint32_t cell_mul, uint32_t cell_sh,
                 ecc_corner *__restrict__ out, int32_t *__restrict__ out_count, int32_t *__restrict__ err) {
    constexpr int NT = 64 * WAVES;
    extern __shared__ uint32_t grid[];  // [gh + 2][gw + 2] kept centre per cell
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t s = blockIdx.x;
    const int64_t lo = s * (int64_t)S;
    const int len = (int)((lo + S < n ? lo + S : n) - lo);  // >= 1: the slice exists
    const uint32_t *c = cand + lo;
    const int cs = 2 * half + 1, reach = LEAN ? nms_reach(half) : 2 * half;
    const int pw = gw + 2;
    const int cells = pw * (gh + 2);
    uint2 *surv = reinterpret_cast<uint2 *>(grid + ((cells + 1) & ~1));  // [WAVES][64]
    uint32_t *wcnt = reinterpret_cast<uint32_t *>(surv + (WAVES > 1 ? NT : 0));  // [WAVES]
    uint32_t *keptl = wcnt + (WAVES > 1 ? WAVES : 0);                            // [kl]
    uint32_t *n_kept_all = keptl + (LDS_OUT ? kl : 0);
    // LEAN: the slice owns len slots of cand, so its first batch is read (clamped) without waiting
    // for its count
    uint32_t nxt = 0u;
    if constexpr (LEAN) nxt = c[min(tid, len - 1)];
    const int total = min(max(n_cand[s], 0), len);
    if constexpr (!LEAN) nxt = tid < total ? c[tid] : 0u;
    for (int i = tid; i < cells; i += NT) grid[i] = kNoCentre;
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int n_kept = 0;  // wave 0's
    bool overflow = false, bad_input = false;
    __syncthreads();
    // wave 0 (wave-uniform): the greedy step over 64 candidates v at cells c0, `alive` those that no
    // earlier kept centre reaches
    auto resolve = [&](uint32_t v, int c0, bool alive) {
        uint64_t am = __ballot(alive), keepm = 0;
        const NmsKey key = nms_key(v, reach);
        while (am) {  // each step keeps the first surviving lane
            const int i0 = __ffsll((unsigned long long)am) - 1;
            keepm |= 1ull << i0;
            am &= am - 1;
            const uint32_t vi = (uint32_t)__builtin_amdgcn_readlane((int)v, i0);
            // (LEAN: am holds lanes above i0 only, so the lanes need not say where they are)
            if constexpr (LEAN) am &= ~__ballot(nms_span(key, vi) <= 2u * (uint32_t)reach);
            else am &= ~__ballot(lane > i0 && near_centre(vi, v, reach));
        }
        if ((keepm >> lane) & 1ull) {
            const int rank = n_kept + __popcll(keepm & lt_mask);
            grid[c0 + pw + 1] = v;
            if constexpr (LDS_OUT) {
                if (rank < kl) keptl[rank] = v;
                if (rank >= cap) overflow = true;
            } else {
                if (rank < cap) out[s * (int64_t)cap + rank] = ecc_corner{ecc::xy_x(v), ecc::xy_y(v), rank};
                else overflow = true;
            }
        }
        n_kept += __popcll(keepm);
    };
    for (int b0 = 0; b0 < total; b0 += NT) {
        uint32_t v = nxt;
        const bool have = b0 + tid < total;
        if constexpr (LEAN) nxt = c[min(b0 + NT + tid, len - 1)];
        else nxt = (b0 + NT + tid < total) ? c[b0 + NT + tid] : 0u;
        int x = ecc::xy_x(v), y = ecc::xy_y(v);
        const bool outside = have && (x >= W || y >= H);
        if (outside) bad_input = true;  // skipped and reported (ecc_corner_nms_status)
        const bool valid = have && !outside;
        if (!valid) { v = 0u; x = 0; y = 0; }
        const int cx = LEAN ? (int)magic_quot((uint32_t)x, cell_mul, cell_sh) : x / cs;
        const int cy = LEAN ? (int)magic_quot((uint32_t)y, cell_mul, cell_sh) : y / cs;
        const int c0 = cy * pw + cx;  // padded cell (cx, cy) - (1, 1)
        const bool alive = valid && cell_free<LEAN>(grid, c0, pw, v, reach);
        if constexpr (WAVES == 1) {
            resolve(v, c0, alive);
        } else {
            const uint64_t am = __ballot(alive);
            if (alive) surv[wave * 64 + __popcll(am & lt_mask)] = make_uint2(v, (uint32_t)c0);
            if (lane == 0) wcnt[wave] = (uint32_t)__popcll(am);
            __syncthreads();
            if (wave == 0) {
                int first[WAVES + 1];  // survivor i of the batch is wave w's (i - first[w])-th
                first[0] = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) first[w + 1] = first[w] + (int)wcnt[w];
                const int tot = first[WAVES];
                for (int q0 = 0; q0 < tot; q0 += 64) {
                    const int i = q0 + lane;
                    int src = i;
#pragma unroll
                    for (int w = 1; w < WAVES; ++w) src += i >= first[w] ? 64 - (first[w] - first[w - 1]) : 0;
                    const bool have2 = i < tot;
                    const uint2 e = surv[have2 ? src : 0];
                    // the chunk before this one may have kept a centre within reach
                    const bool alive2 = have2 && (q0 == 0 || cell_free<LEAN>(grid, (int)e.y, pw, e.x, reach));
                    resolve(e.x, (int)e.y, alive2);
                }
            }
        }
        __syncthreads();
    }
    if (__any(bad_input) && lane == 0) atomicOr(err, 2);
    if constexpr (LDS_OUT) {
        if (tid == 0) *n_kept_all = (uint32_t)n_kept;
        __syncthreads();
        const int m = min(min((int)*n_kept_all, cap), kl);
        for (int r = tid; r < m; r += NT) {
            const uint32_t v = keptl[r];
            out[s * (int64_t)cap + r] = ecc_corner{ecc::xy_x(v), ecc::xy_y(v), r};
        }
    }
    if (wave != 0) return;
    overflow = __any(overflow);
    if (lane == 0) {
        out_count[s] = n_kept < cap ? n_kept : cap;
        if (overflow) atomicOr(err, 1);
    }
}

// Packs per-slice corner lists (slice s at in[s * cap], counts[s] <= cap) densely at
// out[offsets[s]]: one workgroup per slice.
__global__ void __launch_bounds__(256)
corner_pack_kernel(const ecc_corner *__restrict__ in, const int32_t *__restrict__ counts, int cap,
                   const int64_t *__restrict__ offsets, ecc_corner *__restrict__ out) {
    const int64_t s = blockIdx.x;
    const int c = min(max(counts[s], 0), cap);
    const int64_t o = offsets[s];
    for (int d = threadIdx.x; d < c; d += 256) out[o + d] = in[s * cap + d];
}

}  // namespace

namespace ecc {
int nms_check_args(int64_t n, int32_t slice_events, int32_t width, int32_t height, int32_t box_size, int32_t cap) {
    if (n < 0 || slice_events < 1 || slice_events > kMaxCand || width < 1 || height < 1 || width > 32767 ||
        height > 32767 || box_size < 1 || cap < 0)
        return ECC_ERR_INVALID;
    return ECC_OK;
}

int nms_candidates(ecc_ctx *ctx, int64_t n, int32_t slice_events, int32_t width, int32_t height, int32_t box_size,
                   uint32_t **cand, int32_t **n_cand) {
    *cand = nullptr;
    *n_cand = nullptr;
    const int cs = 2 * (box_size / 2) + 1;
    const int gw = (width + cs - 1) / cs, gh = (height + cs - 1) / cs;
    if ((int64_t)(gw + 2) * (gh + 2) > kGridMaxCells) return ECC_OK;  // the one-kernel form takes it
    const int64_t n_slices = (n + slice_events - 1) / slice_events;
    // candidate lists: n xy words + n_slices counts, per context (grown, never shrunk)
    const size_t need = ecc::align_up((size_t)n * 4, 256) + (size_t)n_slices * 4;
    if (need > ctx->nms_buf.bytes)
        if (int rc = buf_reserve(ctx, ctx->nms_buf, ecc::align_up(need + need / 8, 1 << 20), "nms buffer")) return rc;
    char *buf = static_cast<char *>(ctx->nms_buf.p);
    *cand = reinterpret_cast<uint32_t *>(buf);
    *n_cand = reinterpret_cast<int32_t *>(buf + ecc::align_up((size_t)n * 4, 256));
    return ECC_OK;
}

int nms_greedy(ecc_ctx *ctx, const uint32_t *cand, const int32_t *n_cand, int64_t n, int32_t slice_events,
               int32_t width, int32_t height, int32_t box_size, int32_t cap, ecc_corner *out, int32_t *out_count,
               hipStream_t s) {
    const int64_t n_slices = (n + slice_events - 1) / slice_events;
    const int half = box_size / 2, cs = 2 * half + 1;
    const int gw = (width + cs - 1) / cs, gh = (height + cs - 1) / cs;
    // LDS: grid (an even count of words), survivor lists and counts, kept list and count
    const size_t base = (size_t)(((gw + 2) * (gh + 2) + 1) & ~1) * 4 + (kNmsWaves > 1 ? kNmsWaves * (64 * 8 + 4) : 0);
    const int kl = (int)std::min<int64_t>(cap, (int64_t)gw * gh);
    const bool lds_out = kNmsLean && base + (size_t)kl * 4 + 4 <= 65536;  // else the loop stores to out[]
    const size_t lds = lds_out ? base + (size_t)kl * 4 + 4 : base;
    const auto fn = lds_out ? &nms_batch_kernel<kNmsWaves, kNmsLean, kNmsLean> : &nms_batch_kernel<kNmsWaves, kNmsLean, false>;
    if (lds > 65536)
        if (int rc = ecc::allow_dynamic_lds(ctx, fn, (int)lds, "nms LDS")) return rc;
    const MagicDiv md = magic_div31((uint32_t)cs);
    ECC_TIMED(ctx, s, "nms_kernel");
    hipLaunchKernelGGL(fn, dim3((unsigned)n_slices), dim3(64 * kNmsWaves), lds, s, cand, n_cand, n, slice_events, width,
                       height, half, gw, gh, cap, lds_out ? kl : 0, md.mul, md.sh, out, out_count, &ctx->dev->nms);
    return ECC_OK;
}
}  // namespace ecc

ECC_API int ecc_corner_nms(ecc_ctx *ctx, const uint32_t *xy, const uint8_t *corner_flags,
                           int64_t n, int32_t slice_events, int32_t width, int32_t height,
                           int32_t box_size, int32_t cap, ecc_corner *out, int32_t *out_count,
                           ecc_stream_t stream) {
    if (!ctx || ecc::nms_check_args(n, slice_events, width, height, box_size, cap)) return ECC_ERR_INVALID;
    if (n == 0) return ECC_OK;
    if (!xy || !corner_flags || !out_count || (cap > 0 && !out)) return ECC_ERR_INVALID;
    const int64_t n_slices = (n + slice_events - 1) / slice_events;
    if (n_slices > INT32_MAX) return ECC_ERR_INVALID;
    hipStream_t s = ecc::as_stream(stream);
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    ECC_CHECK_HIP(ctx, hipMemsetAsync(&ctx->dev->nms, 0, 4, s), "memset(nms err)");
    uint32_t *cand = nullptr;
    int32_t *n_cand = nullptr;
    int rc = ecc::nms_candidates(ctx, n, slice_events, width, height, box_size, &cand, &n_cand);
    if (rc) return rc;
    if (cand) {
        {
            ECC_TIMED(ctx, s, "nms_compact_kernel");
            hipLaunchKernelGGL(nms_compact_kernel, dim3((unsigned)n_slices), dim3(kCompactThreads), 0, s, xy,
                               corner_flags, n, slice_events, cand, n_cand);
        }
        rc = ecc::nms_greedy(ctx, cand, n_cand, n, slice_events, width, height, box_size, cap, out, out_count, s);
        if (rc) return rc;
    } else {
        ECC_TIMED(ctx, s, "nms_kernel");
        hipLaunchKernelGGL(nms_kernel, dim3((unsigned)n_slices), dim3(kThreads), 0, s, xy,
                           corner_flags, n, slice_events, width, height, box_size / 2, cap, out,
                           out_count, &ctx->dev->nms);
    }
    ECC_CHECK_LAUNCH(ctx, "nms_kernel");
    return ECC_OK;
}

ECC_API int ecc_corner_pack(ecc_ctx *ctx, const ecc_corner *in, const int32_t *counts, int32_t n_slices,
                            int32_t cap, ecc_corner *out, int64_t *offsets, ecc_stream_t stream) {
    if (!ctx || n_slices < 0 || cap < 0 || !offsets || (n_slices > 0 && !counts)) return ECC_ERR_INVALID;
    if (n_slices > 0 && cap > 0 && (!in || !out)) return ECC_ERR_INVALID;
    hipStream_t s = ecc::as_stream(stream);
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    int rc = ecc::ws_reserve(ctx, ecc::scan_scratch_bytes(n_slices));
    if (rc) return rc;
    rc = ecc::exclusive_scan_i32_i64(ctx, counts, n_slices, offsets, reinterpret_cast<int64_t *>(ctx->ws), s);
    if (rc) return rc;
    if (n_slices == 0 || cap == 0) return ECC_OK;
    {
        ECC_TIMED(ctx, s, "corner_pack_kernel");
        hipLaunchKernelGGL(corner_pack_kernel, dim3((unsigned)n_slices), dim3(256), 0, s, in, counts, cap,
                           (const int64_t *)offsets, out);
    }
    ECC_CHECK_LAUNCH(ctx, "corner_pack");
    return ECC_OK;
}

ECC_API int ecc_corner_nms_status(ecc_ctx *ctx, ecc_stream_t stream) {
    if (!ctx) return ECC_ERR_INVALID;
    int32_t f = 0;
    if (int rc = ecc::read_dev_words(ctx, &ctx->dev->nms, 1, &f, ecc::as_stream(stream))) return rc;
    if (f & 2) return ECC_ERR_INVALID;
    return (f & 1) ? ECC_ERR_CAPACITY : ECC_OK;
}
