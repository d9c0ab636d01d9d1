// Corner detection, stages 3-4: the per-pixel value records of every (group, tile) item and the
// SAE prefix over the groups (pipeline: corners.hip); the plain SAE scatter and the max-combine
// of the multi-GPU hand-off.
#include "corner_common.hpp"

namespace {

constexpr int kBuildUnroll = 8;

// 3. Per (group, tile): the distinct (slice, pixel) pairs the tile's events touch, each with the
// value an arc test reads there (max over the slice's events at the pixel: v' or index + 1),
// stored PER PIXEL so that an arc workgroup stages a window pixel from its own fixed addresses,
// with no per-item offset table between its loads:
//   gmask[grp][q]  the slices that touched the pixel (bit j = slice j of the group),
//   pv[grp][q]     its values in ascending j: {v0, v1, v2, v3} when it has <= 4 of them, else
//                  {v0, v1, v2, x} with v3, v4, ... at ovf[4x], ovf[4x + 1], ... (16-B aligned, so
//                  an arc workgroup reads them as whole uint4s),
//   glast[grp][q]  its last timestamp.
// Item i's overflow values go to its own part of ovf: from (its place in the group's range with
// the group's items in tile order) + 4i, rounded up to 16 B.  A pixel with p > 4 values takes
// p - 3 rounded up to 4 words, at most p, and an item has at least as many events as pairs, so
// the 4 words per item cover the rounding and ovf needs n + 4 * n_items words.
__global__ void __launch_bounds__(kThreads)
pair_build_kernel(const int64_t *__restrict__ t, CornerGeom g, Sorted so, uint32_t *__restrict__ ovf,
                  uint4 *__restrict__ pv, uint32_t *__restrict__ gmask, int64_t *__restrict__ glast,
                  const GroupRec *__restrict__ grec) {
    __shared__ uint32_t tab[kGroup][kTilePix];  // 24.5 KiB
    __shared__ uint32_t pmask[kTilePix];        // slices that touched each tile pixel
    __shared__ int32_t wtot[kThreads / 64];
    __shared__ TileSegs segs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t item = blockIdx.x;
    int64_t grp;
    int tile;
    item_decode(g, item, grp, tile);
    const GroupRec rec = grec[grp];  // uniform: one scalar load
    const int lp = tid < kTilePix ? tid : 0;  // this lane's tile pixel
    {
        uint4 *z = reinterpret_cast<uint4 *>(&tab[0][0]);
        for (int i = tid; i < (int)(sizeof(tab) / 16); i += kThreads) z[i] = make_uint4(0u, 0u, 0u, 0u);
        if (tid < kTilePix) pmask[tid] = 0u;
    }
    tile_segs(g, so, grp, tile, segs);
    const GroupRef gr = group_ref_of(rec);
    const bool fmt4 = (rec.bits & kRecFmt4) != 0u;  // uniform; the same test as slice_sort's
    __syncthreads();
    const int total = segs.pref[kGroup];
    if (fmt4) {  // 4-byte keys: slice = the segment, value = relative t + dlt
        for (int i0 = 0; i0 < total; i0 += kBuildUnroll * kThreads) {
            uint32_t k[kBuildUnroll];
            int r[kBuildUnroll];
#pragma unroll
            for (int u = 0; u < kBuildUnroll; ++u) {
                const int i = i0 + u * kThreads + tid;
                const int64_t gi = (i < total) ? seg_at(segs, i, r[u]) : 0;
                k[u] = (i < total) ? so.key[gi] : 0xffffffffu;
            }
#pragma unroll
            for (int u = 0; u < kBuildUnroll; ++u) {
                if (k[u] == 0xffffffffu) continue;
                atomicMax(&tab[r[u]][k[u] & 255u], (k[u] >> 8) + gr.dlt);
                atomicOr(&pmask[k[u] & 255u], 1u << r[u]);
            }
        }
    } else {
        for (int i0 = 0; i0 < total; i0 += kBuildUnroll * kThreads) {
            uint32_t k[kBuildUnroll], tv[kBuildUnroll];
#pragma unroll
            for (int u = 0; u < kBuildUnroll; ++u) {
                const int i = i0 + u * kThreads + tid;
                int r_unused;
                const int64_t gi = (i < total) ? seg_at(segs, i, r_unused) : 0;
                k[u] = (i < total) ? so.key[gi] : 0xffffffffu;
                tv[u] = (i < total && gr.narrow) ? so.t32[gi] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kBuildUnroll; ++u) {
                if (k[u] == 0xffffffffu) continue;
                const uint32_t el = k[u] >> 8;
                const int jr = slice_in_group(el, g);
                atomicMax(&tab[jr][k[u] & 255u], gr.narrow ? tv[u] + gr.dlt : el + 1u);
                atomicOr(&pmask[k[u] & 255u], 1u << jr);
            }
        }
    }
    __syncthreads();
    // lane lp owns tile pixel lp: its slice mask, kept by one LDS atomicOr per event beside its
    // atomicMax (reading the pixel's 32 table words instead cost 32 LDS reads per pixel lane)
    const uint32_t m = tid < kTilePix ? pmask[lp] : 0u;
    const int cnt = __popc(m);
    const int nov = cnt > kRecVals ? (cnt - (kRecVals - 1) + 3) & ~3 : 0;  // past the first three, to 16 B
    const int incl = ecc::wave_incl_scan(nov);                  // DPP (all lanes active)
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int off = incl - nov;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    if (tid >= kTilePix) return;
    int x0, y0;
    tile_origin(g, tile, x0, y0);
    const int px = x0 + lp % kTile, py = y0 + lp / kTile;
    if (px >= g.W || py >= g.H) return;
    const int64_t q = grp * (int64_t)g.H * g.W + (int64_t)py * g.W + px;
    gmask[q] = m;
    if (!m) return;  // no slice touched it: arc workgroups never read its record
    // the pixel's overflow values at 16-B index x4 (off is a multiple of 4)
    const uint32_t x4 = (uint32_t)(((gr.first + segs.base + 4 * item + 3) >> 2) + (off >> 2));
    uint32_t *xo = ovf + 4 * (int64_t)x4 - (kRecVals - 1);
    static_assert(kRecVals == 4, "the record is one uint4");
    uint32_t r0 = 0u, r1 = 0u, r2 = 0u, r3 = x4;  // selects, not a register array indexed by k
    uint32_t v = 0u;
    int k = 0;
    for (uint32_t mm = m; mm; mm &= mm - 1u, ++k) {
        v = tab[__ffs(mm) - 1][lp];
        if (k == 0) r0 = v;
        else if (k == 1) r1 = v;
        else if (k == 2) r2 = v;
        else if (cnt == kRecVals) r3 = v;
        else xo[k] = v;
    }
    pv[q] = make_uint4(r0, r1, r2, r3);
    glast[q] = gr.narrow ? gr.Lt + (int64_t)v : t[gr.first + v - 1u];  // v: the newest slice's value
}

// 4. Per pixel, in place over the groups: gB[g] := B_g, the SAE before group g (the caller's
// `sae` for g = 0, then overwritten by the last event of every group that touched the pixel —
// the reference's `sae.at(y,x) = t`, :921-923); the caller's `sae` receives the final surface.
// The prefix is a "last value set" scan, which is associative: a workgroup takes 64 pixels (one
// per lane) and splits each run of 64 groups over its 4 waves (16 groups each); a wave finds the
// last value its groups set, the waves exchange those through LDS, and each then writes its
// groups' B_g from its incoming value.  (One thread per pixel walking all groups left 90 K
// threads for 256 CUs at 346x260: latency-bound at 31 us.)
constexpr int kPrefixPix = 64;
constexpr int kPrefixPer = 16;  // groups per wave per round
constexpr int kPrefixRound = kPrefixPer * (kThreads / 64);

__global__ void __launch_bounds__(kThreads)
sae_prefix_kernel(CornerGeom g, int64_t n_groups, const uint32_t *__restrict__ gmask, int64_t *__restrict__ gB,
                  int64_t *__restrict__ sae, int32_t *__restrict__ err_status,
                  int32_t *__restrict__ err_pending, int32_t tag,
                  uint32_t *__restrict__ zero0, int32_t *__restrict__ zero1) {
    // the call's sort verdict: its sort phase (finished before this kernel, in this call or in
    // the prepare it finishes) wrote its tag into the pending word iff it saw decreasing time;
    // publish it and consume the pending word (a captured graph replays the same tag, so each
    // replay must start from a clean word; a stale word from an abandoned prepare carries another
    // tag and never matches).
    // A finish-only call also zeroes the counters of its later kernels here (the arc kernels'
    // overflow count, the NMS error word), as slice_sort does in a one-call detection.
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *err_status = *err_pending == tag ? 1 : 0;
        *err_pending = 0;
        if (zero0) *zero0 = 0u;
        if (zero1) *zero1 = 0;
    }
    __shared__ int64_t s_last[kThreads / 64][kPrefixPix];
    __shared__ uint8_t s_has[kThreads / 64][kPrefixPix];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t HW = (int64_t)g.H * g.W;
    const int64_t q = (int64_t)blockIdx.x * kPrefixPix + lane;
    const bool in = q < HW;
    int64_t carry = in ? sae[q] : 0;  // B_0 = the caller's surface
    for (int64_t r0 = 0; r0 < n_groups; r0 += kPrefixRound) {
        const int64_t g0 = r0 + (int64_t)wave * kPrefixPer;
        uint32_t m[kPrefixPer];
        int64_t lt[kPrefixPer];
#pragma unroll
        for (int u = 0; u < kPrefixPer; ++u) m[u] = (in && g0 + u < n_groups) ? gmask[(g0 + u) * HW + q] : 0u;
#pragma unroll
        for (int u = 0; u < kPrefixPer; ++u) lt[u] = m[u] ? gB[(g0 + u) * HW + q] : 0;
        bool has = false;
        int64_t last = 0;
#pragma unroll
        for (int u = 0; u < kPrefixPer; ++u) {
            if (m[u]) { has = true; last = lt[u]; }
        }
        s_last[wave][lane] = last;
        s_has[wave][lane] = has ? 1 : 0;
        __syncthreads();
        int64_t run = carry;  // the value before this wave's first group
        for (int w = 0; w < wave; ++w)
            if (s_has[w][lane]) run = s_last[w][lane];
#pragma unroll
        for (int u = 0; u < kPrefixPer; ++u) {
            if (!in || g0 + u >= n_groups) break;
            gB[(g0 + u) * HW + q] = run;
            if (m[u]) run = lt[u];
        }
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w)
            if (s_has[w][lane]) carry = s_last[w][lane];
        __syncthreads();  // s_last reused by the next round
    }
    if (in && wave == 0) sae[q] = carry;
}

// The shard's own final time surface for the multi-GPU hand-off (ecc_fast_detect_prepare): per
// pixel the last timestamp of the batch, 0 where no event touched it — from the per-group images,
// no global atomics.
__global__ void __launch_bounds__(kThreads)
sae_local_last_kernel(CornerGeom g, int64_t n_groups, const uint32_t *__restrict__ gmask,
                      const int64_t *__restrict__ glast, int64_t *__restrict__ out) {
    const int64_t HW = (int64_t)g.H * g.W;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < HW; q += (int64_t)gridDim.x * kThreads) {
        int64_t run = 0;
        for (int64_t gi = n_groups - 1; gi >= 0; --gi)
            if (gmask[gi * HW + q]) { run = glast[gi * HW + q]; break; }
        out[q] = run;
    }
}

// Plain final-SAE scatter (no detection): sae[q] = max t.
__global__ void __launch_bounds__(kThreads)
sae_scatter_kernel(const uint32_t *__restrict__ xy, const int64_t *__restrict__ t, int64_t n,
                   int W, int H, int64_t *__restrict__ sae) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * kThreads) {
        const uint32_t v = xy[e];
        const int x = ecc::xy_x(v), y = ecc::xy_y(v);
        if (x < W && y < H)
            atomicMax(reinterpret_cast<long long *>(&sae[(int64_t)y * W + x]), (long long)t[e]);
    }
}

__global__ void __launch_bounds__(kThreads)
sae_max_combine_kernel(const int64_t *__restrict__ images, int n_images, int64_t hw,
                       int64_t *__restrict__ out) {
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < hw;
         q += (int64_t)gridDim.x * kThreads) {
        int64_t m = images[q];
        for (int i = 1; i < n_images; ++i) m = max(m, images[(int64_t)i * hw + q]);
        out[q] = m;
    }
}

}  // namespace

void ecc::corner::launch_pair_build(ecc_ctx *ctx, hipStream_t s, const int64_t *t, const CornerGeom &g, int64_t n_items,
                                    const Sorted &so, const GroupImages &gi) {
    ECC_TIMED(ctx, s, "pair_build_kernel");
    hipLaunchKernelGGL(pair_build_kernel, dim3((unsigned)n_items), dim3(kThreads), 0, s, t, g, so, gi.ovf, gi.pv,
                       gi.mask, gi.B, (const GroupRec *)gi.grec);
}

void ecc::corner::launch_sae_local_last(ecc_ctx *ctx, hipStream_t s, const CornerGeom &g, int64_t n_groups,
                                        const GroupImages &gi, int64_t *local_last) {
    ECC_TIMED(ctx, s, "sae_local_last_kernel");
    const int64_t HW = (int64_t)g.W * g.H;
    const unsigned blocks = (unsigned)std::min<int64_t>((HW + kThreads - 1) / kThreads, 8192);
    hipLaunchKernelGGL(sae_local_last_kernel, dim3(blocks), dim3(kThreads), 0, s, g, n_groups,
                       (const uint32_t *)gi.mask, (const int64_t *)gi.B, local_last);
}

void ecc::corner::launch_sae_prefix(ecc_ctx *ctx, hipStream_t s, const CornerGeom &g, int64_t n_groups,
                                    const GroupImages &gi, int64_t *sae, int32_t tag, uint32_t *zero0, int32_t *zero1) {
    ECC_TIMED(ctx, s, "sae_prefix_kernel");
    const int64_t HW = (int64_t)g.W * g.H;
    const unsigned blocks = (unsigned)((HW + kPrefixPix - 1) / kPrefixPix);
    hipLaunchKernelGGL(sae_prefix_kernel, dim3(blocks), dim3(kThreads), 0, s, g, n_groups,
                       (const uint32_t *)gi.mask, gi.B, sae, &ctx->dev->fast_verdict, &ctx->dev->sort_pending, tag,
                       zero0, zero1);
}

ECC_API int ecc_sae_scatter(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                            int32_t width, int32_t height, int64_t *sae, ecc_stream_t stream) {
    if (!ctx || !sae || n < 0 || width < 1 || height < 1) return ECC_ERR_INVALID;
    if (n == 0) return ECC_OK;
    if (!xy || !t) return ECC_ERR_INVALID;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t blocks = std::min<int64_t>((n + kThreads - 1) / kThreads, 4096);
    {
        ECC_TIMED(ctx, ecc::as_stream(stream), "sae_scatter_kernel");
        hipLaunchKernelGGL(sae_scatter_kernel, dim3((unsigned)blocks), dim3(kThreads), 0,
                           ecc::as_stream(stream), xy, t, n, width, height, sae);
    }
    ECC_CHECK_LAUNCH(ctx, "sae_scatter");
    return ECC_OK;
}

ECC_API int ecc_sae_max_combine(ecc_ctx *ctx, const int64_t *images, int32_t n_images, int64_t hw,
                                int64_t *out, ecc_stream_t stream) {
    if (!ctx || !out || hw < 0 || n_images < 0 || (n_images > 0 && !images)) return ECC_ERR_INVALID;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    if (n_images == 0) {
        ECC_CHECK_HIP(ctx, hipMemsetAsync(out, 0, hw * 8, s), "memset(sae)");
        return ECC_OK;
    }
    if (hw == 0) return ECC_OK;
    const int64_t blocks = std::min<int64_t>((hw + kThreads - 1) / kThreads, 4096);
    {
        ECC_TIMED(ctx, s, "sae_max_combine_kernel");
        hipLaunchKernelGGL(sae_max_combine_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, images,
                           n_images, hw, out);
    }
    ECC_CHECK_LAUNCH(ctx, "sae_max_combine");
    return ECC_OK;
}
