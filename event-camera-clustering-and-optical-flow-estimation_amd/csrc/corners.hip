// SAE (time surface) + FAST/arc corner detection: the host driver.
//
// Reference: FCT/metavision_time_surface_periodic_group_track.cpp — per reslicer slice of
// 16384 events the aggregate lambda first writes time_surface.at(y,x) = t for EVERY event
// (:900-923, batch semantics Q14), then runs the eFAST arc test event by event on the CPU
// (:948-1063; circle3 streaks of 3..6 of 16 then circle4 streaks of 4..8 of 20, circles
// :44-45 as {dy,dx}), holding a mutex per event.
//
// Exact batch semantics for a whole batch with no per-slice (or per-group) launches.  The arc
// test of an event in slice s must see V(q,s) = t of the last event at pixel q with index
// < end(s).  Slices are taken in GROUPS of G = 32; with B_g = the SAE before group g,
// V(q,s) = the last t at q in slices j' <= j of the group (j = s mod 32), else B_g[q]
// (timestamps are non-decreasing, so max == last writer; a device check enforces it).
//
// Pipeline (every launch covers the whole batch; one file per stage, corner_common.hpp for what
// they share):
//   slice_sort (corner_sort.hip): per slice, a counting sort by 14x14-pixel TILE into 4-byte
//               keys (group-relative timestamp, or event index within the group, << 8 | pixel
//               within the tile), with a per-slice (slice, pixel) dedup; the time-order check;
//               each group's constants (GroupRec) for the kernels below;
//   pair_build (corner_pairs.hip): per (group, tile) the distinct (slice, pixel) pairs with the
//               value an arc test reads there, as one record per pixel; the slices that touched
//               each pixel and its last timestamp;
//   sae_prefix (corner_pairs.hip): per pixel, B_g for every group (prefix over groups) and the
//               final SAE; publishes the sort's verdict;
//   arc (corner_arc.hip): one 512-lane workgroup per (group, tile) for ALL groups at once: it
//               stages its 22x22 window's values as compact per-pixel lists in LDS and tests each
//               distinct (slice, pixel) pair of its tile once on clamped 32-bit keys;
//   arc_dense (corner_arc.hip): the items arc left (heavy windows, wide groups, ties the clamp
//               may have merged) on dense per-slice planes, with the exact int64 tests;
//   flags (corner_flags.hip): per event in stream order, eligibility (Q11, Q15, border) && its
//               pair's result; for the fused NMS calls also each slice's candidate list.
//
// Arc test: the reference loop "exists i,s: T[c(i)]>=T[c(i-1)], T[c(i+s-1)]>=T[c(i+s)], and
// every T outside the streak < min(streak)" reduces to "the s largest values are strictly
// greater than the rest and occupy a contiguous arc" (the two >= conditions are implied).
// With cnt[j] = #{k : T[k] > T[j]}, the top-s set is {j : cnt[j] < s}; it is strictly
// separated iff its size is s.  This branch-free form is exact; tests/test_gpu_parity.py
// checks it against the literal loop in oracle/oracle.cpp.
// Algorithmic bytes: 12 B/event in (xy + t) + 1 B/event out (corner flag).
#include "corner_common.hpp"

namespace {

// Sequential carve of one allocation; with base == nullptr it only measures.
struct Carve {
    char *base;
    size_t used = 0;
    template <class T> T *take(size_t count) {
        T *r = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += ecc::align_up(count * sizeof(T), 256);
        return r;
    }
};

Sorted carve_sorted(Carve &cv, const CornerGeom &g, int64_t n_items, int64_t n_groups, int32_t **first_border,
                    GroupImages *gi) {
    Sorted so{};
    so.key = cv.take<uint32_t>((size_t)g.n);
    so.t32 = cv.take<uint32_t>((size_t)g.n);
    so.toff = cv.take<int32_t>((size_t)g.n_slices * (g.n_tiles + 2));
    *first_border = cv.take<int32_t>((size_t)g.n_slices);
    const size_t img = (size_t)n_groups * g.W * g.H;
    gi->mask = cv.take<uint32_t>(img);
    gi->B = cv.take<int64_t>(img);
    gi->res = cv.take<uint32_t>((size_t)n_groups * kGroup * g.seg_stride);
    gi->pv = cv.take<uint4>(img);
    gi->ovf = cv.take<uint32_t>((size_t)g.n + 4 * (size_t)n_items + 8);
    gi->over = cv.take<int64_t>((size_t)n_items);
    gi->n_over = cv.take<uint32_t>(64);
    gi->grec = cv.take<GroupRec>((size_t)n_groups);
    return so;
}

}  // namespace

ECC_API void ecc_corner_cfg_default(ecc_corner_cfg *cfg) {
    if (!cfg) return;
    cfg->width = 1280;            // hard-coded bounds of the reference arc test (:952-953)
    cfg->height = 720;
    cfg->slice_events = 16384;    // make_n_events(nevents = ARRAY_SIZE), :745, :772-774
    cfg->margin = 4;              // cs = max_scale * 4, :948-951
    cfg->border_mode = 0;         // fixed; 1 = ref_compat `break` (Q11)
    cfg->first_detect_slice = 1;  // time_surface_flag (Q15)
    cfg->any_order = 0;           // Metavision stream order (checked)
}

// phase bit 1: sort + pair entries (+ the shard-local last-t image when local_last != null);
// phase bit 2: SAE prefix from `sae` + arc tests + flags.  Both phases see the same workspace
// carve (same n and cfg), so prepare/finish may be separate calls with a collective between.
//
// The unsorted-time verdict: DevWords::sort_pending holds the tag of the last sort phase that saw
// decreasing time (every sort phase gets a fresh host-side tag, so a stale word never matches a
// later call); fast_verdict the verdict sae_prefix_kernel published for the last finished call
// (pending word == its prepare's tag).
static int fast_detect_phases(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                              const ecc_corner_cfg *cfg, int64_t *sae, uint8_t *corner_flags, int64_t *local_last,
                              int phases, ecc_stream_t stream, uint32_t *cand = nullptr, int32_t *n_cand = nullptr,
                              int32_t *zero_nms_err = nullptr) {
    if (!ctx || !cfg || n < 0) return ECC_ERR_INVALID;
    if ((phases & 2) && !sae) return ECC_ERR_INVALID;
    if (n > 0 && (!xy || !t || ((phases & 2) && !corner_flags))) return ECC_ERR_INVALID;
    if (cfg->width < 1 || cfg->height < 1 || cfg->width > 65536 || cfg->height > 65536)
        return ECC_ERR_INVALID;
    if (cfg->margin < 4 || 2 * cfg->margin >= cfg->width || 2 * cfg->margin >= cfg->height)
        return ECC_ERR_INVALID;  // the circles reach 4 px from the event
    if (cfg->slice_events < 1 || cfg->slice_events > kMaxSlice ||
        (cfg->border_mode != 0 && cfg->border_mode != 1))
        return ECC_ERR_INVALID;
    if (cfg->any_order != 0 && (cfg->any_order != 1 || phases != 3)) return ECC_ERR_INVALID;
    CornerGeom g{};
    g.W = cfg->width;
    g.H = cfg->height;
    g.S = cfg->slice_events;
    g.inv_S = 1.0f / (float)g.S;
    g.margin = cfg->margin;
    g.border_mode = cfg->border_mode;
    g.first_detect = cfg->first_detect_slice;
    g.any_order = cfg->any_order;
    g.tiles_x = (g.W + kTile - 1) / kTile;
    g.n_tiles = g.tiles_x * ((g.H + kTile - 1) / kTile);
    g.seg_stride = (g.n_tiles * kSegWords + 3) & ~3;
    {
        const MagicDiv nt = magic_div31((uint32_t)g.n_tiles), tx = magic_div31((uint32_t)g.tiles_x);
        g.nt_mul = nt.mul, g.nt_sh = nt.sh, g.tx_mul = tx.mul, g.tx_sh = tx.sh;
    }
    if (g.n_tiles > kMaxTiles) return ECC_ERR_INVALID;  // > 8191 16x16 tiles (~2.1 Mpixel)
    // slice_sort's dedup bitmap (one bit per tile pixel), kept only while two of its workgroups
    // still fit a CU's LDS (sensors up to ~400 tiles of 14x14 pixels, e.g. 346x260)
    g.dedup_words = (int)(((int64_t)g.n_tiles * kTilePix + 31) / 32);
    if (((size_t)g.n_tiles + 1 + kSortSent + kSortChunk + g.dedup_words) * 4 + 256 > 80 * 1024) g.dedup_words = 0;
    g.n = n;
    g.n_slices = (n + g.S - 1) / g.S;
    if (g.n_slices > INT32_MAX) return ECC_ERR_INVALID;
    hipStream_t s = ecc::as_stream(stream);
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    ecc::CornerState *st = &ctx->corner;
    if (phases & 1) {  // a fresh tag for this sort phase (never 0: the pending word starts at 0)
        st->next_tag = st->next_tag == INT32_MAX ? 1 : st->next_tag + 1;
        st->prep_tag = st->next_tag;
    }
    if (n == 0) {
        st->status_src = 0;  // an empty call reports OK, whatever earlier calls saw
        if (local_last) ECC_CHECK_HIP(ctx, hipMemsetAsync(local_last, 0, (size_t)g.W * g.H * 8, s), "memset(local)");
        return ECC_OK;
    }
    const int64_t n_groups = (g.n_slices + kGroup - 1) / kGroup;
    const int64_t n_items = n_groups * g.n_tiles;  // work items: (group, tile)
    if (n_items > (int64_t)INT32_MAX - 8) return ECC_ERR_INVALID;
    if ((n + 4 * n_items) / 4 >= (int64_t)UINT32_MAX) return ECC_ERR_INVALID;  // 16-B overflow index in a u32
    int32_t *first_border = nullptr;
    GroupImages gi{};
    Carve measure{nullptr};
    carve_sorted(measure, g, n_items, n_groups, &first_border, &gi);
    if (!(phases & 1) && measure.used > ctx->corner_buf.bytes) return ECC_ERR_INVALID;  // finish without prepare
    int rc = ECC_OK;
    if ((phases & 1) && measure.used > ctx->corner_buf.bytes) {  // grown, never shrunk
        st->n_over = nullptr;  // it points into the buffer
        rc = ecc::buf_reserve(ctx, ctx->corner_buf, ecc::align_up(measure.used + measure.used / 8, 1 << 20),
                              "corner batch");
        if (rc) return rc;
    }
    Carve cv{static_cast<char *>(ctx->corner_buf.p)};
    const Sorted so = carve_sorted(cv, g, n_items, n_groups, &first_border, &gi);

    if (phases & 1) {
        rc = launch_sort(ctx, s, xy, t, g, so, first_border, st->prep_tag, (phases & 2) ? gi.n_over : nullptr,
                         zero_nms_err, gi.grec);
        if (rc) return rc;
        launch_pair_build(ctx, s, t, g, n_items, so, gi);
        if (local_last) launch_sae_local_last(ctx, s, g, n_groups, gi, local_last);
    }
    if (!(phases & 2)) {
        st->status_src = 1;
        ECC_CHECK_LAUNCH(ctx, "fast_detect_prepare");
        return ECC_OK;
    }
    st->status_src = 2;
    st->n_over = gi.n_over;
    st->n_items = n_items;
    st->n_slices = g.n_slices;
    st->n_groups = n_groups;
    launch_sae_prefix(ctx, s, g, n_groups, gi, sae, st->prep_tag, (phases & 1) ? nullptr : gi.n_over,
                      (phases & 1) ? nullptr : zero_nms_err);
    launch_arc(ctx, s, g, n_items, gi);
    launch_arc_dense(ctx, s, t, g, gi);
    if ((rc = launch_flags(ctx, s, xy, g, gi, first_border, corner_flags, cand, n_cand))) return rc;
    ECC_CHECK_LAUNCH(ctx, "fast_detect");
    return ECC_OK;
}

ECC_API int ecc_fast_detect(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                            const ecc_corner_cfg *cfg, int64_t *sae, uint8_t *corner_flags,
                            ecc_stream_t stream) {
    return fast_detect_phases(ctx, xy, t, n, cfg, sae, corner_flags, nullptr, 3, stream);
}

// detection (phases 3: sort + tests; 2: the finish half) followed by the per-slice NMS
static int fast_detect_nms_phases(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                                  const ecc_corner_cfg *cfg, int64_t *sae, uint8_t *corner_flags, int32_t box_size,
                                  int32_t cap, ecc_corner *out, int32_t *out_count, int phases, ecc_stream_t stream) {
    if (!ctx || !cfg) return ECC_ERR_INVALID;
    if (ecc::nms_check_args(n, cfg->slice_events, cfg->width, cfg->height, box_size, cap)) return ECC_ERR_INVALID;
    if (n > 0 && (!out_count || (cap > 0 && !out))) return ECC_ERR_INVALID;
    const int64_t tiles = (int64_t)((cfg->width + kTile - 1) / kTile) * ((cfg->height + kTile - 1) / kTile);
    uint32_t *cand = nullptr;
    int32_t *n_cand = nullptr;
    // (flags off 4-B alignment: the candidate form would leave each slice to one lane; the flag pass's
    // all-lane scalar arm and nms_compact_kernel take such callers)
    if (n > 0 && cfg->slice_events % 4 == 0 && cfg->slice_events <= kFlagCandMax &&
        (reinterpret_cast<uintptr_t>(corner_flags) & 3) == 0 && tiles * kSegWords * 4 <= (int64_t)kFlagDynLdsMax) {
        int rc = ecc::nms_candidates(ctx, n, cfg->slice_events, cfg->width, cfg->height, box_size, &cand, &n_cand);
        if (rc) return rc;
    }
    if (!cand) {  // the two calls
        int rc = phases == 3 ? ecc_fast_detect(ctx, xy, t, n, cfg, sae, corner_flags, stream)
                             : ecc_fast_detect_finish(ctx, xy, t, n, cfg, sae, corner_flags, stream);
        if (rc) return rc;
        return ecc_corner_nms(ctx, xy, corner_flags, n, cfg->slice_events, cfg->width, cfg->height, box_size, cap, out,
                              out_count, stream);
    }
    hipStream_t s = ecc::as_stream(stream);
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    // the NMS error word is zeroed by the call's first kernel (n > 0 here: nms_candidates gave a
    // buffer): the sort kernel, or in a finish-only call the SAE prefix
    int rc = fast_detect_phases(ctx, xy, t, n, cfg, sae, corner_flags, nullptr, phases, stream, cand, n_cand,
                                &ctx->dev->nms);
    if (rc) return rc;
    rc = ecc::nms_greedy(ctx, cand, n_cand, n, cfg->slice_events, cfg->width, cfg->height, box_size, cap, out,
                         out_count, s);
    if (rc) return rc;
    ECC_CHECK_LAUNCH(ctx, "fast_detect_nms");
    return ECC_OK;
}

ECC_API int ecc_fast_detect_nms(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                                const ecc_corner_cfg *cfg, int64_t *sae, uint8_t *corner_flags, int32_t box_size,
                                int32_t cap, ecc_corner *out, int32_t *out_count, ecc_stream_t stream) {
    return fast_detect_nms_phases(ctx, xy, t, n, cfg, sae, corner_flags, box_size, cap, out, out_count, 3, stream);
}

ECC_API int ecc_fast_detect_finish_nms(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                                       const ecc_corner_cfg *cfg, int64_t *sae, uint8_t *corner_flags,
                                       int32_t box_size, int32_t cap, ecc_corner *out, int32_t *out_count,
                                       ecc_stream_t stream) {
    return fast_detect_nms_phases(ctx, xy, t, n, cfg, sae, corner_flags, box_size, cap, out, out_count, 2, stream);
}

ECC_API int ecc_fast_detect_prepare(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                                    const ecc_corner_cfg *cfg, int64_t *local_last, ecc_stream_t stream) {
    return fast_detect_phases(ctx, xy, t, n, cfg, nullptr, nullptr, local_last, 1, stream);
}

ECC_API int ecc_fast_detect_finish(ecc_ctx *ctx, const uint32_t *xy, const int64_t *t, int64_t n,
                                   const ecc_corner_cfg *cfg, int64_t *sae, uint8_t *corner_flags,
                                   ecc_stream_t stream) {
    return fast_detect_phases(ctx, xy, t, n, cfg, sae, corner_flags, nullptr, 2, stream);
}

ECC_API int ecc_fast_detect_status(ecc_ctx *ctx, ecc_stream_t stream) {
    if (!ctx) return ECC_ERR_INVALID;
    // the verdict of the last call on this context (CornerState::status_src)
    const ecc::CornerState *st = &ctx->corner;
    if (st->status_src == 0) return ECC_OK;
    int32_t w = 0;
    const int32_t *src = st->status_src == 1 ? &ctx->dev->sort_pending : &ctx->dev->fast_verdict;
    if (int rc = ecc::read_dev_words(ctx, src, 1, &w, ecc::as_stream(stream))) return rc;
    const bool bad = st->status_src == 1 ? w == st->prep_tag : w != 0;
    return bad ? ECC_ERR_UNSORTED_TIME : ECC_OK;
}

ECC_API int ecc_fast_detect_stats(ecc_ctx *ctx, int64_t *out, int32_t n_out, ecc_stream_t stream) {
    if (!ctx || n_out < 0 || (n_out > 0 && !out)) return ECC_ERR_INVALID;
    const ecc::CornerState *st = &ctx->corner;
    uint32_t ov = 0;
    if (st->n_over) {
        ECC_CHECK_HIP(ctx, hipMemcpyAsync(&ov, st->n_over, 4, hipMemcpyDeviceToHost, ecc::as_stream(stream)),
                      "read overflow count");
        ECC_CHECK_HIP(ctx, hipStreamSynchronize(ecc::as_stream(stream)), "sync");
    }
    const int64_t v[4] = {st->n_items, (int64_t)ov, st->n_slices, st->n_groups};
    for (int i = 0; i < n_out && i < 4; ++i) out[i] = v[i];
    return ECC_OK;
}
