// The corner tracker's switch points, in plain C++ so that the host can read them
// (tests/tracker_paths_probe.cpp): which kernel takes a slice, and inside each kernel the sizes at
// which the matching scan, the per-track lists, the one-wave tail and the grouping change their
// path.  tracker.hip uses exactly these; the tests' case generators read them through the probe, so
// a changed constant moves the cases with it.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECC_TRK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ECC_TRK_HD inline
#endif

namespace trk_paths {

// ---- tracker_fast_kernel ---------------------------------------------------------------------
constexpr int kFT = 256;        // the largest T + C of a slice handled there (LDS arrays)
constexpr int kFThreads = 512;  // 8 waves: the round-0 scan runs 2-4 lanes per track
constexpr int kFList = 8;       // in-range detections a track keeps in registers (more: it rescans)
constexpr int kFTailTracks = 64;  // unresolved tracks the one-wave tail finishes
constexpr int kFLaneShiftT = 128;  // up to this many tracks 4 lanes scan for one, above it 2
constexpr int kFChunkNarrow = 16, kFChunkWide = 32;  // detections per scan chunk

// log2 of the lanes per track of the round-0 scan: L = 1 << shift, T * L <= kFThreads
ECC_TRK_HD int fast_lane_shift(int T) { return T <= kFLaneShiftT ? 2 : 1; }
// narrow chunks while every lane of a track has at most one of them
ECC_TRK_HD bool fast_chunk_narrow(int C, int L) { return C <= kFChunkNarrow * L; }

// ---- tracker_kernel --------------------------------------------------------------------------
constexpr int kNT = 512;       // one workgroup of 8 waves (2 per SIMD)
constexpr int kBuckets = 512;  // detection grid: hash buckets
constexpr int kBucketBits = 9;
constexpr int kBrute = 384;    // up to this many detections a scan walks all of them (uniform, no grid)
constexpr int kLaneList = 4;   // in-range detections a matching lane keeps in registers
constexpr int kTailCap = 1024;  // candidate entries of the one-wave matching tail
constexpr int kTailTracks = 64;  // unresolved tracks the one-wave tail finishes
constexpr int kLanesMax = 64;  // lanes per track of the brute scan
static_assert(kBuckets == 1 << kBucketBits, "bucket hash takes the top kBucketBits bits");

// grid matching for sane radii; otherwise every scan walks all detections
ECC_TRK_HD bool grid_ok(float max_distance) { return max_distance >= 0.0f && max_distance < 1.0e5f; }
// |dx| or |dy| above max_distance + 1 cannot give dist < max_distance (for sane radii)
ECC_TRK_HD float grid_reach(float max_distance) { return max_distance + 1.0f; }
// cell size: the integer box [p - reach, p + reach] of a prediction spans at most 3 cells an axis
ECC_TRK_HD int grid_cell(float max_distance) {
    return grid_ok(max_distance) ? (int)ceilf(grid_reach(max_distance)) + 1 : 1;
}
ECC_TRK_HD int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
// The cells on one axis that the grid visitor walks for a prediction coordinate p: those of the
// integer box [floor(p - reach), ceil(p + reach)] (|p| < 1e9, so the conversions are defined).
ECC_TRK_HD int grid_cell_lo(float p, float reach, int cell) { return floor_div((int)floorf(p - reach), cell); }
ECC_TRK_HD int grid_cell_hi(float p, float reach, int cell) { return floor_div((int)ceilf(p + reach), cell); }
ECC_TRK_HD int cell_bucket(int cx, int cy) {
    return (int)(((uint32_t)cx * 0x9E3779B1u ^ (uint32_t)cy * 0x85EBCA77u) >> (32 - kBucketBits));
}
// L lanes per track of the brute scan (a power of two, T * L * 2 <= kNT); the grid scan has one.
// The rule is a statement macro over an `int L = 1`: tracker_kernel expands it in place (through
// an inlined call the compiler lays the whole kernel out differently), general_lanes() wraps the
// same text for the host.
#define ECC_TRK_GENERAL_LANES(L, T, use_grid)                                                 \
    do {                                                                                      \
        if (!(use_grid))                                                                      \
            while ((L) < trk_paths::kLanesMax && (T) * (L) * 2 <= trk_paths::kNT) (L) <<= 1;   \
    } while (0)
ECC_TRK_HD int general_lanes(int T, bool use_grid) {
    int L = 1;
    ECC_TRK_GENERAL_LANES(L, T, use_grid);
    return L;
}
// a lane owns one track (its round-0 in-range detections stay in its registers)
ECC_TRK_HD bool lists_ok(int T, int L) { return T <= kNT / L; }

// ---- grouping (both kernels) -----------------------------------------------------------------
constexpr int kGroupWave = 64;  // up to this many candidates: one per lane, ballots, squared threshold

}  // namespace trk_paths
