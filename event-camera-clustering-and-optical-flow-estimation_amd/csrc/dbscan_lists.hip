// The product of DBSCANSimpleCluster::extract (PCC/DBSCAN_simple.h:27-90) as the reference returns
// it, std::vector<pcl::PointIndices> (used at PCC/pcl_cluster.cpp:131-142), built on the device from
// what ecc_dbscan_grid / _extract / _cloud_* leave there: labels, n_clusters and the unordered
// (point, cluster) pairs of the further memberships.  Per segment: the clusters in output order,
// each cluster's indices ascending (:82), a border point in every cluster that reached it.
//
// A membership is a key (cluster, j).  Sorted keys are the `members` row, and a cluster's interval is
// where its keys begin and end.
//
// Window path (seg_stride <= 8192), a workgroup per segment:
//   * a pre-pass bins the valid dup pairs by segment (count, scan, scatter into the workspace);
//     a pair that fails a range check is dropped there and never seen again;
//   * a segment of at most kLdsMembers memberships and at most kLdsClusters clusters packs its
//     keys into 32 bits (cluster << 13 | j), sorts them in LDS (bitonic, padded to a power of two
//     with the all-ones key) and finds every cluster's interval by two binary searches: the bytes
//     cannot depend on the order of the dups, and an empty cluster gets {begin, begin - 1} for free;
//     the launch is made twice, for the segments of at most kLdsMembers / 2 memberships with half
//     the LDS (twice the workgroups per CU: most downsample windows) and for the rest;
//   * any other segment goes through its own output rows: cluster sizes are counted and scanned in
//     its `pairs` row, and each membership's place is its cluster's begin plus the number of
//     memberships of that cluster that precede it in (j, label before dup, dup position) order,
//     counted from the inputs.  That count is quadratic in the memberships; it is the route of
//     fabricated input only (more than kLdsMembers - 8192 dups in one window).
// Cloud path (one segment of any size): 64-bit keys cluster << 32 | point for every slot and every
// dup (the all-ones key for what is not a membership), ecc::sort_pairs_u64_i32, and a cut of the
// sorted run.
#include "ecc_internal.hpp"
#include "sort_internal.hpp"

#include <algorithm>

namespace {

constexpr int kNT = 256;
constexpr int kMaxStride = 8192;             // window path: j fits 13 bits
constexpr int kJBits = 13;
constexpr int kLdsMembers = 16384;           // memberships of one segment sorted in LDS (64 KiB of keys)
constexpr int kLdsClusters = 1 << 18;        // cluster ids a packed key holds beside j, below the pad key
constexpr uint32_t kPadKey = 0xffffffffu;
constexpr uint64_t kNoKey = ~uint64_t(0);
constexpr int64_t kMaxBlocks = int64_t(1) << 30;
constexpr unsigned kDupBlocks = 2048;

struct DupView {
    const int64_t *dups;
    int64_t dup_cap;
    const int64_t *n_dups;
    __device__ __forceinline__ int64_t count() const {
        const int64_t n = *n_dups;
        return n < 0 ? 0 : (n < dup_cap ? n : dup_cap);
    }
};

// The segment and slot of dup pair k if it passes every range check, else s = -1.
struct DupRef {
    int64_t s;
    int32_t j, c;
};
__device__ __forceinline__ DupRef dup_ref(const DupView &d, int64_t k, const int32_t *n_clusters, int64_t n_segs,
                                          int64_t stride, const int32_t *seg_counts) {
    const int64_t p = d.dups[2 * k], c = d.dups[2 * k + 1];
    DupRef r{-1, 0, 0};
    if (p < 0 || p >= n_segs * stride) return r;
    const int64_t s = p / stride, j = p - s * stride;
    if (j >= ecc::seg_points(seg_counts, stride, s)) return r;
    if (c < 0 || c >= (int64_t)n_clusters[s]) return r;
    r.s = s, r.j = (int32_t)j, r.c = (int32_t)c;
    return r;
}

// ---- pre-pass: dups by segment
__global__ __launch_bounds__(kNT) void dup_count_kernel(DupView d, const int32_t *__restrict__ n_clusters,
                                                        int64_t n_segs, int64_t stride,
                                                        const int32_t *__restrict__ seg_counts, int32_t *seg_ndup,
                                                        int32_t *flag) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && *d.n_dups > d.dup_cap) flag[0] = 1;
    const int64_t nd = d.count();
    for (int64_t k = (int64_t)blockIdx.x * kNT + threadIdx.x; k < nd; k += (int64_t)gridDim.x * kNT) {
        const DupRef r = dup_ref(d, k, n_clusters, n_segs, stride, seg_counts);
        if (r.s < 0) flag[1] = 1;
        else atomicAdd(&seg_ndup[r.s], 1);
    }
}

__global__ __launch_bounds__(kNT) void dup_scatter_kernel(DupView d, const int32_t *__restrict__ n_clusters,
                                                          int64_t n_segs, int64_t stride,
                                                          const int32_t *__restrict__ seg_counts,
                                                          const int64_t *__restrict__ seg_off, int32_t *cursor,
                                                          int2 *binned) {
    const int64_t nd = d.count();
    for (int64_t k = (int64_t)blockIdx.x * kNT + threadIdx.x; k < nd; k += (int64_t)gridDim.x * kNT) {
        const DupRef r = dup_ref(d, k, n_clusters, n_segs, stride, seg_counts);
        if (r.s >= 0) binned[seg_off[r.s] + atomicAdd(&cursor[r.s], 1)] = make_int2(r.c, r.j);
    }
}

// ---- one segment
__device__ __forceinline__ int lower_bound_key(const uint32_t *keys, int n, uint32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Packed keys sorted in LDS.  M <= lds_keys, C <= kLdsClusters.
__device__ __forceinline__ void lists_in_lds(uint32_t *s_key, int *s_fill, const int32_t *__restrict__ lab, int n,
                                             int C, const int2 *__restrict__ dup, int nd, int M, int32_t *members_row,
                                             int32_t *pairs_row) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    int P2 = 2;
    while (P2 < M) P2 <<= 1;
    // labelled points, compacted a wave at a time (the sort makes their order irrelevant)
    for (int base = 0; base < n; base += kNT) {
        const int i = base + tid;
        const int l = i < n ? lab[i] : -1;
        const bool in = l >= 0 && l < C;
        const uint64_t mask = __ballot(in);
        int at = 0;
        if (lane == 0 && mask) at = atomicAdd(s_fill, __popcll(mask));
        at = __builtin_amdgcn_readfirstlane(at);
        if (in) s_key[at + __popcll(mask & ((uint64_t(1) << lane) - 1))] = ((uint32_t)l << kJBits) | (uint32_t)i;
    }
    const int n_lab = M - nd;
    for (int k = tid; k < nd; k += kNT) s_key[n_lab + k] = ((uint32_t)dup[k].x << kJBits) | (uint32_t)dup[k].y;
    for (int i = M + tid; i < P2; i += kNT) s_key[i] = kPadKey;
    __syncthreads();

    if (M > 1)
        for (int k = 2; k <= P2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P2 >> 1); t += kNT) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
                    const uint32_t a = s_key[i], b = s_key[q];
                    if ((a > b) == ((i & k) == 0)) s_key[i] = b, s_key[q] = a;
                }
                __syncthreads();
            }

    for (int i = tid; i < M; i += kNT) members_row[i] = (int32_t)(s_key[i] & (uint32_t)(kMaxStride - 1));
    for (int c = tid; c < C; c += kNT) {
        pairs_row[(int64_t)c * 2] = lower_bound_key(s_key, M, (uint32_t)c << kJBits);
        pairs_row[(int64_t)c * 2 + 1] = lower_bound_key(s_key, M, (uint32_t)(c + 1) << kJBits) - 1;
    }
}

// Through the segment's own rows: sizes and begins in `pairs`, each place counted from the inputs.
__device__ __forceinline__ void lists_in_rows(int *s_wave, const int32_t *__restrict__ lab, int n, int C,
                                              const int2 *__restrict__ dup, int64_t nd, int32_t *members_row,
                                              int32_t *pairs_row) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c < C; c += kNT) pairs_row[(int64_t)c * 2 + 1] = 0;
    __threadfence();
    __syncthreads();
    for (int i = tid; i < n; i += kNT) {
        const int l = lab[i];
        if (l >= 0 && l < C) atomicAdd(&pairs_row[(int64_t)l * 2 + 1], 1);
    }
    for (int64_t k = tid; k < nd; k += kNT) atomicAdd(&pairs_row[(int64_t)dup[k].x * 2 + 1], 1);
    __threadfence();
    __syncthreads();
    int carry = 0;
    for (int base = 0; base < C; base += kNT) {
        const int c = base + tid;
        const int cnt = c < C ? pairs_row[(int64_t)c * 2 + 1] : 0;
        const int incl = ecc::wave_incl_scan(cnt);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = carry, total = carry;
        for (int w = 0; w < kNT / 64; ++w) {
            const int v = s_wave[w];
            if (w < wave) before += v;
            total += v;
        }
        if (c < C) {
            const int begin = before + incl - cnt;
            pairs_row[(int64_t)c * 2] = begin;
            pairs_row[(int64_t)c * 2 + 1] = begin + cnt - 1;
        }
        carry = total;
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    // order inside a cluster: (j, the label before the dups, position among the binned dups)
    for (int i = tid; i < n; i += kNT) {
        const int l = lab[i];
        if (l < 0 || l >= C) continue;
        int r = 0;
        for (int q = 0; q < i; ++q) r += lab[q] == l;
        for (int64_t k = 0; k < nd; ++k) r += dup[k].x == l && dup[k].y < i;
        members_row[pairs_row[(int64_t)l * 2] + r] = i;
    }
    for (int64_t k = tid; k < nd; k += kNT) {
        const int2 m = dup[k];
        int r = 0;
        for (int q = 0; q <= m.y; ++q) r += lab[q] == m.x;
        for (int64_t o = 0; o < nd; ++o) r += dup[o].x == m.x && (dup[o].y < m.y || (dup[o].y == m.y && o < k));
        members_row[pairs_row[(int64_t)m.x * 2] + r] = m.y;
    }
}

__global__ __launch_bounds__(kNT) void dbscan_lists_kernel(const int32_t *__restrict__ labels,
                                                           const int32_t *__restrict__ n_clusters,
                                                           const int2 *__restrict__ binned,
                                                           const int64_t *__restrict__ seg_off, int64_t s0,
                                                           int64_t stride, const int32_t *__restrict__ seg_counts,
                                                           int32_t *members, int64_t member_stride,
                                                           int64_t *n_members, int32_t *pairs, int64_t pair_cap,
                                                           int lds_keys, int64_t m_above, int64_t m_upto,
                                                           int32_t *flag) {
    extern __shared__ uint32_t s_key[];
    __shared__ int s_wave[kNT / 64], s_fill;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = s0 + blockIdx.x;
    const int n = ecc::seg_points(seg_counts, stride, s);
    const int raw_c = n_clusters[s], C = raw_c < 0 ? 0 : raw_c;
    const int32_t *lab = labels + s * stride;
    const int64_t nd = seg_off[s + 1] - seg_off[s];
    const int2 *dup = binned + seg_off[s];

    int mine = 0;
    bool bad = raw_c < 0;
    for (int i = tid; i < n; i += kNT) {
        const int l = lab[i];
        mine += l >= 0 && l < C;
        bad |= l < -1 || l >= C;
    }
    if (bad) flag[1] = 1;
    mine = ecc::wave_incl_scan(mine);
    if (lane == 63) s_wave[wave] = mine;
    if (tid == 0) s_fill = 0;
    __syncthreads();
    int n_lab = 0;
    for (int w = 0; w < kNT / 64; ++w) n_lab += s_wave[w];
    __syncthreads();  // s_wave is used again
    const int64_t M = n_lab + nd;
    if (tid == 0) n_members[s] = M;
    if (M > member_stride || C > pair_cap) {  // all or nothing
        if (tid == 0) flag[0] = 1;
        return;
    }
    if (M <= m_above || M > m_upto) return;  // the other launch's segment
    int32_t *members_row = members + s * member_stride, *pairs_row = pairs + s * pair_cap * 2;
    if (M <= lds_keys && C <= kLdsClusters)
        lists_in_lds(s_key, &s_fill, lab, n, C, dup, (int)nd, (int)M, members_row, pairs_row);
    else
        lists_in_rows(s_wave, lab, n, C, dup, nd, members_row, pairs_row);
}

// ---- cloud path
__global__ __launch_bounds__(kNT) void cloud_keys_kernel(const int32_t *__restrict__ labels,
                                                         const int32_t *__restrict__ n_clusters, DupView d,
                                                         int64_t stride, const int32_t *__restrict__ seg_counts,
                                                         uint64_t *keys, int64_t n_keys, unsigned long long *n_valid,
                                                         int32_t *flag) {
    const int n = ecc::seg_points(seg_counts, stride, 0);
    const int raw_c = n_clusters[0], C = raw_c < 0 ? 0 : raw_c;
    const int64_t nd = d.count();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (*d.n_dups > d.dup_cap) flag[0] = 1;
        if (raw_c < 0) flag[1] = 1;
    }
    unsigned long long mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * kNT) {
        uint64_t key = kNoKey;
        if (i < stride) {
            if (i < n) {
                const int l = labels[i];
                if (l >= 0 && l < C) key = ((uint64_t)l << 32) | (uint64_t)i;
                else if (l != -1) flag[1] = 1;
            }
        } else if (i - stride < nd) {
            const int64_t p = d.dups[2 * (i - stride)], c = d.dups[2 * (i - stride) + 1];
            if (p >= 0 && p < n && c >= 0 && c < C) key = ((uint64_t)c << 32) | (uint64_t)p;
            else flag[1] = 1;
        }
        keys[i] = key;
        mine += key != kNoKey;
    }
    if (mine) atomicAdd(n_valid, mine);
}

__global__ __launch_bounds__(kNT) void cloud_cut_kernel(const uint64_t *__restrict__ keys,
                                                        const unsigned long long *__restrict__ n_valid,
                                                        const int32_t *__restrict__ n_clusters, int32_t *members,
                                                        int64_t member_stride, int64_t *n_members, int32_t *pairs,
                                                        int64_t pair_cap, int32_t *flag) {
    const int64_t M = (int64_t)*n_valid;
    const int raw_c = n_clusters[0], C = raw_c < 0 ? 0 : raw_c;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first) n_members[0] = M;
    if (M > member_stride || C > pair_cap) {
        if (first) flag[0] = 1;
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i <= M; i += (int64_t)gridDim.x * kNT) {
        const int prev = i > 0 ? (int)(keys[i - 1] >> 32) : -1;
        const int cur = i < M ? (int)(keys[i] >> 32) : C;
        if (i < M) members[i] = (int32_t)(uint32_t)keys[i];
        if (cur == prev) continue;
        for (int64_t c = (int64_t)prev + 1; c < cur; ++c) {  // empty clusters between the two
            pairs[c * 2] = (int32_t)i;
            pairs[c * 2 + 1] = (int32_t)(i - 1);
        }
        if (i < M) pairs[(int64_t)cur * 2] = (int32_t)i;
        if (i > 0) pairs[(int64_t)prev * 2 + 1] = (int32_t)(i - 1);
    }
}

int pow2_at_least(int64_t v) {
    int p = 64;
    while (p < v) p <<= 1;
    return p;
}

int windows(ecc_ctx *ctx, const int32_t *labels, const int32_t *n_clusters, DupView d, int64_t n_segs,
            int64_t stride, const int32_t *seg_counts, int32_t *members, int64_t member_stride, int64_t *n_members,
            int32_t *pairs, int64_t pair_cap, hipStream_t s, int32_t *flag) {
    // workspace: dups per segment, scatter cursors, offsets, scan scratch, the binned pairs
    const size_t cnt_bytes = ecc::align_up((size_t)n_segs * 4, 16), off_bytes = ecc::align_up((size_t)(n_segs + 1) * 8, 16);
    const size_t scan_bytes = ecc::align_up(ecc::scan_scratch_bytes(n_segs), 16);
    const size_t bin_bytes = ecc::align_up((size_t)std::max<int64_t>(d.dup_cap, 1) * 8, 16);
    if (int rc = ecc::ws_reserve(ctx, 2 * cnt_bytes + off_bytes + scan_bytes + bin_bytes); rc != ECC_OK) return rc;
    char *w = static_cast<char *>(ctx->ws);
    int32_t *seg_ndup = reinterpret_cast<int32_t *>(w);
    int32_t *cursor = reinterpret_cast<int32_t *>(w + cnt_bytes);
    int64_t *seg_off = reinterpret_cast<int64_t *>(w + 2 * cnt_bytes);
    int64_t *scan = reinterpret_cast<int64_t *>(w + 2 * cnt_bytes + off_bytes);
    int2 *binned = reinterpret_cast<int2 *>(w + 2 * cnt_bytes + off_bytes + scan_bytes);

    // two launches: segments of at most `small` memberships with that many keys of LDS, the rest with `large`
    const int small = pow2_at_least(std::min<int64_t>(stride, kLdsMembers / 2));
    const int large = pow2_at_least(std::min<int64_t>(stride + std::min<int64_t>(d.dup_cap, kLdsMembers), kLdsMembers));
    if (int rc = ecc::allow_dynamic_lds(ctx, dbscan_lists_kernel, large * 4, "dbscan_lists LDS"); rc != ECC_OK) return rc;

    ECC_CHECK_HIP(ctx, hipMemsetAsync(seg_ndup, 0, 2 * cnt_bytes, s), "memset(dbscan lists counts)");
    const unsigned dup_blocks =
        (unsigned)std::min<int64_t>(std::max<int64_t>((d.dup_cap + kNT - 1) / kNT, 1), kDupBlocks);
    {
        ECC_TIMED(ctx, s, "dbscan_lists_dup_count_kernel");
        hipLaunchKernelGGL(dup_count_kernel, dim3(dup_blocks), dim3(kNT), 0, s, d, n_clusters, n_segs, stride,
                           seg_counts, seg_ndup, flag);
    }
    if (int rc = ecc::exclusive_scan_i32_i64(ctx, seg_ndup, n_segs, seg_off, scan, s); rc != ECC_OK) return rc;
    if (d.dup_cap > 0) {
        ECC_TIMED(ctx, s, "dbscan_lists_dup_scatter_kernel");
        hipLaunchKernelGGL(dup_scatter_kernel, dim3(dup_blocks), dim3(kNT), 0, s, d, n_clusters, n_segs, stride,
                           seg_counts, seg_off, cursor, binned);
    }
    ECC_TIMED(ctx, s, "dbscan_lists_kernel");
    for (int pass = 0; pass < (large > small ? 2 : 1); ++pass) {
        const int lds_keys = pass == 0 ? small : large;
        const int64_t m_above = pass == 0 ? -1 : small, m_upto = pass == 0 && large > small ? small : INT64_MAX;
        for (int64_t s0 = 0; s0 < n_segs; s0 += kMaxBlocks) {
            hipLaunchKernelGGL(dbscan_lists_kernel, dim3((unsigned)std::min(n_segs - s0, kMaxBlocks)), dim3(kNT),
                               (size_t)lds_keys * 4, s, labels, n_clusters, binned, seg_off, s0, stride, seg_counts,
                               members, member_stride, n_members, pairs, pair_cap, lds_keys, m_above, m_upto, flag);
            ECC_CHECK_LAUNCH(ctx, "dbscan_lists");
        }
    }
    return ECC_OK;
}

int cloud(ecc_ctx *ctx, const int32_t *labels, const int32_t *n_clusters, DupView d, int64_t stride,
          const int32_t *seg_counts, int32_t *members, int64_t member_stride, int64_t *n_members, int32_t *pairs,
          int64_t pair_cap, hipStream_t s, int32_t *flag) {
    const int64_t n_keys = stride + d.dup_cap;
    const size_t key_bytes = ecc::align_up((size_t)n_keys * 8, 16), val_bytes = ecc::align_up((size_t)n_keys * 4, 16);
    const size_t tmp_bytes = ecc::align_up(ecc::sort_pairs_u64_i32_temp_bytes(n_keys, 64), 16);
    if (int rc = ecc::ws_reserve(ctx, 16 + 2 * key_bytes + 2 * val_bytes + tmp_bytes); rc != ECC_OK) return rc;
    char *w = static_cast<char *>(ctx->ws);
    unsigned long long *n_valid = reinterpret_cast<unsigned long long *>(w);
    uint64_t *keys_in = reinterpret_cast<uint64_t *>(w + 16), *keys_out = reinterpret_cast<uint64_t *>(w + 16 + key_bytes);
    int32_t *vals_in = reinterpret_cast<int32_t *>(w + 16 + 2 * key_bytes);
    int32_t *vals_out = reinterpret_cast<int32_t *>(w + 16 + 2 * key_bytes + val_bytes);
    void *tmp = w + 16 + 2 * key_bytes + 2 * val_bytes;

    ECC_CHECK_HIP(ctx, hipMemsetAsync(n_valid, 0, 16, s), "memset(dbscan lists count)");
    ECC_CHECK_HIP(ctx, hipMemsetAsync(vals_in, 0, val_bytes, s), "memset(dbscan lists values)");
    const unsigned blocks = (unsigned)std::min<int64_t>((n_keys + kNT - 1) / kNT, 8192);
    {
        ECC_TIMED(ctx, s, "dbscan_lists_cloud_keys_kernel");
        hipLaunchKernelGGL(cloud_keys_kernel, dim3(blocks), dim3(kNT), 0, s, labels, n_clusters, d, stride, seg_counts,
                           keys_in, n_keys, n_valid, flag);
    }
    if (int rc = ecc::sort_pairs_u64_i32(ctx, tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, n_keys, 64, s);
        rc != ECC_OK)
        return rc;
    ECC_TIMED(ctx, s, "dbscan_lists_cloud_cut_kernel");
    hipLaunchKernelGGL(cloud_cut_kernel, dim3(blocks), dim3(kNT), 0, s, keys_out, n_valid, n_clusters, members,
                       member_stride, n_members, pairs, pair_cap, flag);
    ECC_CHECK_LAUNCH(ctx, "dbscan_lists(cloud)");
    return ECC_OK;
}

}  // namespace

ECC_API int ecc_dbscan_lists(ecc_ctx *ctx, const int32_t *labels, const int32_t *n_clusters, const int64_t *dups,
                             int64_t dup_cap, const int64_t *n_dups, int64_t n_segs, int64_t seg_stride,
                             const int32_t *seg_counts, int32_t *members, int64_t member_stride, int64_t *n_members,
                             int32_t *pairs, int64_t pair_cap, ecc_stream_t stream) {
    if (!ctx || n_segs < 0 || dup_cap < 0 || pair_cap < 0) return ECC_ERR_INVALID;
    if (seg_stride < 1 || seg_stride > INT32_MAX || member_stride < 0 || member_stride > INT32_MAX) return ECC_ERR_INVALID;
    if (seg_stride > kMaxStride && n_segs > 1) return ECC_ERR_INVALID;
    if (dup_cap > 0 && !dups) return ECC_ERR_INVALID;
    if (n_segs > 0 && (!labels || !n_clusters || !n_dups || !members || !n_members || !pairs)) return ECC_ERR_INVALID;
    if (n_segs == 0) return ECC_OK;
    ECC_CHECK_HIP(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = ecc::as_stream(stream);
    int32_t *flag = ctx->dev->dbscan_lists;
    ECC_CHECK_HIP(ctx, hipMemsetAsync(flag, 0, 8, s), "memset(dbscan lists err)");
    const DupView d{dups, dup_cap, n_dups};
    if (seg_stride <= kMaxStride)
        return windows(ctx, labels, n_clusters, d, n_segs, seg_stride, seg_counts, members, member_stride, n_members,
                       pairs, pair_cap, s, flag);
    return cloud(ctx, labels, n_clusters, d, seg_stride, seg_counts, members, member_stride, n_members, pairs,
                 pair_cap, s, flag);
}

ECC_API int ecc_dbscan_lists_status(ecc_ctx *ctx, ecc_stream_t stream) {
    if (!ctx) return ECC_ERR_INVALID;
    int32_t f[2] = {0, 0};
    if (int rc = ecc::read_dev_words(ctx, ctx->dev->dbscan_lists, 2, f, ecc::as_stream(stream))) return rc;
    return f[1] ? ECC_ERR_INVALID : (f[0] ? ECC_ERR_CAPACITY : ECC_OK);
}
