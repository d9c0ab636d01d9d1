// Shared by host/optics_xi.cpp and host/optics_tree.cpp: the xi pairs of many device-resident plots,
// left on the device.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/ecc.hpp"

namespace ecc {
namespace optics {

// ecc_optics_xi over all segments (n_segs >= 1; arguments as get_chi_clusters_flat_windows) into
// d_pairs at the capacity it returns: a second pass with the largest count as capacity when the
// first guess was too small.  d_n (n_segs int32) and counts get the pairs per segment.  Throws
// Error; synchronises the context's stream.
int64_t xi_pairs_on_device(Context &ctx, const double *device_reach, int64_t n_segs, int64_t seg_stride,
                           const int32_t *device_seg_counts, double chi, std::size_t min_pts,
                           double steep_area_min_diff, DeviceBuffer &d_pairs, DeviceBuffer &d_n,
                           std::vector<int32_t> &counts);

}  // namespace optics
}  // namespace ecc
