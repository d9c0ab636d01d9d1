// Stand-in for <pcl/point_types.h> and the other PCL names PCC/DBSCAN_simple.h uses, so that the
// reference header is included whole and unmodified without PCL.  TEST INFRASTRUCTURE ONLY; our code,
// from PCL's documented types: pcl::PointXYZ has float x, y, z; pcl::PointCloud<T> has a public
// std::vector `points` and a `header`, and Ptr is a shared pointer; pcl::PointIndices has a
// `header` and std::vector<int> `indices`; pcl::search::KdTree<T>::Ptr is a shared pointer (the
// simple DBSCAN stores it and never searches through it: its radiusSearch is a brute-force loop).
// The standard headers below are those PCL's own headers bring in and DBSCAN_simple.h relies on.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <string>
#include <vector>

namespace pcl {
struct PCLHeader {
    std::uint32_t seq = 0;
    std::uint64_t stamp = 0;
    std::string frame_id;
};
struct PointXYZ {
    float x = 0, y = 0, z = 0;
};
template <typename PointT>
struct PointCloud {
    typedef std::shared_ptr<PointCloud<PointT>> Ptr;
    PCLHeader header;
    std::vector<PointT> points;
};
struct PointIndices {
    PCLHeader header;
    std::vector<int> indices;
};
namespace search {
template <typename PointT>
struct KdTree {
    typedef std::shared_ptr<KdTree<PointT>> Ptr;
};
}  // namespace search
}  // namespace pcl
