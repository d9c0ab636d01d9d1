// ecc.hpp — C++ host layer of the MI355X event pipeline, mirroring the reference's own
// operator interfaces (same names, argument meaning and error behaviour) on top of the C ABI in
// ecc.h, so a reference host program switches by changing its includes:
//
//   reference                                                    here
//   CornerFilter::filterCorners      FCT/…group_track.cpp:81-152   ecc::CornerFilter::filterCorners
//   CornerTracker(...)::updateTrackedCorners / getCornerGroups
//                                    FCT/…group_track.cpp:401-536  ecc::CornerTracker
//   struct Corner / TrackedCorner / CornerGroup / DirectionVector
//                                    FCT/…group_track.cpp:61-199   ecc::Corner ... (cv::Point2f ->
//                                                                  ecc::Point2f, cv::Point -> ecc::Point)
//   optics::compute_reachability_dists<N>(pts, min_pts, eps)
//                                    OPT/include/optics/optics.hpp:413-565  ecc::optics::compute_reachability_dists
//                                                                  (runtime N instead of the template N)
//   optics::get_chi_clusters_flat    optics.hpp:803-944             ecc::optics::get_chi_clusters_flat[_windows]
//   optics::get_chi_clusters / flat_clusters_to_tree, Node / Tree / tree_depth / tree_size / flatten_dfs
//                                    optics.hpp:948-995, 1018-1021, tree.hpp  ecc::optics::get_chi_clusters[_windows] ...
//   optics::get_cluster_points       optics.hpp:692-721, 760-774    ecc::optics::get_cluster_points
//   per-cluster size, centroid, variance  OPT/test/cluster_event_data.cpp:472-527
//                                                                  ecc::optics::cluster_statistics[_windows]
//   optics::get_cluster_indices / epsilon_estimation
//                                    optics.hpp:674-690, 369-387   ecc::optics::...
//   DBSCANSimpleCluster / DBSCANPrecompCluster::{setInputCloud, setClusterTolerance,
//     setCorePointMinPts, setMin/MaxClusterSize, extract}
//                                    PCC/DBSCAN_simple.h:14-143, DBSCAN_precomp.h  ecc::DBSCANSimpleCluster ...
//   the same extract per downsample window, and the statistics of its lists
//                                    PCC/DBSCAN_simple.h:27-90      ecc::dbscan_extract_windows,
//                                                                  ecc::dbscan_statistics_windows
//   process_coordinates + host slice path  SMP/…opencl_store.cpp:250-417  ecc::HashDownsampler
//   assign_to_centers + k-means host loop  KM/assign_to_centers2.c:184-548 ecc::KMeans
//   the same loop per slice + centroid - centroid_prev[id]
//                                    DSA/…opencl_store.cpp:389-445, TWE/…:396-448  ecc::KMeans::fit_windows,
//                                                                  ecc::window_centroid_flow
//   aggregate lambda (batch SAE + arc test) FCT/…group_track.cpp:884-1070  ecc::TimeSurfaceCornerDetector
//
// Errors: the C ABI returns negative ecc_status codes; this layer throws ecc::Error (the
// reference hosts perror()+exit(1); its host programs in apps/ do the same on an ecc::Error).
// Compute always runs on the GPU through libecc; there is no CPU fallback.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cmath>
#include <deque>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ecc.h"

#pragma GCC visibility push(default)
namespace ecc {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string &what)
        : std::runtime_error(what + ": " + ecc_status_string(status)), status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

// One GPU context + stream (replaces create_device/clCreateContext/clCreateCommandQueue).
class Context {
  public:
    explicit Context(int device = 0);
    ~Context();
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ecc_ctx *get() const { return ctx_; }
    ecc_stream_t stream() const { return stream_; }
    void sync() const;
    // process-wide default context on device 0 (the reference's single global OpenCL device)
    static Context &default_context();

  private:
    ecc_ctx *ctx_ = nullptr;
    ecc_stream_t stream_ = nullptr;
};

// Owning device buffer.
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t bytes);
    ~DeviceBuffer();
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    void *data() const { return p_; }
    size_t size() const { return n_; }
    void reserve(size_t bytes);  // grows (content not kept)
    template <typename T> T *as() const { return static_cast<T *>(p_); }
    void upload(const void *src, size_t bytes, ecc_stream_t s);
    void download(void *dst, size_t bytes, ecc_stream_t s) const;

  private:
    void *p_ = nullptr;
    size_t n_ = 0;
};

inline uint32_t pack_xy(int x, int y) { return (uint32_t)(x & 0xffff) | ((uint32_t)(y & 0xffff) << 16); }

// ------------------------------------------------------------------------------ corners
struct Corner {  // FCT/…group_track.cpp:61-67
    int x;
    int y;
    int label;
};

struct Point {  // cv::Point
    int x, y;
};

struct Point2f {  // cv::Point2f
    float x, y;
};

struct DirectionVector {  // :163-175
    Point2f current;
    Point2f target;
    float damping;
    float smoothing;
};

struct TrackedCorner {  // :177-190
    int x;
    int y;
    int label;
    int frame_count;
    bool is_matched;
    int frames_since_last_detection;
    std::deque<Point> position_history;
    Point2f velocity;
    DirectionVector direction;
    int group_id;
};

struct CornerGroup {  // :193-199
    std::vector<int> corner_labels;
    Point2f average_velocity;
    Point2f centroid;
    float radius;
};

class CornerFilter {  // :69-153
  public:
    static std::vector<Corner> filterCorners(const std::vector<Corner> &corners, int image_width,
                                             int image_height, int box_size, float threshold);
    static std::vector<Corner> filterCorners(Context &ctx, const std::vector<Corner> &corners,
                                             int image_width, int image_height, int box_size,
                                             float threshold);
};

class CornerTracker {  // :201-537, device-resident state
  public:
    CornerTracker(float max_matching_distance = 30.0f, int max_frames = 30, int history_size = 10,
                  int frames_to_skip = 5, float damping = 0.8f, float smoothing = 0.3f,
                  float group_rad = 50.0f);
    CornerTracker(Context &ctx, const ecc_tracker_cfg &cfg, int max_tracks = ECC_TRACKER_MAX_TRACKS,
                  int max_detections = 4096);
    ~CornerTracker();
    CornerTracker(const CornerTracker &) = delete;
    CornerTracker &operator=(const CornerTracker &) = delete;

    std::vector<TrackedCorner> updateTrackedCorners(const std::vector<Corner> &current_corners);
    const std::map<int, CornerGroup> &getCornerGroups() const { return groups_; }
    // Batched form: n_slices NMS outputs already on the device (one launch for all slices).
    void updateDevice(const ecc_corner *d_corners, const int32_t *d_counts, int n_slices, int cap);
    std::vector<TrackedCorner> tracks();  // current state (host copy)
    void refreshGroups();

  private:
    Context *ctx_;
    ecc_tracker *tr_ = nullptr;
    int max_tracks_, max_det_;
    DeviceBuffer d_corners_, d_count_;
    std::map<int, CornerGroup> groups_;
};

// Batch SAE + arc-test corner detector (the aggregate lambda, :884-1070), stream-continuable.
class TimeSurfaceCornerDetector {
  public:
    // any_order: timestamps need not be non-decreasing (ecc_corner_cfg.any_order; exact path)
    TimeSurfaceCornerDetector(Context &ctx, int width, int height, int slice_events = 16384,
                              int border_mode = 0, bool any_order = false);
    // xy/t on the device; flags (device, n bytes) receive 1 for corner events.  The SAE carries
    // over between calls; the first call skips the first slice (time_surface_flag, :926).
    void detect(const uint32_t *d_xy, const int64_t *d_t, int64_t n, uint8_t *d_flags);
    int64_t *sae() const { return sae_.as<int64_t>(); }
    const ecc_corner_cfg &config() const { return cfg_; }

  private:
    Context &ctx_;
    ecc_corner_cfg cfg_;
    DeviceBuffer sae_;
    bool first_ = true;
};

// ------------------------------------------------------------------------------ ingest
// RAW recording reader (the role of Metavision::Camera::from_file(argv[1]), FCT/…group_track.cpp
// :756-760): the host streams payload words from disk, the GPU decodes them (ecc_evt_decode)
// with the carry state between chunks, so a recording of any length decodes piecewise.
// EVT 2.0, EVT 2.1 (both half orders) and EVT 3.0.  An EVT 2.1 word holds up to 32 events, so for
// that format the event buffers grow to each chunk's true count (the mask bits of its CD words,
// counted on the host) and are never sized from the 32-per-word bound.
class RawFileReader {
  public:
    RawFileReader(Context &ctx, const std::string &path, int64_t chunk_words = int64_t(1) << 24);
    const ecc_raw_info &info() const { return info_; }
    // Decodes the next chunk; device arrays stay valid until the next call.  0 at end of file.
    int64_t next(const uint32_t **d_xy, const int64_t **d_t, const uint8_t **d_p);
    // Whole recording into host vectors.
    void read_all(std::vector<uint32_t> &xy, std::vector<int64_t> &t, std::vector<uint8_t> &p);

  private:
    Context &ctx_;
    std::string path_;
    ecc_raw_info info_{};
    int64_t chunk_, pos_ = 0;
    std::vector<uint8_t> host_;
    DeviceBuffer words_, xy_, t_, p_, n_, state_;
};

// n-events / n-µs slicing (EventBufferReslicerAlgorithm::Condition::make_n_events /
// make_n_us): slice k = events [bounds[k], bounds[k+1]).  t on the device.
std::vector<int64_t> reslice_n_events(int64_t n, int64_t n_events);
std::vector<int64_t> reslice_n_us(Context &ctx, const int64_t *d_t, int64_t n, int64_t period_us);

// ------------------------------------------------------------------------------ downsample / k-means
struct DownsampleResult {
    std::vector<int32_t> unique_count, repeated_count;  // per window
    std::vector<std::vector<std::pair<int, int>>> unique_coords;  // per window (ascending index)
};

class HashDownsampler {  // process_coordinates + slice path (SMP/…opencl_store.cpp:341-417)
  public:
    explicit HashDownsampler(Context &ctx, const ecc_hash_cfg *cfg = nullptr);
    // device-level: all windows of a batch in one launch
    void run(const uint32_t *d_xy, int64_t n, uint32_t *d_rep_xy, uint32_t *d_rep_idx,
             int32_t *d_unique, int32_t *d_repeated);
    // host convenience: (x,y) pairs in, per-window unique coordinates out
    DownsampleResult process(const std::vector<std::pair<int, int>> &coords);
    const ecc_hash_cfg &config() const { return cfg_; }

  private:
    Context &ctx_;
    ecc_hash_cfg cfg_;
};

// Exact dedup of one window.  FCT/metavision_time_surface_periodic.cpp:
// CoordinateInfo :47-52, analyzeCoordinates :68-120 over the reference's int data[] laid out
// x0, y0, x1, y1, ... (ARRAY_SIZE = 16384 ints).  Returns uniqueCount; `coords` (optional) gets the
// distinct coordinates in first-occurrence order with their counts.  GPU: ecc_dedup_exact.
struct CoordinateInfo {
    int x, y, count;
};
int analyzeCoordinates(Context &ctx, const int *data, int n_ints = 16384, std::vector<CoordinateInfo> *coords = nullptr);

class KMeans {  // assign_to_centers + host loop, "fixed" mode (Appendix A Q7-Q10)
  public:
    KMeans(Context &ctx, int k, int max_iters = 20, float threshold = 50.f, float tol = 1e-3f);
    // host convenience: points (x,y floats), centroids in/out; returns labels (255 = none)
    std::vector<uint8_t> fit(const std::vector<std::array<float, 2>> &points,
                             std::vector<std::array<float, 2>> &centroids, int *iters = nullptr);
    const ecc_kmeans_cfg &config() const { return cfg_; }
    // the reference's own loop ("ref_compat", Appendix A Q7-Q9: 8 centres, <= 16384 points, bins of
    // 2048 never cleared, the ss[j+1] index quirk, the int-abs restart test); returns the passes
    static int fit_ref_compat(Context &ctx, const std::vector<std::array<float, 2>> &points,
                              std::array<float, 16> &centroids, int max_passes = 50,
                              std::array<int32_t, 8> *bin_counts = nullptr);
    // k-means per downsample window, all windows in one launch (ecc_kmeans_windows_xy16): xy holds
    // window w's packed points at w * stride + j, j < counts[w] (counts empty: every window full),
    // and xy.size() is a multiple of stride.  Every window starts from `init` (k centres).
    struct Windows {
        int64_t n_windows = 0;
        std::vector<float> centroids;  // [n_windows * 2k]
        std::vector<uint8_t> labels;   // [n_windows * stride], set for j < counts[w] (else 255)
        std::vector<int32_t> sizes;    // [n_windows * k]
        std::vector<int32_t> iters;    // [n_windows]
    };
    Windows fit_windows(const std::vector<uint32_t> &xy, int64_t stride, const std::vector<int32_t> &counts,
                        const std::vector<std::array<float, 2>> &init);

  private:
    Context &ctx_;
    ecc_kmeans_cfg cfg_;
};

// Per-id displacement of every window's centroids against the previous window's (the reference
// draws it per slice, TWE/…opencl_store.cpp:396-448; ecc_kmeans_windows_flow_host): diff
// [n_windows * 2k] and has_prev [n_windows * k] from KMeans::Windows' centroids and sizes.
struct WindowFlow {
    std::vector<float> diff;
    std::vector<uint8_t> has_prev;
};
WindowFlow window_centroid_flow(const std::vector<float> &centroids, const std::vector<int32_t> &sizes, int k);

// ------------------------------------------------------------------------------ AEClustering
// Host restatement of the reference's downsample consumer:
// DSA/MyCluster.{h,cpp} and DSA/AEClustering.{h,cpp} — a per-event incremental clusterer,
// serial by construction, fed from the GPU downsampler.  Eigen::VectorXd(2) is a
// std::array<double, 2>; arithmetic is the same double-precision expressions.
using Vec2d = std::array<double, 2>;

class MyCluster {  // MyCluster.h:9-77
  public:
    MyCluster();                       // :5-11
    MyCluster(double alpha, int kappa);  // :13-20 (without the constructor print)
    void reset(int kappa, double alpha, int minN);
    // e = {t, x, y, pol}; t relative to t0 is stored; eventId is post-incremented (:26-49)
    void add(const std::deque<double> &e, int &eventId, double t0);
    void forget(double t);             // :51-63, guarded on an empty cluster (Appendix A Q18)
    double manhattanDistance(const Vec2d &x) const;               // :65-68
    double manhattanDistanceWithSampling(const Vec2d &x) const;   // :70-99 (std::rand, as the reference)
    void setN(int n) { n_ = n; }
    void setDatId(const std::deque<int> &v) { datId_ = v; }
    void setDat(const std::deque<Vec2d> &v) { dat_ = v; }
    void setDatT(const std::deque<double> &v) { datT_ = v; }
    void setDatPol(const std::deque<bool> &v) { datPol_ = v; }
    void setMu(const Vec2d &mu) { mu_ = mu; }
    void setMuPrev(const Vec2d &mu) { muPrev_ = mu; }
    void setClusterId(int id) { clusterId_ = id; }
    int getN() const { return n_; }
    const std::deque<int> &getDatId() const { return datId_; }
    const std::deque<Vec2d> &getDat() const { return dat_; }
    const std::deque<double> &getDatT() const { return datT_; }
    const std::deque<bool> &getDatPol() const { return datPol_; }
    Vec2d getClusterCentroid() const;  // :180-195 mean of the stored points
    const Vec2d &getMu() const { return mu_; }
    const Vec2d &getMuPrev() const { return muPrev_; }
    int getClusterId() const { return clusterId_; }

  private:
    std::deque<int> datId_;
    std::deque<Vec2d> dat_;
    std::deque<double> datT_;
    std::deque<bool> datPol_;
    double alpha_ = 0.5;
    Vec2d mu_{0.0, 0.0}, muPrev_{0.0, 0.0};
    int n_ = 0, kappa_ = 0, clusterId_ = 0;
};

class AEClustering {  // AEClustering.h:6-44
  public:
    AEClustering();  // :7-18: minN 10, buffer 800, radius 40, alpha 0.5, kappa 0
    void init(int szBuffer, double radius = 10, int kappa = 10, double alpha = 0.5, int minN = 5);
    // e = {t, x, y, pol}; always returns false, as the reference (:51-125)
    bool update(const std::deque<double> &e);
    int getLastUpdatedClusterIdx() const { return lastUpdatedCluster_; }
    int getMinN() const { return minN_; }
    double t = 0.0;
    std::deque<MyCluster> clusters;

  private:
    void updateBuffer_(double t);                        // :141-149
    void merge_clusters_(const std::deque<int> &assigned);  // :151-211
    int minN_, szBuffer_;
    std::deque<double> tBuffer_;
    double tMin_, radius_, alpha_;
    int kappa_, eventId_;
    double t0_;
    int lastUpdatedCluster_, clusterID_;
};

// The downsample -> clusterer hand-off of DSA/…opencl_store.cpp:428-445 for one window's
// representatives (ascending index): the reference walks the interleaved int array with
// i += 4 while i < diff, i.e. representatives k = 0, 2, 4, ... with 2k < n_reps, each fed as
// {cumulative_unique / 1000.0, x, y, 0} (the fake time axis, Appendix A Q6; per-window counts, Q4).
void aeclustering_feed_window(AEClustering &ae, const std::vector<std::pair<int, int>> &reps,
                              int64_t cumulative_unique);

// Centroid-displacement "flow" (DSA/…opencl_store.cpp:470-518,
// TWE/…opencl_store.cpp:396-448): per slice, every cluster with getN() >= minN gets
// cen = getClusterCentroid(), prev = centroid_prev[id % 16384], diff = cen - prev, drawn as an
// arrow from prev to prev + scale * diff (scale 1 DSA, 3 TWE) when prev.x > 0 && prev.y > 0;
// then centroid_prev[id] = cen.
struct ClusterFlow {
    int cluster_id, n;
    Vec2d centroid, prev, diff;
    bool has_prev;
};

class CentroidFlow {
  public:
    std::vector<ClusterFlow> update(const AEClustering &ae);

  private:
    std::vector<Vec2d> prev_ = std::vector<Vec2d>(16384, Vec2d{0.0, 0.0});  // double centroid_prev[16384][2]
};

// Writers: the per-slice cluster frame the reference draws with OpenCV and saves with
// cv::imwrite (DSA/…opencl_store.cpp:479-555) as a binary PPM (no OpenCV here): points in
// the 10-colour palette by id % 10, centroid green, previous centroid red, flow arrow green.
// CSV: one "x,y,t,cluster" line per clustered point (PCC/pcl_cluster.cpp:140 layout).
bool write_cluster_ppm(const std::string &path, int width, int height, const AEClustering &ae,
                       const std::vector<ClusterFlow> &flow, double arrow_scale = 1.0);
bool write_cluster_csv(const std::string &path, const AEClustering &ae, int minN);

// ------------------------------------------------------------------------------ OPTICS
namespace optics {

struct reachability_dist {  // optics.hpp:57-65
    reachability_dist(std::size_t point_index_, double reach_dist_)
        : point_index(point_index_), reach_dist(reach_dist_) {}
    std::string to_string() const;
    std::size_t point_index;
    double reach_dist;
};
bool operator<(const reachability_dist &lhs, const reachability_dist &rhs);   // :67-69
bool operator==(const reachability_dist &lhs, const reachability_dist &rhs);  // :70-72

// eps-balls, core distances and neighbour lists on the GPU for any number of points in 1-3
// dimensions (ecc_radius_*_f64: one global cell grid, fp64 distances in the reference's
// operation order), the ordered seed-set expansion on the host (sequential by nature,
// :525-555).  The reference's template N (points.size() must equal it, :422-425) is the runtime
// size.  epsilon <= 0: estimated with epsilon_estimation (:428-430).
std::vector<reachability_dist> compute_reachability_dists(
    const std::vector<std::array<int, 2>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    const std::vector<std::array<int, 3>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    const std::vector<std::array<double, 1>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    const std::vector<std::array<double, 2>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    const std::vector<std::array<double, 3>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    Context &ctx, const std::vector<std::array<int, 2>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    Context &ctx, const std::vector<std::array<int, 3>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    Context &ctx, const std::vector<std::array<double, 1>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    Context &ctx, const std::vector<std::array<double, 2>> &points, std::size_t min_pts, double epsilon = -1.0);
std::vector<reachability_dist> compute_reachability_dists(
    Context &ctx, const std::vector<std::array<double, 3>> &points, std::size_t min_pts, double epsilon = -1.0);
// the same over a raw host array of n D-dim points (the ecc_optics_f64 C ABI)
std::vector<reachability_dist> optics_f64_export(ecc_ctx *ctx, ecc_stream_t s, const double *pts, int64_t n, int D,
                                                 std::size_t min_pts, double epsilon);

// The same ordering for many independent windows of packed u16 xy points already on the DEVICE
// (ecc_optics_grid: the whole expansion on the GPU, one launch for all segments; seg_stride
// <= 8192, device_seg_counts null = full segments, epsilon in (0, 32767], min_pts in [1, 64]).
// One vector per segment, point_index local to the segment.  Synchronises the context's stream.
std::vector<std::vector<reachability_dist>> compute_reachability_dists_windows(
    Context &ctx, const uint32_t *device_xy, int64_t n_segs, int64_t seg_stride, const int32_t *device_seg_counts,
    std::size_t min_pts, double epsilon);

template <typename T, std::size_t dimension>
double epsilon_estimation(const std::vector<std::array<T, dimension>> &points, std::size_t min_pts);

std::vector<std::vector<std::size_t>> get_cluster_indices(
    const std::vector<reachability_dist> &reach_dists, double reachability_threshold);

// optics.hpp:803-944 — the xi ("chi") extraction of nested clusters from a reachability plot:
// (begin, end) positions in the ordered plot, inclusive, in the reference's push order
// (ecc_optics_xi_host; no GPU).  chi in (0, 1), steep_area_min_diff in [0, 1), min_pts >= 2.
std::vector<std::pair<std::size_t, std::size_t>> get_chi_clusters_flat(
    const std::vector<reachability_dist> &reach_dists, double chi, std::size_t min_pts,
    double steep_area_min_diff = 0.0);
// The same for many plots already on the DEVICE, laid out as ecc_optics_grid writes `reach`
// (ecc_optics_xi: one launch for all segments, any seg_stride; device_seg_counts null = full
// segments).  One vector of pairs per segment.  Synchronises the context's stream.
std::vector<std::vector<std::pair<std::size_t, std::size_t>>> get_chi_clusters_flat_windows(
    Context &ctx, const double *device_reach, int64_t n_segs, int64_t seg_stride, const int32_t *device_seg_counts,
    double chi, std::size_t min_pts, double steep_area_min_diff = 0.0);

// optics.hpp:692-721 and :760-774 — the points of every threshold cluster / of every xi pair
// (positions begin..end of the ordered plot, inclusive), in plot order.  Error(ECC_ERR_INVALID) for
// a point_index outside `points` or a pair outside the plot (the reference asserts or reads past).
using chi_cluster_indices = std::pair<std::size_t, std::size_t>;  // :50
template <typename T, std::size_t dimension>
std::vector<std::vector<std::array<T, dimension>>> get_cluster_points(
    const std::vector<reachability_dist> &reach_dists, double reachability_threshold,
    const std::vector<std::array<T, dimension>> &points);
template <typename T, std::size_t dimension>
std::vector<std::vector<std::array<T, dimension>>> get_cluster_points(
    const std::vector<reachability_dist> &reach_dists, const std::vector<chi_cluster_indices> &clusters,
    const std::vector<std::array<T, dimension>> &points);

// OPT/test/cluster_event_data.cpp:472-527 — what the reference's event driver prints per cluster:
// its first position in the ordered plot, its size, the centroid sum / size and the per-axis
// variance sum((x - centroid)^2) / size, accumulated in plot order in fp64 as the driver does.
template <std::size_t dimension>
struct cluster_stat {
    std::size_t begin, size;
    std::array<double, dimension> centroid, variance;
};
template <typename T, std::size_t dimension>
std::vector<cluster_stat<dimension>> cluster_statistics(const std::vector<std::array<T, dimension>> &points,
                                                        const std::vector<reachability_dist> &reach_dists,
                                                        double reachability_threshold);
template <typename T, std::size_t dimension>
std::vector<cluster_stat<dimension>> cluster_statistics(const std::vector<std::array<T, dimension>> &points,
                                                        const std::vector<reachability_dist> &reach_dists,
                                                        const std::vector<chi_cluster_indices> &clusters);
// The same for many windows of packed u16 xy points on the DEVICE, on the arrays ecc_optics_grid
// (device_order, device_cluster) and ecc_optics_xi (device_pairs, pair_cap, device_n_pairs) leave
// there: one launch for all segments (ecc_cluster_stats_runs / _pairs; seg_stride <= 8192,
// device_seg_counts null = full segments).  One vector per segment, in run / pair order.
// Synchronises the context's stream.
std::vector<std::vector<cluster_stat<2>>> cluster_statistics_windows(
    Context &ctx, const uint32_t *device_xy, const int32_t *device_order, const int32_t *device_cluster,
    int64_t n_segs, int64_t seg_stride, const int32_t *device_seg_counts);
std::vector<std::vector<cluster_stat<2>>> cluster_statistics_windows(
    Context &ctx, const uint32_t *device_xy, const int32_t *device_order, const int32_t *device_pairs,
    int64_t pair_cap, const int32_t *device_n_pairs, int64_t n_segs, int64_t seg_stride,
    const int32_t *device_seg_counts);

// OPT/include/optics/tree.hpp:11-112 — the value-type tree optics::get_chi_clusters returns: a
// node owns its data and its children, copies are deep.
template <typename T>
class Node {  // tree.hpp:15-54
  public:
    Node(T data) : data_(std::move(data)) {}
    Node(T data, std::vector<Node<T>> children) : data_(std::move(data)), children_(std::move(children)) {}
    T get_data() const { return data_; }
    std::vector<Node<T>> &get_children() { return children_; }
    const std::vector<Node<T>> &get_children() const { return children_; }
    void add_child(const Node<T> &new_child) { children_.push_back(new_child); }
    void add_children(const std::vector<Node<T>> &new_children) {
        children_.insert(children_.end(), new_children.begin(), new_children.end());
    }

  private:
    T data_;
    std::vector<Node<T>> children_;
};

template <typename T>
class Tree {  // tree.hpp:57-79
  public:
    Tree() : root_(T{}) {}
    Tree(Node<T> root) : root_(std::move(root)) {}
    std::vector<T> flatten() const {  // the root, then every subtree in child order
        std::vector<T> result;
        preorder(root_, result);
        return result;
    }
    Node<T> &get_root() { return root_; }
    const Node<T> &get_root() const { return root_; }

  private:
    static void preorder(const Node<T> &node, std::vector<T> &out) {
        out.push_back(node.get_data());
        for (const auto &c : node.get_children()) preorder(c, out);
    }
    Node<T> root_;
};

template <typename T>
std::size_t tree_depth(const Node<T> &root) {  // tree.hpp:82-87: a leaf has depth 1
    std::size_t deepest = 0;
    for (const auto &c : root.get_children()) deepest = std::max(deepest, tree_depth(c));
    return 1 + deepest;
}
template <typename T>
std::size_t tree_size(const Node<T> &root) {  // tree.hpp:89-93
    std::size_t n = 1;
    for (const auto &c : root.get_children()) n += tree_size(c);
    return n;
}
template <typename T>
std::vector<T> flatten_dfs(const Tree<T> &t) {  // tree.hpp:106-112
    return t.flatten();
}

using cluster_tree = Tree<chi_cluster_indices>;  // optics.hpp:51

// optics.hpp:948-995 — the forest of nested clusters of a flat xi list (ecc_optics_xi_tree_host: the
// reference's placement loop and first-parent search, literally; no GPU).  Trees in the
// reference's order, children in the order it adds them.  Error(ECC_ERR_INVALID) for a position
// above INT32_MAX.
std::vector<cluster_tree> flat_clusters_to_tree(const std::vector<chi_cluster_indices> &clusters_flat);
// optics.hpp:1018-1021 — flat_clusters_to_tree(get_chi_clusters_flat(...)), both on the host.
std::vector<cluster_tree> get_chi_clusters(const std::vector<reachability_dist> &reach_dists, double chi,
                                           std::size_t min_pts, double steep_area_min_diff = 0.0);
// The same for many plots already on the DEVICE (ecc_optics_xi, then ecc_optics_xi_tree on the pairs
// it leaves there: one launch each for all segments; arguments as get_chi_clusters_flat_windows).
// One forest per segment.  Synchronises the context's stream.
std::vector<std::vector<cluster_tree>> get_chi_clusters_windows(
    Context &ctx, const double *device_reach, int64_t n_segs, int64_t seg_stride, const int32_t *device_seg_counts,
    double chi, std::size_t min_pts, double steep_area_min_diff = 0.0);

}  // namespace optics

// ------------------------------------------------------------------------------ DBSCAN
struct PointXYZ {  // pcl::PointXYZ
    float x, y, z;
};
struct PointIndices {  // pcl::PointIndices
    std::vector<int> indices;
};

class DBSCANSimpleCluster {  // PCC/DBSCAN_simple.h:14-143 (GPU radius search + extraction, any size)
  public:
    explicit DBSCANSimpleCluster(Context &ctx = Context::default_context()) : ctx_(ctx) {}
    virtual ~DBSCANSimpleCluster() = default;
    virtual void setInputCloud(const std::vector<PointXYZ> &cloud) { cloud_ = cloud; }
    void setClusterTolerance(double tolerance) { eps_ = tolerance; }
    void setMinClusterSize(int min_cluster_size) { min_pts_per_cluster_ = min_cluster_size; }
    void setMaxClusterSize(int max_cluster_size) { max_pts_per_cluster_ = max_cluster_size; }
    void setCorePointMinPts(int core_point_min_pts) { minPts_ = core_point_min_pts; }
    // float x,y,z clouds of any size (ecc_dbscan_cloud_f32); clusters sorted by size,
    // descending (ties: smallest member index first, then creation order)
    void extract(std::vector<PointIndices> &cluster_indices);

  protected:
    // the tolerance the neighbourhoods are built with (radiusSearch(i, eps_, ...), :36, :61)
    virtual double searchTolerance() const { return eps_; }
    Context &ctx_;
    std::vector<PointXYZ> cloud_;
    double eps_{0.0};
    int minPts_{1};
    int min_pts_per_cluster_{1};
    int max_pts_per_cluster_{std::numeric_limits<int>::max()};
};

// DBSCAN_precomp.h:7-55: the adjacency is precomputed in setInputCloud with the tolerance set AT
// THAT TIME (precomp() reads eps_, :28) — a later setClusterTolerance does not change it.  The
// neighbourhoods themselves are the same test as the simple variant's, so extraction is shared.
class DBSCANPrecompCluster : public DBSCANSimpleCluster {
  public:
    using DBSCANSimpleCluster::DBSCANSimpleCluster;
    void setInputCloud(const std::vector<PointXYZ> &cloud) override {
        cloud_ = cloud;
        precomp_eps_ = eps_;
    }

  protected:
    double searchTolerance() const override { return precomp_eps_; }
    double precomp_eps_{0.0};
};

// DBSCANSimpleCluster::extract (DBSCAN_simple.h:27-90) for many windows of packed u16 xy points
// already on the DEVICE, laid out as ecc_downsample_hash leaves them (seg_stride <= 8192,
// device_seg_counts null = full segments): ecc_dbscan_grid, then ecc_dbscan_lists, one launch each
// for all windows; the host only cuts the downloaded rows.  One vector of clusters per window, in
// output order, indices local to the window and ascending (:82).  Synchronises the context's stream.
std::vector<std::vector<PointIndices>> dbscan_extract_windows(Context &ctx, const uint32_t *device_xy, int64_t n_segs,
                                                              int64_t seg_stride, const int32_t *device_seg_counts,
                                                              double eps, int min_pts, int min_cluster_size = 1,
                                                              int max_cluster_size = 1 << 30);
// Size, centroid and per-axis variance of each of those clusters (ecc_cluster_stats_lists: the
// record of optics::cluster_statistics over the list's points in list order; the reference computes
// it for OPTICS clusters only).  begin is the cluster's first position in the window's members row.
std::vector<std::vector<optics::cluster_stat<2>>> dbscan_statistics_windows(
    Context &ctx, const uint32_t *device_xy, int64_t n_segs, int64_t seg_stride, const int32_t *device_seg_counts,
    double eps, int min_pts, int min_cluster_size = 1, int max_cluster_size = 1 << 30);

// Neighbour lists of 2-D integer points (x,y of the cloud) on the GPU: CSR, ascending indices
// (DBSCAN_precomp.h's adjacency row order); any number of points and any min_pts.
void eps_neighbour_lists(Context &ctx, const std::vector<std::array<int, 2>> &points, double eps,
                         std::vector<int64_t> &offsets, std::vector<int32_t> &nbr,
                         int min_pts = 1, std::vector<double> *core_dist = nullptr);

// ---- template definitions
namespace optics {
// optics.hpp:340-387 — bounding box (max initialised from points[1], Q20), uniform-density
// eps for min_pts points per unit ball.
template <typename T, std::size_t dimension>
double epsilon_estimation(const std::vector<std::array<T, dimension>> &points, std::size_t min_pts) {
    if (points.size() <= 1) return 0;
    const double d = static_cast<double>(dimension);
    std::array<T, dimension> mn(points[0]), mx(points[1]);
    for (const auto &p : points)
        for (std::size_t i = 0; i < dimension; i++) {
            if (p[i] < mn[i]) mn[i] = p[i];
            if (p[i] > mx[i]) mx[i] = p[i];
        }
    double volume = 1;
    for (std::size_t i = 0; i < dimension; i++) volume *= std::abs(static_cast<double>(mx[i] - mn[i]));
    const double space_per_minpts = (volume / static_cast<double>(points.size())) * static_cast<double>(min_pts);
    const double unit_ball = std::sqrt(std::pow(M_PI, d)) / std::tgamma(d / 2.0 + 1.0);
    return std::pow(space_per_minpts / unit_ball, 1.0 / d);
}

// optics.hpp:692-721: fplus::elems_at_idxs(cluster_indices, points) per threshold cluster
template <typename T, std::size_t dimension>
std::vector<std::vector<std::array<T, dimension>>> get_cluster_points(
    const std::vector<reachability_dist> &reach_dists, double reachability_threshold,
    const std::vector<std::array<T, dimension>> &points) {
    std::vector<std::vector<std::array<T, dimension>>> result;
    for (const auto &cluster_indices : get_cluster_indices(reach_dists, reachability_threshold)) {
        result.emplace_back();
        result.back().reserve(cluster_indices.size());
        for (std::size_t i : cluster_indices) {
            if (i >= points.size()) throw Error(ECC_ERR_INVALID, "get_cluster_points");
            result.back().push_back(points[i]);
        }
    }
    return result;
}

// optics.hpp:724-739 and :760-774: reach_dists[c.first .. c.second].point_index per pair
template <typename T, std::size_t dimension>
std::vector<std::vector<std::array<T, dimension>>> get_cluster_points(
    const std::vector<reachability_dist> &reach_dists, const std::vector<chi_cluster_indices> &clusters,
    const std::vector<std::array<T, dimension>> &points) {
    std::vector<std::vector<std::array<T, dimension>>> result;
    result.reserve(clusters.size());
    for (const auto &c : clusters) {
        if (c.first > c.second || c.second >= reach_dists.size()) throw Error(ECC_ERR_INVALID, "get_cluster_points");
        result.emplace_back();
        result.back().reserve(c.second - c.first + 1);
        for (std::size_t idx = c.first; idx <= c.second; idx++) {
            const std::size_t i = reach_dists[idx].point_index;
            if (i >= points.size()) throw Error(ECC_ERR_INVALID, "get_cluster_points");
            result.back().push_back(points[i]);
        }
    }
    return result;
}

// cluster_event_data.cpp:493-526 for one cluster's points
template <typename T, std::size_t dimension>
cluster_stat<dimension> cluster_points_statistics(std::size_t begin,
                                                  const std::vector<std::array<T, dimension>> &cluster_points) {
    cluster_stat<dimension> r{begin, cluster_points.size(), {}, {}};
    for (std::size_t a = 0; a < dimension; a++) {
        double sum = 0.0, deviation = 0.0;
        for (const auto &p : cluster_points) sum += p[a];
        r.centroid[a] = sum / cluster_points.size();
        for (const auto &p : cluster_points) {
            const double deviation_diff = p[a] - r.centroid[a];
            deviation += deviation_diff * deviation_diff;
        }
        r.variance[a] = deviation / cluster_points.size();
    }
    return r;
}

template <typename T, std::size_t dimension>
std::vector<cluster_stat<dimension>> cluster_statistics(const std::vector<std::array<T, dimension>> &points,
                                                        const std::vector<reachability_dist> &reach_dists,
                                                        double reachability_threshold) {
    std::vector<cluster_stat<dimension>> result;
    std::size_t begin = 0;
    for (const auto &cluster_points : get_cluster_points(reach_dists, reachability_threshold, points)) {
        result.push_back(cluster_points_statistics(begin, cluster_points));
        begin += cluster_points.size();
    }
    return result;
}

template <typename T, std::size_t dimension>
std::vector<cluster_stat<dimension>> cluster_statistics(const std::vector<std::array<T, dimension>> &points,
                                                        const std::vector<reachability_dist> &reach_dists,
                                                        const std::vector<chi_cluster_indices> &clusters) {
    std::vector<cluster_stat<dimension>> result;
    const auto cluster_points = get_cluster_points(reach_dists, clusters, points);
    for (std::size_t k = 0; k < clusters.size(); k++)
        result.push_back(cluster_points_statistics(clusters[k].first, cluster_points[k]));
    return result;
}
}  // namespace optics

}  // namespace ecc
#pragma GCC visibility pop
