// ref_cpu: runs the REFERENCE's own CPU code — the corner filter, tracker and detection lambda of
// FCT/metavision_time_surface_periodic_group_track.cpp, PCC/DBSCAN_simple.h, DSA/AEClustering.cpp +
// MyCluster.cpp — on flat binary files, so that tests can compare the oracle, the host library and
// the device with the reference itself.  TEST INFRASTRUCTURE ONLY; never a product path.
//
// This file is our code.  The reference text is not in it: oracle/ref/Makefile copies the needed
// line spans of the reference files into oracle/_ref/ (git-ignored) at build time, each behind a
// guard on its first and last line, and they are included below where the reference has them: the
// structs and classes at namespace scope, the lambda inside a function that declares the names it
// captures.  The Metavision, OpenCV, PCL and Eigen names those spans use come from the stand-ins
// under oracle/ref/standin/ (our code as well).
//
// Files are raw little-endian arrays.  "Lists" files are int32 words: n_slices, then per slice a
// count followed by count records of 2 (x, y) or 3 (x, y, label) words.  Floats are written as
// their bit patterns.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "cv_standin.hpp"

// Metavision::EventCD (sdk/base/events/event_cd.h): unsigned short x, y; short p; timestamp t, with
// timestamp = std::int64_t (sdk/base/utils/timestamp.h).
namespace Metavision {
using timestamp = std::int64_t;
struct EventCD {
    unsigned short x, y;
    short p;
    timestamp t;
};
}  // namespace Metavision

// Metavision::MostRecentTimestampBuffer(rows, cols, channels = 1): at(y, x) is a reference to the
// timestamp (int64) of pixel (x, y); set_to fills it.
struct TimeSurface {
    int rows_, cols_;
    std::vector<Metavision::timestamp> v;
    TimeSurface(int rows, int cols) : rows_(rows), cols_(cols), v((std::size_t)rows * cols, 0) {}
    Metavision::timestamp &at(int y, int x) {
        if (y < 0 || y >= rows_ || x < 0 || x >= cols_) {  // the reference reads 4 px around non-border events only
            std::fprintf(stderr, "ref_cpu: time surface access (%d, %d) outside %dx%d\n", y, x, rows_, cols_);
            std::exit(3);
        }
        return v[(std::size_t)y * cols_ + x];
    }
};

#include "gt_circles.inc"  // FCT/…group_track.cpp:44-45  (circle3_, circle4_)
#include "gt_classes.inc"  // FCT/…group_track.cpp:61-537 (Corner … CornerTracker)

#include "DBSCAN_simple.h"  // the reference's header, found through -I, behind standin/pcl/point_types.h
#include "AEClustering.h"   // likewise, behind standin/eigen3/Eigen

namespace {

constexpr int kW = 1280, kH = 720;  // the lambda hard-codes this border (:952-953)
constexpr int ARRAY_SIZE = 1 << 14;  // the name the lambda's coordinate ring wraps at (its value in main())

[[noreturn]] void die(const std::string &m) {
    std::fprintf(stderr, "ref_cpu: %s\n", m.c_str());
    std::exit(2);
}

template <typename T>
std::vector<T> read_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) die(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)sizeof(T)) die(std::string("bad size: ") + path);
    std::vector<T> v((std::size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) die(std::string("short read: ") + path);
    std::fclose(f);
    return v;
}

template <typename T>
void write_file(const char *path, const std::vector<T> &v) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f) die(std::string("cannot create ") + path);
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) die(std::string("short write: ") + path);
    std::fclose(f);
}

struct Words {
    std::vector<int32_t> w;
    void i(int v) { w.push_back((int32_t)v); }
    void f(float v) {
        int32_t b;
        std::memcpy(&b, &v, 4);
        w.push_back(b);
    }
};

// ---- the detection lambda -----------------------------------------------------------------
// The names the lambda captures by reference, as main() declares them (:749, :776-799).
struct ArcState {
    TimeSurface time_surface{kH, kW};
    std::mutex frame_mutex;
    std::vector<int> data_store = std::vector<int>((std::size_t)ARRAY_SIZE * 2);
    int data_index = 0;
    Metavision::timestamp last_time = 0;
    int time_surface_flag = 0;
    cv::DisplayImage corner_img;
    std::vector<Corner> corners;
};

void run_lambda(ArcState &S, const Metavision::EventCD *first, const Metavision::EventCD *last) {
    TimeSurface &time_surface = S.time_surface;
    std::mutex &frame_mutex = S.frame_mutex;
    int *data = S.data_store.data();
    int &data_index = S.data_index;
    Metavision::timestamp &last_time = S.last_time;
    int &time_surface_flag = S.time_surface_flag;
    cv::DisplayImage &corner_img = S.corner_img;
    std::vector<Corner> &corners = S.corners;
#include "gt_lambda.inc"  // FCT/…group_track.cpp:884-1070: auto aggregate_events_fct = [&](…) { … };
    aggregate_events_fct(first, last);
    (void)last_time;
}

std::vector<Metavision::EventCD> load_events(const char *xy_path, const char *t_path) {
    const auto xy = read_file<uint32_t>(xy_path);
    const auto t = read_file<int64_t>(t_path);
    if (xy.size() != t.size()) die("xy and t differ in length");
    std::vector<Metavision::EventCD> ev(xy.size());
    for (std::size_t i = 0; i < xy.size(); ++i) {
        const unsigned x = xy[i] & 0xffffu, y = xy[i] >> 16;
        if (x >= (unsigned)kW || y >= (unsigned)kH) die("event outside 1280x720");
        ev[i] = Metavision::EventCD{(unsigned short)x, (unsigned short)y, 0, t[i]};
    }
    return ev;
}

void put_list(Words &o, const std::vector<Corner> &c, bool with_label) {
    o.i((int)c.size());
    for (const Corner &k : c) {
        o.i(k.x);
        o.i(k.y);
        if (with_label) o.i(k.label);
    }
}

std::vector<std::vector<Corner>> get_lists(const std::vector<int32_t> &w, int rec) {
    std::size_t p = 0;
    auto next = [&]() {
        if (p >= w.size()) die("lists file truncated");
        return w[p++];
    };
    const int ns = next();
    std::vector<std::vector<Corner>> out((std::size_t)ns);
    for (int s = 0; s < ns; ++s) {
        const int n = next();
        for (int k = 0; k < n; ++k) {
            Corner c{};
            c.x = next();
            c.y = next();
            c.label = rec == 3 ? next() : 0;
            out[(std::size_t)s].push_back(c);
        }
    }
    return out;
}

// Every TrackedCorner field and the groups after one updateTrackedCorners:
// n_tracks, then per track x, y, label, frame_count, is_matched, frames_since_last_detection,
// group_id, |history|, the history (x, y) front to back, velocity, direction.current,
// direction.target, damping, smoothing; then n_groups and per group (map order) id, |labels|,
// average_velocity, centroid, radius, the labels.
void put_tracker(Words &o, const std::vector<TrackedCorner> &tr, const std::map<int, CornerGroup> &groups) {
    o.i((int)tr.size());
    for (const TrackedCorner &t : tr) {
        o.i(t.x); o.i(t.y); o.i(t.label); o.i(t.frame_count); o.i(t.is_matched ? 1 : 0);
        o.i(t.frames_since_last_detection); o.i(t.group_id); o.i((int)t.position_history.size());
        for (const cv::Point &p : t.position_history) { o.i(p.x); o.i(p.y); }
        o.f(t.velocity.x); o.f(t.velocity.y);
        o.f(t.direction.current.x); o.f(t.direction.current.y);
        o.f(t.direction.target.x); o.f(t.direction.target.y);
        o.f(t.direction.damping); o.f(t.direction.smoothing);
    }
    o.i((int)groups.size());
    for (const auto &kv : groups) {
        const CornerGroup &g = kv.second;
        o.i(kv.first); o.i((int)g.corner_labels.size());
        o.f(g.average_velocity.x); o.f(g.average_velocity.y);
        o.f(g.centroid.x); o.f(g.centroid.y); o.f(g.radius);
        for (int l : g.corner_labels) o.i(l);
    }
}

// The command-line interface's number, printed by `ref_cpu api` (tests/ref_cpu_cases.py:REF_CPU_API):
// a binary left in oracle/_ref/ by another revision of this file answers another number or none.
// 2: track takes a configuration.
constexpr int kRefCpuApi = 2;

CornerTracker make_tracker() {  // as main() constructs it (:805-813)
    return CornerTracker(30.0f, 30, 10, 5, 0.8f, 0.3f, 100.0f);
}

// arc XY T SLICE FLAG0 SAE_IN|- OUT_CORNERS OUT_SAE
// chain XY T SLICE OUT_CORNERS OUT_NMS OUT_TRACK OUT_SAE
int cmd_arc(int argc, char **argv, bool chain) {
    if (argc != 9) die("arc/chain: wrong argument count");
    const auto ev = load_events(argv[2], argv[3]);
    const long slice = std::atol(argv[4]);
    if (slice <= 0) die("slice must be positive");
    ArcState S;
    const char *out_corners, *out_sae, *out_nms = nullptr, *out_track = nullptr;
    if (chain) {
        out_corners = argv[5]; out_nms = argv[6]; out_track = argv[7]; out_sae = argv[8];
    } else {
        S.time_surface_flag = std::atoi(argv[5]);
        if (std::strcmp(argv[6], "-")) {
            const auto in = read_file<int64_t>(argv[6]);
            if (in.size() != S.time_surface.v.size()) die("initial surface has the wrong size");
            S.time_surface.v = in;
        }
        out_corners = argv[7]; out_sae = argv[8];
    }
    CornerTracker tracker = make_tracker();
    const long ns = ((long)ev.size() + slice - 1) / slice;
    Words oc, on, ot;
    oc.i((int)ns); on.i((int)ns); ot.i((int)ns);
    for (long s = 0; s < ns; ++s) {
        const long lo = s * slice, hi = std::min<long>((long)ev.size(), lo + slice);
        run_lambda(S, ev.data() + lo, ev.data() + hi);  // the reslicer's event callback for the slice
        put_list(oc, S.corners, false);
        // the on-new-slice callback (:815-882): filter, track, then flag / clear
        if (chain) {
            std::vector<Corner> filtered = CornerFilter::filterCorners(S.corners, kW, kH, 15, 0.5f);  // :832-838
            put_list(on, filtered, true);
            std::vector<TrackedCorner> tracked = tracker.updateTrackedCorners(filtered);  // :847
            put_tracker(ot, tracked, tracker.getCornerGroups());                         // :850
        }
        S.time_surface_flag = 1;  // :878
        S.corners.clear();        // :881
    }
    write_file(out_corners, oc.w);
    write_file(out_sae, S.time_surface.v);
    if (chain) {
        write_file(out_nms, on.w);
        write_file(out_track, ot.w);
    }
    return 0;
}

// nms IN_LISTS(x, y) W H OUT_LISTS(x, y, label)
int cmd_nms(int argc, char **argv) {
    if (argc != 6) die("nms: wrong argument count");
    const auto in = get_lists(read_file<int32_t>(argv[2]), 2);
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
    Words o;
    o.i((int)in.size());
    for (const auto &c : in) {
        for (const Corner &k : c)  // filterCorners indexes the mask without a check: corners must be inside
            if (k.x < 0 || k.x >= W || k.y < 0 || k.y >= H) die("nms: corner outside the image");
        put_list(o, CornerFilter::filterCorners(c, W, H, 15, 0.5f), true);
    }
    write_file(argv[5], o.w);
    return 0;
}

// The constructor's seven arguments as one word each, comma-separated hex: max_distance (float
// bits), max_frames, history_size, frames_to_skip (int bits), damping, smoothing, group_radius
// (float bits).  Bit patterns, so that NaN and an exact radius arrive as they were meant.
CornerTracker make_tracker(const char *cfg) {
    uint32_t w[7];
    const char *q = cfg;
    for (int k = 0; k < 7; ++k) {
        char *end = nullptr;
        w[k] = (uint32_t)std::strtoul(q, &end, 16);
        if (end == q || *end != (k < 6 ? ',' : '\0')) die("track: the configuration is seven hex words");
        q = end + 1;
    }
    const auto f = [&](int k) { float v; std::memcpy(&v, &w[k], 4); return v; };
    return CornerTracker(f(0), (int)w[1], (int)w[2], (int)w[3], f(4), f(5), f(6));
}

// track IN_LISTS(x, y, label) OUT_DUMP [CFG]
int cmd_track(int argc, char **argv) {
    if (argc != 4 && argc != 5) die("track: wrong argument count");
    const auto in = get_lists(read_file<int32_t>(argv[2]), 3);
    CornerTracker tracker = argc == 5 ? make_tracker(argv[4]) : make_tracker();
    Words o;
    o.i((int)in.size());
    for (const auto &c : in) {
        std::vector<TrackedCorner> tracked = tracker.updateTrackedCorners(c);
        put_tracker(o, tracked, tracker.getCornerGroups());
    }
    write_file(argv[3], o.w);
    return 0;
}

// dbscan PTS(float x, y, z) EPS MIN_PTS MIN_SIZE MAX_SIZE OUT: n_clusters, the sizes, the indices
int cmd_dbscan(int argc, char **argv) {
    if (argc != 8) die("dbscan: wrong argument count");
    const auto p = read_file<float>(argv[2]);
    if (p.size() % 3) die("dbscan: points are float triples");
    pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>);
    for (std::size_t i = 0; i < p.size(); i += 3) {
        pcl::PointXYZ q;
        q.x = p[i]; q.y = p[i + 1]; q.z = p[i + 2];
        cloud->points.push_back(q);
    }
    pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>);
    std::vector<pcl::PointIndices> clusters;
    DBSCANSimpleCluster<pcl::PointXYZ> ec;  // the calls of PCC/pcl_cluster.cpp:112-123
    ec.setCorePointMinPts(std::atoi(argv[4]));
    ec.setClusterTolerance(std::atof(argv[3]));
    ec.setMinClusterSize(std::atoi(argv[5]));
    ec.setMaxClusterSize(std::atoi(argv[6]));
    ec.setSearchMethod(tree);
    ec.setInputCloud(cloud);
    ec.extract(clusters);
    Words o;
    o.i((int)clusters.size());
    for (const auto &c : clusters) o.i((int)c.indices.size());
    for (const auto &c : clusters)
        for (int i : c.indices) o.i(i);
    write_file(argv[7], o.w);
    return 0;
}

// aec FEED(double t, x, y per update) WIN_COUNTS(int32 updates per window) OUT(double)
// A default-constructed AEClustering (the driver's, DSA/…opencl_store.cpp:42) gets one update per
// feed row, e = {t, x, y, 0} (:439-444).  After each window: the number of clusters, then per
// cluster in deque order its id, n, getClusterCentroid() and getMu().
int cmd_aec(int argc, char **argv) {
    if (argc != 5) die("aec: wrong argument count");
    const auto feed = read_file<double>(argv[2]);
    const auto wins = read_file<int32_t>(argv[3]);
    std::cout.setstate(std::ios_base::failbit);  // the classes narrate every cluster on std::cout
    AEClustering ae;
    std::vector<double> o;
    std::size_t r = 0;
    for (int32_t n : wins) {
        for (int32_t k = 0; k < n; ++k, ++r) {
            if (3 * r + 2 >= feed.size()) die("aec: feed shorter than the window counts");
            std::deque<double> e(4, 0.0);
            e[0] = feed[3 * r]; e[1] = feed[3 * r + 1]; e[2] = feed[3 * r + 2]; e[3] = 0;
            ae.update(e);
        }
        o.push_back((double)ae.clusters.size());
        for (auto cc : ae.clusters) {  // by value, as the driver iterates (:466)
            Eigen::VectorXd cen(cc.getClusterCentroid());
            Eigen::VectorXd mu(cc.getMu());
            o.push_back(cc.getClusterId()); o.push_back(cc.getN());
            o.push_back(cen[0]); o.push_back(cen[1]); o.push_back(mu[0]); o.push_back(mu[1]);
        }
    }
    write_file(argv[4], o);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) die("usage: ref_cpu api|arc|chain|nms|track|dbscan|aec …");
    const std::string c = argv[1];
    if (c == "api") { std::printf("%d\n", kRefCpuApi); return 0; }
    if (c == "arc") return cmd_arc(argc, argv, false);
    if (c == "chain") return cmd_arc(argc, argv, true);
    if (c == "nms") return cmd_nms(argc, argv);
    if (c == "track") return cmd_track(argc, argv);
    if (c == "dbscan") return cmd_dbscan(argc, argv);
    if (c == "aec") return cmd_aec(argc, argv);
    die("unknown subcommand " + c);
}
