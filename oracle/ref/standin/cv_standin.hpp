// Stand-in for the few OpenCV names the reference's corner filter, tracker and detection lambda
// use (FCT/metavision_time_surface_periodic_group_track.cpp:61-537, :884-1070), so that those spans
// compile verbatim without OpenCV.  TEST INFRASTRUCTURE ONLY.  Our code: written from OpenCV's
// documented behaviour (core/types.hpp, core/mat.hpp, imgproc.hpp).  Every operator names the
// library behaviour it stands for; this arithmetic is the one thing the reference pin takes on
// trust.  Conversions the reference does not use are left out on purpose, so that a
// new use fails to compile instead of getting a guess.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

typedef unsigned char uchar;  // OpenCV's global typedef (core/hal/interface.h)
#define CV_8UC1 0
#define CV_8UC3 16

namespace cv {

// cv::Point_<_Tp>: two public members, a zeroing default constructor and Point_(_Tp x, _Tp y).
// Point2f(int, int) therefore converts each int argument to float at the call (C++ argument
// conversion), which is what `cv::Point2f(corner.x, corner.y)` relies on.
template <typename T>
struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point;      // cv::Point = Point2i
typedef Point_<float> Point2f;

// operator+ : Point_<_Tp>(saturate_cast<_Tp>(a.x + b.x), ...); for float, a.x + b.x is a float sum
// and saturate_cast<float>(float) is the identity: one fp32 rounding per component.
static inline Point2f operator+(const Point2f &a, const Point2f &b) { return Point2f(a.x + b.x, a.y + b.y); }
// operator+= : a.x += b.x; a.y += b.y (fp32).
static inline Point2f &operator+=(Point2f &a, const Point2f &b) {
    a.x += b.x;
    a.y += b.y;
    return a;
}
// operator*(Point_<_Tp>, float): saturate_cast<_Tp>(a.x * b) with a.x * b a float product: the
// multiplication is done in fp32.
static inline Point2f operator*(const Point2f &a, float b) { return Point2f(a.x * b, a.y * b); }
// operator*(Point_<_Tp>, double): a.x * b is a double product; saturate_cast<float>(double) narrows
// it with the current rounding mode.
static inline Point2f operator*(const Point2f &a, double b) { return Point2f((float)(a.x * b), (float)(a.y * b)); }
// operator*=(Point_<_Tp>&, float): a.x = saturate_cast<_Tp>(a.x * b), fp32 product.
static inline Point2f &operator*=(Point2f &a, float b) {
    a.x = a.x * b;
    a.y = a.y * b;
    return a;
}
// operator*=(Point_<_Tp>&, double): double product, narrowed.
static inline Point2f &operator*=(Point2f &a, double b) {
    a.x = (float)(a.x * b);
    a.y = (float)(a.y * b);
    return a;
}
// `int = float` (track.x = pred.x) is plain C++ and truncates toward zero; no stand-in code takes
// part in it.  (OpenCV's Point2f -> Point conversion rounds instead; the reference does not use it
// in these spans and it is not provided.)

// cv::Scalar: four doubles; Scalar(v0) leaves the others 0.
struct Scalar {
    double val[4];
    Scalar(double v0 = 0, double v1 = 0, double v2 = 0, double v3 = 0) : val{v0, v1, v2, v3} {}
};

// cv::Mat, single-channel 8-bit only: Mat::zeros(rows, cols, type) is a zero-filled matrix and
// at<uchar>(row, col) a reference to element (row, col), as in OpenCV (row first).
struct Mat {
    int rows = 0, cols = 0;
    std::vector<uchar> data;
    static Mat zeros(int rows_, int cols_, int /*type*/) {
        Mat m;
        m.rows = rows_;
        m.cols = cols_;
        m.data.assign((std::size_t)rows_ * (std::size_t)cols_, 0);
        return m;
    }
    template <typename T>
    T &at(int row, int col) {
        static_assert(sizeof(T) == 1, "8-bit single-channel only");
        return reinterpret_cast<T &>(data[(std::size_t)row * (std::size_t)cols + (std::size_t)col]);
    }
};

// cv::rectangle(img, pt1, pt2, color, thickness < 0): a FILLED rectangle whose two opposite
// corners are pt1 and pt2, both inclusive, clipped to the image; the value written to an 8-bit
// pixel is saturate_cast<uchar>(color[0]).  Only the filled form is provided.
static inline void rectangle(Mat &img, Point p1, Point p2, const Scalar &color, int thickness) {
    if (thickness >= 0) __builtin_trap();
    int x0 = p1.x < p2.x ? p1.x : p2.x, x1 = p1.x < p2.x ? p2.x : p1.x;
    int y0 = p1.y < p2.y ? p1.y : p2.y, y1 = p1.y < p2.y ? p2.y : p1.y;
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > img.cols - 1) x1 = img.cols - 1;
    if (y1 > img.rows - 1) y1 = img.rows - 1;
    const double c = color.val[0];
    const uchar v = c <= 0 ? 0 : (c >= 255 ? 255 : (uchar)(c + 0.5));
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) img.at<uchar>(y, x) = v;
}

// The detection lambda draws every corner into a display image (:1060); drawing has no effect on
// what it computes, so the image is an empty type and circle a no-op.
struct DisplayImage {};
static inline void circle(DisplayImage &, Point, int, const Scalar &, int) {}

}  // namespace cv
