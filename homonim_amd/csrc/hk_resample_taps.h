// hk_resample_taps.h -- THE statement of what the re-samplers do with a continuous source coordinate (integers = pixel edges):
// GDAL's published warp kernels (gdal/alg/gdalwarpkernel.cpp) restated.  What this file is held to is the exact statement of
// tests/_resample_exact.py -- the same rules in rational arithmetic, sharing no formula with this file -- for every method, on scaled
// grids and on the per-pixel coordinates of hk_warp.hip: identical nodata pattern, the exact-valued methods to the bit, the weighted
// ones within half a float32 ulp plus a derived 2^-40 float64 slack.  The arithmetic is, operation for operation, that of
// oracle/oracle_np.py::reproject, which meets the same statement and to which the tests also hold the kernels bit for bit (lanczos:
// 1e-6, the device's sin) at the large shapes.  hk_resample.hip (same-CRS scaled grids) and
// hk_warp.hip (two CRSs, rotated grids) differ in where a destination pixel's source coordinate comes from and in how threads and
// bands are laid out; what is done with the coordinate is written here only.  Every function takes plain values -- plane pointer,
// stride, shape, nodata rule, coordinates -- and no kernel's argument struct.  (upsample_apply_kernel of hk_resample.hip mirrors
// rs_axis_taps / rs_tap_sum by hand: see there.)
//   nearest                     : the centre pixel (rs_centre, rs_centre_value)
//   bilinear / cubic_spline, up : centre pixel must be valid; separable 2 / 4-tap (cubic B-spline) kernel, invalid or outside taps
//                                 skipped, renormalised by the accumulated weight (rs_taps2, rs_tap_sum)
//   bilinear / cubic / cubic_spline / lanczos, any scale : GDAL's GWKResample (rs_conv_axis, rs_conv_sum)
//   footprint methods           : the source pixels under the destination pixel, clipped to the plane (rs_footprint_axis,
//                                 rs_edge_weight)
// float64 throughout; the callers round the result to float32.
#pragma once
#include "hk_kernels.h"

namespace hk {

__device__ __forceinline__ bool rs_valid(float v, int mode, float nodata) {
    return mode == 0 ? true : (mode == 1 ? !(v != v) : !(v == nodata));
}

// ---------------------------------------------------------------------------------------------------------------------
// the centre pixel: the source pixel that contains the coordinate, per axis (n pixels) and for both; false when it lies outside
// the plane
__device__ __forceinline__ bool rs_centre_axis(double s, int n, long long& c) {
    c = (long long)floor(s + 1e-10);
    return c >= 0 && c < n;
}
__device__ __forceinline__ bool rs_centre(double sx, double sy, int sh, int sw, long long& cx, long long& cy) {
    const bool in_x = rs_centre_axis(sx, sw, cx), in_y = rs_centre_axis(sy, sh, cy);
    return in_x && in_y;
}

// ... and its value in one plane; false when it is nodata (no re-sampler but the footprint ones gives a value then)
__device__ __forceinline__ bool rs_centre_value(const float* __restrict__ sp, long long stride, long long cx, long long cy,
                                                int nd_mode, float nodata, float& v) {
    v = sp[cy * stride + cx];
    return rs_valid(v, nd_mode, nodata);
}

// ---------------------------------------------------------------------------------------------------------------------
// taps of one axis: the origin i = floor(s - 0.5), the pixel whose centre is at or before s, and the fraction d = s - 0.5 - i
__device__ __forceinline__ int rs_axis_origin(double s, double& d) {
    const int i = (int)floor(s - 0.5);
    d = s - 0.5 - (double)i;
    return i;
}

__device__ __forceinline__ void bspline4(double d, double (&w)[4]) {
    const double a = 1.0 - d, b = 2.0 - d, c = 3.0 - d;
    w[0] = a * a * a / 6.0;
    w[1] = (b * b * b - 4.0 * (a * a * a)) / 6.0;
    w[2] = (c * c * c - 4.0 * (b * b * b) + 6.0 * (a * a * a)) / 6.0;
    w[3] = d * d * d / 6.0;
}

// MODE 1 bilinear: RS_NT = 2 taps from the origin; MODE 3 cubic_spline: 4 taps from the pixel before it (RS_T0 = -1)
template <int MODE>
constexpr int RS_NT = MODE == 1 ? 2 : 4;
template <int MODE>
constexpr int RS_T0 = MODE == 1 ? 0 : -1;

// the origin and the RS_NT weights of one axis (unused weights are 0); tap t is pixel origin + RS_T0 + t
template <int MODE>
__device__ __forceinline__ int rs_axis_taps(double s, double (&w)[4]) {
    double d;
    const int i = rs_axis_origin(s, d);
    if constexpr (MODE == 1) {
        w[0] = 1.0 - d, w[1] = d, w[2] = w[3] = 0.0;
    } else {
        bspline4(d, w);
    }
    return i;
}

// both axes: all of the 2 / 4-tap sum that depends on the coordinate and not on the plane (a kernel that loops over bands forms
// it once)
struct Taps2 {
    int iy, ix;
    double wy[4], wx[4];
};
template <int MODE>
__device__ __forceinline__ void rs_taps2(double sx, double sy, Taps2& t) {
    t.iy = rs_axis_taps<MODE>(sy, t.wy);
    t.ix = rs_axis_taps<MODE>(sx, t.wx);
}

// The 2 / 4-tap sum over one plane.  Taps outside the plane or invalid are skipped; nothing is produced when the weight that is
// left is below 1e-6; the sum is divided by it only when it is off 1 by more than 1e-5 (GDAL's rule: interior pixels keep `acc`).
template <int MODE>
__device__ __forceinline__ bool rs_tap_sum(const float* __restrict__ sp, long long stride, int sh, int sw, int nd_mode, float nodata,
                                           const Taps2& t, double& result) {
    double acc = 0.0, wacc = 0.0;
#pragma unroll
    for (int tj = 0; tj < RS_NT<MODE>; ++tj) {
        const int yy = t.iy + RS_T0<MODE> + tj;
        if (yy < 0 || yy >= sh) continue;
#pragma unroll
        for (int ti = 0; ti < RS_NT<MODE>; ++ti) {
            const int xx = t.ix + RS_T0<MODE> + ti;
            if (xx < 0 || xx >= sw) continue;
            const float v = sp[(long long)yy * stride + xx];
            if (!rs_valid(v, nd_mode, nodata)) continue;
            const double wgt = t.wx[ti] * t.wy[tj];
            acc += (double)v * wgt;
            wacc += wgt;
        }
    }
    if (wacc < 1e-6) return false;
    result = (wacc < 0.99999 || wacc > 1.00001) ? acc / wacc : acc;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// GDAL's re-sampling kernels as functions of the (scaled) distance: GWKBilinear / GWKCubic (a = -0.5) / GWKBSpline /
// GWKLanczosSinc (radius 3)
template <int KIND>
__device__ __forceinline__ double conv_weight(double x) {
    const double ax = fabs(x);
    if constexpr (KIND == 1) {
        return ax <= 1.0 ? 1.0 - ax : 0.0;
    } else if constexpr (KIND == 2) {
        const double x2 = ax * ax;
        if (ax <= 1.0) return x2 * (1.5 * ax - 2.5) + 1.0;
        if (ax <= 2.0) return x2 * (-0.5 * ax + 2.5) - 4.0 * ax + 2.0;
        return 0.0;
    } else if constexpr (KIND == 3) {
        if (ax > 2.0) return 0.0;
        const double xp2 = x + 2.0, xp1 = x + 1.0, xm1 = x - 1.0;
        const double a = xp2 > 0.0 ? xp2 * xp2 * xp2 : 0.0, b = xp1 > 0.0 ? xp1 * xp1 * xp1 : 0.0;
        const double c = x > 0.0 ? x * x * x : 0.0, d = xm1 > 0.0 ? xm1 * xm1 * xm1 : 0.0;
        return (a - 4.0 * b + 6.0 * c - 4.0 * d) / 6.0;
    } else {
        if (ax >= 3.0) return 0.0;
        if (x == 0.0) return 1.0;
        const double pi = 3.14159265358979323846, px = pi * x, px3 = px / 3.0;
        return sin(px) * sin(px3) / (px * px3);
    }
}

// GWKResample's support on one axis that steps k source pixels per destination pixel: the kernel of radius R (1, 2, 2, 3 for KIND
// 1..4) is stretched by 1 / scale, scale = min(1, 1 / k), when the axis is down-sampled: taps origin + [1 - r, r], r = ceil(R / scale)
struct ConvAxis {
    double scale;
    int r;
};
template <int KIND>
__device__ __forceinline__ ConvAxis rs_conv_axis(double k) {
    constexpr int R = KIND == 1 ? 1 : (KIND == 4 ? 3 : 2);
    const double scale = k > 1.0 ? 1.0 / k : 1.0;
    return {scale, scale < 1.0 ? (int)ceil((double)R / scale) : R};
}

// The GWKResample sum over one plane, from the origins (iy, ix) and fractions (dy, dx) of rs_axis_origin: weight
// f((tap - fraction) * scale) per axis, taps outside the plane or invalid skipped, always renormalised.
template <int KIND>
__device__ __forceinline__ bool rs_conv_sum(const float* __restrict__ sp, long long stride, int sh, int sw, int nd_mode, float nodata,
                                            ConvAxis cy, ConvAxis cx, int iy, int ix, double dy, double dx, double& result) {
    double acc = 0.0, wacc = 0.0;
    for (int tj = 1 - cy.r; tj <= cy.r; ++tj) {
        const int yy = iy + tj;
        if (yy < 0 || yy >= sh) continue;
        const double wy = conv_weight<KIND>(((double)tj - dy) * cy.scale);
        if (wy == 0.0) continue;
        for (int ti = 1 - cx.r; ti <= cx.r; ++ti) {
            const int xx = ix + ti;
            if (xx < 0 || xx >= sw) continue;
            const float v = sp[(long long)yy * stride + xx];
            if (!rs_valid(v, nd_mode, nodata)) continue;
            const double wgt = conv_weight<KIND>(((double)ti - dx) * cx.scale) * wy;
            acc += (double)v * wgt;
            wacc += wgt;
        }
    }
    if (fabs(wacc) < 1e-6) return false;
    result = acc / wacc;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// One axis of a destination pixel's footprint: its edges e0 < e1 in source coordinates, clipped to the plane's n pixels, and the
// pixels [i0, i1) they touch (at least one where the clipped span is thinner than 1e-10).  False when the span shares no length
// with the plane: a footprint wholly outside it, however close, holds no pixel.
struct FootAxis {
    double p0, p1;
    int i0, i1;
};
__device__ __forceinline__ bool rs_footprint_axis(double e0, double e1, int n, FootAxis& f) {
    f.p0 = fmax(e0, 0.0), f.p1 = fmin(e1, (double)n);
    f.i0 = (int)floor(f.p0 + 1e-10), f.i1 = (int)ceil(f.p1 - 1e-10);
    if (f.i0 == f.i1 && f.i1 < n) ++f.i1;
    return f.i1 > f.i0 && f.i0 >= 0 && f.p1 > f.p0;
}

// the share of pixel p of that axis that the footprint covers: partial at the first and the last pixel, 1 between them and where
// the axis holds a single pixel
__device__ __forceinline__ double rs_edge_weight(const FootAxis& f, int p) {
    if (f.i0 + 1 == f.i1) return 1.0;
    return p == f.i0 ? 1.0 - (f.p0 - (double)f.i0) : (p == f.i1 - 1 ? 1.0 - ((double)f.i1 - f.p1) : 1.0);
}

}  // namespace hk
