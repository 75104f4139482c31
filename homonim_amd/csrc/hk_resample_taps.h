// hk_resample_taps.h -- the per-tap arithmetic the re-samplers share: the validity test and GDAL's re-sampling kernels as
// functions of the distance.  hk_resample.hip (same-CRS grids) and hk_warp.hip (grids of two CRSs) differ in where a destination
// pixel's source coordinate comes from, not in what is done with it.
#pragma once
#include "hk_kernels.h"

namespace hk {

__device__ __forceinline__ bool rs_valid(float v, int mode, float nodata) {
    return mode == 0 ? true : (mode == 1 ? !(v != v) : !(v == nodata));
}

__device__ __forceinline__ void bspline4(double d, double (&w)[4]) {
    const double a = 1.0 - d, b = 2.0 - d, c = 3.0 - d;
    w[0] = a * a * a / 6.0;
    w[1] = (b * b * b - 4.0 * (a * a * a)) / 6.0;
    w[2] = (c * c * c - 4.0 * (b * b * b) + 6.0 * (a * a * a)) / 6.0;
    w[3] = d * d * d / 6.0;
}

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

}  // namespace hk
