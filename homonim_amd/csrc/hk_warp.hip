// hk_warp.hip -- re-sampling between grids of DIFFERENT coordinate reference systems: what the reference gets from GDAL when
// utils.same_orientation_crs (homonim/utils.py:190-209) wraps the processing-grid image in a WarpedVRT, and RasterArray.reproject
// (homonim/raster_array.py:526-578) with another `crs`.
//
// Per destination pixel: destination geo-transform -> destination CRS inverse -> (lon, lat) -> source CRS forward -> inverse
// source geo-transform = continuous source pixel coordinates (integers = pixel edges), all in float64.  What is then done with
// the coordinate is stated in hk_resample_taps.h, the same functions hk_resample.hip calls: the kernels below get `sx, sy` from
// warp_coord() instead of `k * (j + 0.5) + o`, call them and store.  Every pixel is transformed exactly -- GDAL's default warp
// interpolates the transformation linearly within 0.125 pixel.
//
// CRSs: geographic (degrees) and Transverse Mercator on one ellipsoid (no datum shifts).  Transverse Mercator is the Krueger
// series in the third flattening n to n^6 (Karney 2011, "Transverse Mercator with an accuracy of a few nanometers", eqs. 35 / 36
// for the alpha / beta coefficients): truncation < 1e-12 m on the WGS84 ellipsoid, far below float64 rounding of a 1e7 m
// coordinate.  The six-term series are summed by one complex Clenshaw recurrence from a single sincos(2 xi) and exp(2 eta); the
// inverse takes the conformal latitude to the geodetic one by Newton on tau = tan(phi) (Karney eqs. 7-9, 19-21), three steps from
// tau' / (1 - e^2): the error squares per step from ~e^2, i.e. it is below 1e-20 after the third.
//
// The coordinate kernel (hk_warp_coords*) and the re-samplers call the same warp_coord() with the same arguments under
// -ffp-contract=off: the coordinates a re-sampler uses are, bit for bit, the ones the coordinate kernel returns.
#include "../../include/homonim_hk.h"
#include "hk_kernels.h"
#include "hk_resample_taps.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

namespace hk {

// One CRS, ready for the device.  Passed by value inside the kernel argument struct; alp / bet are indexed by unrolled constants only.
struct CrsParams {
    int kind;        // hk_crs_kind
    double e, e2m;   // first eccentricity, 1 - e^2
    double ka;       // k0 * A: scale factor x rectifying radius
    double xi0;      // xi of the latitude of origin (northing origin on the conformal sphere)
    double lon0;     // central meridian, degrees
    double fe, fn;
    double alp[6], bet[6];
};

// How a destination pixel position becomes a source pixel coordinate: the template parameter of warp_coord() and of everything
// that carries a map.  WARP_AXIS: two CRSs, axis-aligned geo-transforms (hk_warp_desc).  WARP_AFFINE: two CRSs, full six-coefficient
// affines at both ends (rotated / sheared grids).  WARP_AFFINE_SAME: full affines within ONE CRS -- no CRS mathematics at all, so
// it serves CRSs this library cannot define.
enum { WARP_AXIS = 0, WARP_AFFINE = 1, WARP_AFFINE_SAME = 2 };

// geo-transform in Affine order: x = a * col + b * row + c, y = d * col + e * row + f
struct AffineGt {
    double a, b, c, d, e, f;
};

template <int PATH>
struct WarpMapT;
template <>
struct WarpMapT<WARP_AXIS> {
    CrsParams src, dst;
    double dx0, ddx, dy0, ddy;  // destination geo-transform: X = dx0 + col * ddx, Y = dy0 + row * ddy
    double sx0, sdx, sy0, sdy;  // source geo-transform, inverted per pixel: col = (X - sx0) / sdx
};
template <>
struct WarpMapT<WARP_AFFINE> {
    CrsParams src, dst;
    AffineGt d, s;  // destination and source geo-transforms
    double det;     // s.a * s.e - s.b * s.d, formed once on the host
};
template <>
struct WarpMapT<WARP_AFFINE_SAME> {
    AffineGt d, s;
    double det;
};

constexpr double WARP_DEG = 57.295779513082320877;   // degrees per radian
constexpr double WARP_COORD_MAX = 1e15;              // a source coordinate at or beyond this (or NaN) is "no data"

// sum_j c[j] sin(2 (j + 1) (xi + i eta)), real and imaginary part (Clenshaw on the complex argument)
__device__ __forceinline__ void tm_series(const double (&c)[6], double xi, double eta, double& re, double& im) {
    double s0, c0;
    sincos(2.0 * xi, &s0, &c0);
    const double ex = exp(2.0 * eta), exi = 1.0 / ex;
    const double ch0 = 0.5 * (ex + exi), sh0 = 0.5 * (ex - exi);
    const double ar = 2.0 * (c0 * ch0), ai = -2.0 * (s0 * sh0);  // 2 cos(2 zeta)
    double y0r = 0.0, y0i = 0.0, y1r = 0.0, y1i = 0.0;
#pragma unroll
    for (int j = 5; j >= 0; --j) {
        const double tr = ar * y0r - ai * y0i - y1r + c[j];
        const double ti = ar * y0i + ai * y0r - y1i;
        y1r = y0r, y1i = y0i, y0r = tr, y0i = ti;
    }
    const double zr = s0 * ch0, zi = c0 * sh0;  // sin(2 zeta)
    re = zr * y0r - zi * y0i;
    im = zr * y0i + zi * y0r;
}

// tan of the conformal latitude from tan of the geodetic latitude
__device__ __forceinline__ double tm_taup(double tau, double t1 /* sqrt(1 + tau^2) */, double e) {
    const double sig = sinh(e * atanh(e * tau / t1));
    return tau * sqrt(1.0 + sig * sig) - sig * t1;
}

// (lat, lon - lon0) in radians -> (easting, northing); false beyond 90 degrees from the central meridian
__device__ __forceinline__ bool tm_forward(const CrsParams& c, double phi, double dlam, double& x, double& y) {
    const double tau = tan(phi);
    const double tp = tm_taup(tau, sqrt(1.0 + tau * tau), c.e);
    double sl, cl;
    sincos(dlam, &sl, &cl);
    const double xip = atan2(tp, cl), etap = asinh(sl / hypot(tp, cl));
    double zr, zi;
    tm_series(c.alp, xip, etap, zr, zi);
    x = c.fe + c.ka * (etap + zi);
    y = c.fn + c.ka * ((xip + zr) - c.xi0);
    return cl > 0.0;
}

// (easting, northing) -> (lat, lon - lon0) in radians
__device__ __forceinline__ void tm_inverse(const CrsParams& c, double x, double y, double& phi, double& dlam) {
    const double xi = (y - c.fn) / c.ka + c.xi0, eta = (x - c.fe) / c.ka;
    double zr, zi;
    tm_series(c.bet, xi, eta, zr, zi);
    const double xip = xi - zr, etap = eta - zi;
    double s, cx;
    sincos(xip, &s, &cx);
    const double sh = sinh(etap);
    const double tp = s / hypot(sh, cx);
    dlam = atan2(sh, cx);
    double tau = tp / c.e2m;
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const double t1 = sqrt(1.0 + tau * tau);
        const double tpi = tm_taup(tau, t1, c.e);
        tau += (tp - tpi) / sqrt(1.0 + tpi * tpi) * (1.0 + c.e2m * (tau * tau)) / (c.e2m * t1);
    }
    phi = atan(tau);
}

// a longitude (difference) in degrees brought to (-180, 180]
__device__ __forceinline__ double wrap180(double d) {
    d = remainder(d, 360.0);
    return d <= -180.0 ? d + 360.0 : d;
}

// THE coordinate function: destination pixel position (row, col; continuous, integers = pixel edges) -> continuous source pixel
// coordinates; NaN where the position has no image in the source CRS.  The association of every expression is part of the
// contract (the tests restate it): axis-aligned X = dx0 + col * ddx and (x - sx0) / sdx; affine X = (c + col * a) + row * b,
// Y = (f + col * d) + row * e, u = x - s.c, v = y - s.f, column (u * s.e - v * s.b) / det, row (v * s.a - u * s.d) / det.
// The order of the declarations below is the one the axis-aligned builds were first compiled from: with it they compile to the
// same instructions as before the affine paths existed (the compiler's schedule follows the order of the locals).
template <int PATH>
__device__ __forceinline__ void warp_coord(const WarpMapT<PATH>& m, double row, double col, double& sx, double& sy) {
    double X, Y;
    if constexpr (PATH == WARP_AXIS) X = m.dx0 + col * m.ddx, Y = m.dy0 + row * m.ddy;
    else X = (m.d.c + col * m.d.a) + row * m.d.b, Y = (m.d.f + col * m.d.d) + row * m.d.e;
    double lon, lat;  // degrees
    bool ok = true;
    if constexpr (PATH != WARP_AFFINE_SAME) {
        if (m.dst.kind == HK_CRS_GEOGRAPHIC) {
            lon = X, lat = Y;
            ok = fabs(Y) <= 90.0;
        } else {
            double phi, dlam;
            tm_inverse(m.dst, X, Y, phi, dlam);
            lon = m.dst.lon0 + dlam * WARP_DEG, lat = phi * WARP_DEG;
        }
    }
    double x, y;
    if constexpr (PATH == WARP_AFFINE_SAME) {
        x = X, y = Y;  // one CRS: no CRS mathematics
    } else {
        if (m.src.kind == HK_CRS_GEOGRAPHIC) {
            x = wrap180(lon), y = lat;
        } else {
            ok = tm_forward(m.src, lat / WARP_DEG, wrap180(lon - m.src.lon0) / WARP_DEG, x, y) && ok;
        }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if constexpr (PATH == WARP_AXIS) {
        sx = ok ? (x - m.sx0) / m.sdx : nan;
        sy = ok ? (y - m.sy0) / m.sdy : nan;
    } else {
        const double u = x - m.s.c, v = y - m.s.f;
        sx = ok ? (u * m.s.e - v * m.s.b) / m.det : nan;
        sy = ok ? (v * m.s.a - u * m.s.d) / m.det : nan;
    }
}

__device__ __forceinline__ bool warp_coord_usable(double sx, double sy) {
    return fabs(sx) < WARP_COORD_MAX && fabs(sy) < WARP_COORD_MAX;  // false for NaN
}

// ---------------------------------------------------------------------------------------------------------------------
// Thread mapping.  The axis-aligned builds keep one workgroup = 256 consecutive pixels of one destination row: their source
// footprint is a row segment, whatever the CRSs.  Between rotated grids a destination row crosses source rows -- at 90 degrees the
// 64 lanes of a wave would read 64 source rows, one cache line each -- so the affine builds run on a two-dimensional thread tile
// (blockDim.x x blockDim.y = 256, chosen by warp_tile()): a workgroup's source footprint stays compact at any angle.

// a thread's destination row: the launch's row of workgroups (axis-aligned builds), or its place in the tile
template <int PATH>
__device__ __forceinline__ int warp_row() {
    if constexpr (PATH == WARP_AXIS) return blockIdx.y;
    else return blockIdx.y * blockDim.y + threadIdx.y;
}

template <int PATH>
struct WarpCoordArgsT {
    WarpLattice l;
    WarpMapT<PATH> map;
};

template <int PATH>
__global__ void __launch_bounds__(256) warp_coords_kernel(const WarpCoordArgsT<PATH> a) {
    const WarpLattice& l = a.l;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = warp_row<PATH>();
    if (j >= l.w || (PATH != WARP_AXIS && i >= l.h)) return;
    double sx, sy;
    warp_coord(a.map, (double)i + l.off_row, (double)j + l.off_col, sx, sy);
    l.x[(long long)i * l.stride + j] = sx;
    l.y[(long long)i * l.stride + j] = sy;
}

template <int PATH>
struct WarpArgsT {
    ResamplePlanes p;
    double kx, ky;  // source pixels per destination pixel (mean step): pick and scale the stretched kernels
    WarpMapT<PATH> map;
};

// a thread's destination pixel -> its source coordinate and centre pixel; false when the pixel has no image inside the plane
template <int PATH>
__device__ __forceinline__ bool warp_centre(const WarpArgsT<PATH>& a, int i, int j, double& sx, double& sy, long long& cx,
                                            long long& cy) {
    warp_coord(a.map, (double)i + 0.5, (double)j + 0.5, sx, sy);
    return warp_coord_usable(sx, sy) && rs_centre(sx, sy, a.p.sh, a.p.sw, cx, cy);
}

// 0 nearest, 1 bilinear / 3 cubic_spline when no axis is down-sampled; one thread per destination pixel, all bands: what depends
// on the coordinate alone (centre pixel, taps and weights) is formed once, outside the band loop
template <int MODE, int PATH>
__global__ void __launch_bounds__(256) warp_kernel(const WarpArgsT<PATH> a) {
    const ResamplePlanes& p = a.p;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = warp_row<PATH>();
    if (j >= p.dw || (PATH != WARP_AXIS && i >= p.dh)) return;
    double sx, sy;
    long long cx = -1, cy = -1;
    const bool inside = warp_centre(a, i, j, sx, sy, cx, cy);
    Taps2 t = {};
    if constexpr (MODE != 0) {
        if (inside) rs_taps2<MODE>(sx, sy, t);
    }
    for (int b = 0; b < p.n_bands; ++b) {
        const float* __restrict__ sp = p.src + (long long)b * p.src_band_stride;
        double result = 0.0;
        bool got = false;
        float vc;
        if (inside && rs_centre_value(sp, p.src_stride, cx, cy, p.nd_mode, p.nodata, vc)) {
            if constexpr (MODE == 0) result = (double)vc, got = true;
            else got = rs_tap_sum<MODE>(sp, p.src_stride, p.sh, p.sw, p.nd_mode, p.nodata, t, result);
        }
        p.dst[(long long)b * p.dst_band_stride + (long long)i * p.dst_stride + j] = got ? (float)result : p.dst_fill;
    }
}

// GWKResample for any scale: bilinear (1) / cubic (2) / cubic_spline (3) / lanczos (4); threads and bands as in warp_kernel
template <int KIND, int PATH>
__global__ void __launch_bounds__(256) warp_conv_kernel(const WarpArgsT<PATH> a) {
    const ResamplePlanes& p = a.p;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = warp_row<PATH>();
    if (j >= p.dw || (PATH != WARP_AXIS && i >= p.dh)) return;
    const ConvAxis ay = rs_conv_axis<KIND>(a.ky), ax = rs_conv_axis<KIND>(a.kx);
    double sx, sy;
    long long cx = -1, cy = -1;
    const bool inside = warp_centre(a, i, j, sx, sy, cx, cy);
    int iy = 0, ix = 0;
    double dy = 0.0, dx = 0.0;
    if (inside) iy = rs_axis_origin(sy, dy), ix = rs_axis_origin(sx, dx);
    for (int b = 0; b < p.n_bands; ++b) {
        const float* __restrict__ sp = p.src + (long long)b * p.src_band_stride;
        double result = 0.0;
        float vc;
        const bool got = inside && rs_centre_value(sp, p.src_stride, cx, cy, p.nd_mode, p.nodata, vc) &&
                         rs_conv_sum<KIND>(sp, p.src_stride, p.sh, p.sw, p.nd_mode, p.nodata, ay, ax, iy, ix, dy, dx, result);
        p.dst[(long long)b * p.dst_band_stride + (long long)i * p.dst_stride + j] = got ? (float)result : p.dst_fill;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host: descriptor -> device parameters

static bool crs_params(const hk_crs_desc& d, CrsParams& p, const char** why) {
    memset(&p, 0, sizeof(p));
    p.kind = d.kind;
    if (d.kind != HK_CRS_GEOGRAPHIC && d.kind != HK_CRS_TMERC) return *why = "unknown CRS kind", false;
    if (!(d.a > 0.0) || !(d.inv_f == 0.0 || d.inv_f > 1.0) || !isfinite(d.a) || !isfinite(d.inv_f)) return *why = "bad ellipsoid", false;
    p.lon0 = d.lon0, p.fe = d.fe, p.fn = d.fn;
    if (d.kind == HK_CRS_GEOGRAPHIC) return true;
    if (!(d.k0 > 0.0) || !isfinite(d.k0) || !(fabs(d.lat0) <= 90.0) || !isfinite(d.lon0) || !isfinite(d.fe) || !isfinite(d.fn))
        return *why = "bad Transverse Mercator parameters", false;
    const double f = d.inv_f == 0.0 ? 0.0 : 1.0 / d.inv_f, n = f / (2.0 - f);
    const double n2 = n * n, n3 = n2 * n, n4 = n2 * n2, n5 = n4 * n, n6 = n3 * n3;
    p.e = sqrt(f * (2.0 - f)), p.e2m = (1.0 - f) * (1.0 - f);
    p.ka = d.k0 * (d.a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0));
    p.alp[0] = n / 2.0 - 2.0 * n2 / 3.0 + 5.0 * n3 / 16.0 + 41.0 * n4 / 180.0 - 127.0 * n5 / 288.0 + 7891.0 * n6 / 37800.0;
    p.alp[1] = 13.0 * n2 / 48.0 - 3.0 * n3 / 5.0 + 557.0 * n4 / 1440.0 + 281.0 * n5 / 630.0 - 1983433.0 * n6 / 1935360.0;
    p.alp[2] = 61.0 * n3 / 240.0 - 103.0 * n4 / 140.0 + 15061.0 * n5 / 26880.0 + 167603.0 * n6 / 181440.0;
    p.alp[3] = 49561.0 * n4 / 161280.0 - 179.0 * n5 / 168.0 + 6601661.0 * n6 / 7257600.0;
    p.alp[4] = 34729.0 * n5 / 80640.0 - 3418889.0 * n6 / 1995840.0;
    p.alp[5] = 212378941.0 * n6 / 319334400.0;
    p.bet[0] = n / 2.0 - 2.0 * n2 / 3.0 + 37.0 * n3 / 96.0 - n4 / 360.0 - 81.0 * n5 / 512.0 + 96199.0 * n6 / 604800.0;
    p.bet[1] = n2 / 48.0 + n3 / 15.0 - 437.0 * n4 / 1440.0 + 46.0 * n5 / 105.0 - 1118711.0 * n6 / 3870720.0;
    p.bet[2] = 17.0 * n3 / 480.0 - 37.0 * n4 / 840.0 - 209.0 * n5 / 4480.0 + 5569.0 * n6 / 90720.0;
    p.bet[3] = 4397.0 * n4 / 161280.0 - 11.0 * n5 / 504.0 - 830251.0 * n6 / 7257600.0;
    p.bet[4] = 4583.0 * n5 / 161280.0 - 108847.0 * n6 / 3991680.0;
    p.bet[5] = 20648693.0 * n6 / 638668800.0;
    // xi of the latitude of origin: the series on the central meridian (eta = 0)
    const double tau = tan(d.lat0 / WARP_DEG), t1 = sqrt(1.0 + tau * tau);
    const double sig = sinh(p.e * atanh(p.e * tau / t1));
    const double xip = atan(tau * sqrt(1.0 + sig * sig) - sig * t1);
    double xi0 = xip;
    for (int j = 0; j < 6; ++j) xi0 += p.alp[j] * sin(2.0 * (j + 1) * xip);
    p.xi0 = fabs(d.lat0) == 90.0 ? copysign(1.5707963267948966, d.lat0) : xi0;
    return true;
}

static bool warp_map(const hk_warp_desc& d, WarpMapT<WARP_AXIS>& m, const char** why) {
    if (!crs_params(d.src_crs, m.src, why) || !crs_params(d.dst_crs, m.dst, why)) return false;
    if (d.src_crs.a != d.dst_crs.a || d.src_crs.inv_f != d.dst_crs.inv_f)
        return *why = "the two CRSs are on different ellipsoids (no datum shifts)", false;
    for (int k = 0; k < 4; ++k)
        if (!isfinite(d.src_gt[k]) || !isfinite(d.dst_gt[k])) return *why = "geo-transform is not finite", false;
    if (d.src_gt[1] == 0.0 || d.src_gt[3] == 0.0 || d.dst_gt[1] == 0.0 || d.dst_gt[3] == 0.0)
        return *why = "degenerate geo-transform", false;
    m.dx0 = d.dst_gt[0], m.ddx = d.dst_gt[1], m.dy0 = d.dst_gt[2], m.ddy = d.dst_gt[3];
    m.sx0 = d.src_gt[0], m.sdx = d.src_gt[1], m.sy0 = d.src_gt[2], m.sdy = d.src_gt[3];
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// full affines (hk_affine_warp_desc)

static bool affine_gt(const double (&src)[6], const double (&dst)[6], AffineGt& s, AffineGt& d, double& det, const char** why) {
    for (int k = 0; k < 6; ++k)
        if (!isfinite(src[k]) || !isfinite(dst[k])) return *why = "geo-transform is not finite", false;
    s = {src[0], src[1], src[2], src[3], src[4], src[5]};
    d = {dst[0], dst[1], dst[2], dst[3], dst[4], dst[5]};
    det = s.a * s.e - s.b * s.d;
    const double ddet = d.a * d.e - d.b * d.d;
    if (det == 0.0 || ddet == 0.0 || !isfinite(det) || !isfinite(ddet)) return *why = "degenerate geo-transform", false;
    return true;
}

static bool warp_map(const hk_affine_warp_desc& d, WarpMapT<WARP_AFFINE>& m, const char** why) {
    if (!crs_params(d.src_crs, m.src, why) || !crs_params(d.dst_crs, m.dst, why)) return false;
    if (d.src_crs.a != d.dst_crs.a || d.src_crs.inv_f != d.dst_crs.inv_f)
        return *why = "the two CRSs are on different ellipsoids (no datum shifts)", false;
    return affine_gt(d.src_gt, d.dst_gt, m.s, m.d, m.det, why);
}

static bool warp_map(const hk_affine_warp_desc& d, WarpMapT<WARP_AFFINE_SAME>& m, const char** why) {
    return affine_gt(d.src_gt, d.dst_gt, m.s, m.d, m.det, why);
}

// The thread tile of the affine builds, width x height = 256.  32 x 8 is provisional: no measurement has chosen it yet
// (profiles/warp.txt).  HK_WARP_TILE=WxH, read once, overrides it for that measurement (tools/warp_timing.py).  Any tile gives
// the same bits: a thread's pixel is all it sees.
static dim3 warp_tile() {
    static const dim3 tile = [] {
        int w = 32, h = 8, ew = 0, eh = 0;
        const char* e = getenv("HK_WARP_TILE");
        if (e && sscanf(e, "%dx%d", &ew, &eh) == 2 && ew >= 1 && eh >= 1 && ew * eh == 256) w = ew, h = eh;
        return dim3(w, h);
    }();
    return tile;
}

// ---------------------------------------------------------------------------------------------------------------------
// The launch path: descriptor -> map, then the build of PATH that the arguments pick, on PATH's thread mapping (above).  Each
// build is launched under its own spelling, which is its name in the launch ledger (HK_LAUNCH).
template <int PATH>
static dim3 warp_block() {
    return PATH == WARP_AXIS ? dim3(256, 1) : warp_tile();
}
static dim3 warp_grid(dim3 block, int h, int w) { return dim3((w + block.x - 1) / block.x, (h + block.y - 1) / block.y); }

template <int PATH, typename Desc>
static hipError_t launch_coords_path(const Desc* desc, const WarpLattice& l, hipStream_t stream, const char** why) {
    WarpCoordArgsT<PATH> a;
    if (!warp_map(*desc, a.map, why)) return hipErrorInvalidValue;
    a.l = l;
    const dim3 block = warp_block<PATH>(), grid = warp_grid(block, l.h, l.w);
    if constexpr (PATH == WARP_AXIS) HK_LAUNCH(warp_coords_kernel<WARP_AXIS>, grid, block, 0, stream, a);
    else if constexpr (PATH == WARP_AFFINE) HK_LAUNCH(warp_coords_kernel<WARP_AFFINE>, grid, block, 0, stream, a);
    else HK_LAUNCH(warp_coords_kernel<WARP_AFFINE_SAME>, grid, block, 0, stream, a);
    return hipGetLastError();
}

// the build of one path that `mode` (rasterio.enums.Resampling value 0..4) and `stretched` pick.  `path` must be spelled, not a
// template parameter: the parenthesised kernel is the ledger's name of the build, and two builds under one name would hide one.
#define HK_WARP_LAUNCH_MODES(path)                                                                                               \
    switch (mode) {                                                                                                              \
        case 0: HK_LAUNCH((warp_kernel<0, path>), grid, block, 0, stream, a); break;                                             \
        case 1:                                                                                                                  \
            if (stretched) HK_LAUNCH((warp_conv_kernel<1, path>), grid, block, 0, stream, a);                                    \
            else HK_LAUNCH((warp_kernel<1, path>), grid, block, 0, stream, a);                                                   \
            break;                                                                                                               \
        case 2: HK_LAUNCH((warp_conv_kernel<2, path>), grid, block, 0, stream, a); break;                                        \
        case 3:                                                                                                                  \
            if (stretched) HK_LAUNCH((warp_conv_kernel<3, path>), grid, block, 0, stream, a);                                    \
            else HK_LAUNCH((warp_kernel<3, path>), grid, block, 0, stream, a);                                                   \
            break;                                                                                                               \
        case 4: HK_LAUNCH((warp_conv_kernel<4, path>), grid, block, 0, stream, a); break;                                        \
        default: *why = "resampling is not one of nearest / bilinear / cubic / cubic_spline / lanczos"; return hipErrorInvalidValue; \
    }

template <int PATH, typename Desc>
static hipError_t launch_resample_path(int mode, const Desc* desc, const ResamplePlanes& p, double kx, double ky, hipStream_t stream,
                                       const char** why) {
    WarpArgsT<PATH> a;
    if (!warp_map(*desc, a.map, why)) return hipErrorInvalidValue;
    a.p = p, a.kx = kx, a.ky = ky;
    const dim3 block = warp_block<PATH>(), grid = warp_grid(block, p.dh, p.dw);
    const bool stretched = resample_stretched(kx, ky);
    if constexpr (PATH == WARP_AXIS) {
        HK_WARP_LAUNCH_MODES(WARP_AXIS)
    } else if constexpr (PATH == WARP_AFFINE) {
        HK_WARP_LAUNCH_MODES(WARP_AFFINE)
    } else {
        HK_WARP_LAUNCH_MODES(WARP_AFFINE_SAME)
    }
    return hipGetLastError();
}

hipError_t launch_warp_coords(const hk_warp_desc* desc, const WarpLattice& l, hipStream_t stream, const char** why) {
    return launch_coords_path<WARP_AXIS>(desc, l, stream, why);
}

hipError_t launch_warp_coords(const hk_affine_warp_desc* desc, const WarpLattice& l, hipStream_t stream, const char** why) {
    return desc->same_crs ? launch_coords_path<WARP_AFFINE_SAME>(desc, l, stream, why)
                          : launch_coords_path<WARP_AFFINE>(desc, l, stream, why);
}

hipError_t launch_warp_resample(int mode, const hk_warp_desc* desc, const ResamplePlanes& p, double kx, double ky, hipStream_t stream,
                                const char** why) {
    return launch_resample_path<WARP_AXIS>(mode, desc, p, kx, ky, stream, why);
}

hipError_t launch_warp_resample(int mode, const hk_affine_warp_desc* desc, const ResamplePlanes& p, double kx, double ky,
                                hipStream_t stream, const char** why) {
    return desc->same_crs ? launch_resample_path<WARP_AFFINE_SAME>(mode, desc, p, kx, ky, stream, why)
                          : launch_resample_path<WARP_AFFINE>(mode, desc, p, kx, ky, stream, why);
}

}  // namespace hk
