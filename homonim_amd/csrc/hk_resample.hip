// hk_resample.hip -- re-sampling between same-CRS, north-up, axis-aligned grids: RasterArray.reproject
// (homonim/raster_array.py:526-578 -> rasterio.warp.reproject -> GDAL warp) as RefSpaceModel / SrcSpaceModel use it
// (homonim/kernel_model.py:397,480,491,497,520), and RefSpaceModel.apply fused with its up-sampling.
//
// GDAL is not part of the reference project and not installed here: its published warp kernels are RESTATED, parity with GDAL
// itself unpinned.  What is done with a source coordinate is stated once, in hk_resample_taps.h; this file supplies the coordinate
//   mapping : src_col = kx * dst_col + ox, src_row = ky * dst_row + oy on continuous coordinates (integers = pixel edges)
// and the methods that need a scaled mapping's rectangular footprint (the destination pixel's edges mapped and clipped to the plane):
//   5 average      : weighted mean of the valid source pixels under the footprint, edge pixels by their overlap
//   8 max / 9 min / 13 sum / 14 rms : over the same pixels; sum and rms weight the edge pixels like average
//   6 mode / 10 med / 11 q1 / 12 q3 : rank order of the same pixels, no weights
// One thread per destination pixel (gather), one row per workgroup, one band per blockIdx.z; float64 accumulation, float32 result.
// footprint_typed_kernel<T> is `average` on a plane of any sample type as it was uploaded, with the coverage fraction of its valid
// mask from the same loop (hk_srcspace_fit_apply: the reference block of SrcSpaceModel.fit is read once).
#include "hk_kernels.h"
#include "hk_resample_taps.h"

namespace hk {

struct ResampleArgs {
    ResamplePlanes p;
    double kx, ox, ky, oy;
};

// the mapping on one axis: destination position (pixel index = its leading edge, + 0.5 = its centre) -> source coordinate
__device__ __forceinline__ double scaled_coord(double k, double o, double pos) { return k * pos + o; }

// 0 nearest, 1 bilinear / 3 cubic_spline when no axis is down-sampled, and the footprint methods
template <int MODE>
__global__ void __launch_bounds__(256) resample_kernel(const ResampleArgs a) {
    const ResamplePlanes& p = a.p;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= p.dw) return;
    const float* __restrict__ sp = p.src + (long long)blockIdx.z * p.src_band_stride;
    float* __restrict__ dp = p.dst + (long long)blockIdx.z * p.dst_band_stride;
    double result = 0.0;
    bool got = false;
    if constexpr (MODE >= 5) {
        FootAxis fy, fx;
        // the destination pixel's leading and trailing edges on each axis
        const bool rows = rs_footprint_axis(scaled_coord(a.ky, a.oy, (double)i), scaled_coord(a.ky, a.oy, (double)(i + 1)), p.sh, fy);
        const bool cols = rs_footprint_axis(scaled_coord(a.kx, a.ox, (double)j), scaled_coord(a.kx, a.ox, (double)(j + 1)), p.sw, fx);
        if (rows && cols) {  // shares area with the plane
            if constexpr (MODE == 5 || MODE == 8 || MODE == 9 || MODE == 13 || MODE == 14) {
                double tot = 0.0, wsum = 0.0;
                for (int yy = fy.i0; yy < fy.i1; ++yy) {
                    const double wy = rs_edge_weight(fy, yy);
                    for (int xx = fx.i0; xx < fx.i1; ++xx) {
                        const float v = sp[(long long)yy * p.src_stride + xx];
                        if (!rs_valid(v, p.nd_mode, p.nodata)) continue;
                        const double wgt = rs_edge_weight(fx, xx) * wy;
                        if constexpr (MODE == 8) {
                            tot = wsum > 0.0 ? fmax(tot, (double)v) : (double)v;
                        } else if constexpr (MODE == 9) {
                            tot = wsum > 0.0 ? fmin(tot, (double)v) : (double)v;
                        } else if constexpr (MODE == 14) {
                            tot += (double)v * (double)v * wgt;
                        } else {
                            tot += (double)v * wgt;
                        }
                        wsum += wgt;
                    }
                }
                if (wsum > 0.0) {
                    result = (MODE == 5) ? tot / wsum : ((MODE == 14) ? sqrt(tot / wsum) : tot);
                    got = true;
                }
            } else {
                // GWKAverageOrMode's rank-order branches (no weights): med / q1 / q3 = element ceil(q * n - 1) of the sorted valid
                // values; mode = the value whose running count first reaches the highest count, in row-major scan order.  No
                // per-thread storage: the footprint (a few dozen pixels, cache-resident) is scanned once per candidate.
                static_assert(MODE == 6 || MODE == 10 || MODE == 11 || MODE == 12, "not a resampling method of this kernel");
                int n = 0;
                for (int yy = fy.i0; yy < fy.i1; ++yy)
                    for (int xx = fx.i0; xx < fx.i1; ++xx)
                        n += rs_valid(sp[(long long)yy * p.src_stride + xx], p.nd_mode, p.nodata) ? 1 : 0;
                if (n > 0) {
                    constexpr double q = MODE == 10 ? 0.5 : (MODE == 11 ? 0.25 : 0.75);
                    int want = (int)ceil(q * (double)n - 1.0);
                    want = want < 0 ? 0 : want;
                    int best_cnt = 0, best_last = 0;
                    for (int yc = fy.i0; yc < fy.i1 && !(MODE != 6 && got); ++yc) {
                        for (int xc = fx.i0; xc < fx.i1; ++xc) {
                            const float c = sp[(long long)yc * p.src_stride + xc];
                            if (!rs_valid(c, p.nd_mode, p.nodata)) continue;
                            int less = 0, equal = 0, last = 0, pos = 0;
                            for (int yy = fy.i0; yy < fy.i1; ++yy)
                                for (int xx = fx.i0; xx < fx.i1; ++xx, ++pos) {
                                    const float v = sp[(long long)yy * p.src_stride + xx];
                                    if (!rs_valid(v, p.nd_mode, p.nodata)) continue;
                                    less += v < c ? 1 : 0;
                                    if (v == c) ++equal, last = pos;
                                }
                            if constexpr (MODE == 6) {
                                // the value that reaches the highest count first = most occurrences, then earliest last occurrence
                                if (equal > best_cnt || (equal == best_cnt && last < best_last))
                                    best_cnt = equal, best_last = last, result = (double)c, got = true;
                            } else if (less <= want && want < less + equal) {
                                result = (double)c, got = true;
                                break;
                            }
                        }
                    }
                }
            }
        }
    } else {
        static_assert(MODE == 0 || MODE == 1 || MODE == 3, "not a resampling method of this kernel");
        const double sy = scaled_coord(a.ky, a.oy, (double)i + 0.5), sx = scaled_coord(a.kx, a.ox, (double)j + 0.5);
        long long cx, cy;
        float vc;
        if (rs_centre(sx, sy, p.sh, p.sw, cx, cy) && rs_centre_value(sp, p.src_stride, cx, cy, p.nd_mode, p.nodata, vc)) {
            if constexpr (MODE == 0) {
                result = (double)vc, got = true;
            } else {
                Taps2 t;
                rs_taps2<MODE>(sx, sy, t);
                got = rs_tap_sum<MODE>(sp, p.src_stride, p.sh, p.sw, p.nd_mode, p.nodata, t, result);
            }
        }
    }
    dp[(long long)i * p.dst_stride + j] = got ? (float)result : p.dst_fill;
}

// GWKResample for any scale: bilinear (1) / cubic (2) / cubic_spline (3) / lanczos (4)
template <int KIND>
__global__ void __launch_bounds__(256) resample_conv_kernel(const ResampleArgs a) {
    const ResamplePlanes& p = a.p;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= p.dw) return;
    const float* __restrict__ sp = p.src + (long long)blockIdx.z * p.src_band_stride;
    float* __restrict__ dp = p.dst + (long long)blockIdx.z * p.dst_band_stride;
    const double sy = scaled_coord(a.ky, a.oy, (double)i + 0.5), sx = scaled_coord(a.kx, a.ox, (double)j + 0.5);
    long long cx, cy;
    float vc;
    double result = 0.0;
    bool got = false;
    if (rs_centre(sx, sy, p.sh, p.sw, cx, cy) && rs_centre_value(sp, p.src_stride, cx, cy, p.nd_mode, p.nodata, vc)) {
        double dy, dx;
        const int iy = rs_axis_origin(sy, dy), ix = rs_axis_origin(sx, dx);
        got = rs_conv_sum<KIND>(sp, p.src_stride, p.sh, p.sw, p.nd_mode, p.nodata, rs_conv_axis<KIND>(a.ky), rs_conv_axis<KIND>(a.kx),
                                iy, ix, dy, dx, result);
    }
    dp[(long long)i * p.dst_stride + j] = got ? (float)result : p.dst_fill;
}

// `average` of a plane of sample type T as it was uploaded, and the coverage fraction of its valid mask, from ONE pass over the
// typed pixels under the footprint (SrcSpaceModel.fit across grids, kernel_model.py:520 and :375-409: the reference block is the
// big input there).  The value is resample_kernel<5> on the plane cast_in_kernel<T> would have written: the same (float) conversion,
// in registers, the same loop and accumulation order.  The coverage is resample_kernel<5> without nodata on the plane
// valid_plane_kernel would have written from that: sum of w * [valid] over sum of w, over ALL pixels of the clipped footprint.
// One loop serves both: an invalid pixel adds w * 0.0 = +0.0 there, which changes no bit of a sum of non-negative terms, and a
// valid one adds w * 1.0 = w, so the numerator is `wsum`, the weight sum of the value, bit for bit; only the denominator `wall`
// is new.  A footprint that shares no area with the plane gets `fill` and coverage 0.
template <typename T>
__global__ void __launch_bounds__(256) footprint_typed_kernel(const FootTypedArgs<T> a) {
    typedef __attribute__((address_space(1))) const T gT;
    typedef __attribute__((address_space(1))) float gfloat;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= a.dw) return;
    gT* const sp = (gT*)a.src;
    double tot = 0.0, wsum = 0.0, wall = 0.0;
    FootAxis fy, fx;
    const bool rows = rs_footprint_axis(scaled_coord(a.ky, a.oy, (double)i), scaled_coord(a.ky, a.oy, (double)(i + 1)), a.sh, fy);
    const bool cols = rs_footprint_axis(scaled_coord(a.kx, a.ox, (double)j), scaled_coord(a.kx, a.ox, (double)(j + 1)), a.sw, fx);
    if (rows && cols) {
        for (int yy = fy.i0; yy < fy.i1; ++yy) {
            const double wy = rs_edge_weight(fy, yy);
            gT* const row = sp + (long long)yy * a.src_stride;
            for (int xx = fx.i0; xx < fx.i1; ++xx) {
                const float v = (float)row[xx];
                const double wgt = rs_edge_weight(fx, xx) * wy;
                wall += wgt;
                if (!rs_valid(v, a.nd_mode, a.nodata)) continue;
                tot += (double)v * wgt;
                wsum += wgt;
            }
        }
    }
    const long long o = (long long)i * a.dst_stride + j;
    ((gfloat*)a.value)[o] = wsum > 0.0 ? (float)(tot / wsum) : a.fill;
    if (a.coverage) ((gfloat*)a.coverage)[o] = wall > 0.0 ? (float)(wsum / wall) : 0.f;
}

// valid(src) as a float32 0/1 plane: RasterArray.mask_ra (raster_array.py:320-327) before it is re-projected
__global__ void __launch_bounds__(256) valid_plane_kernel(const float* __restrict__ in, long long in_stride, int nd_mode,
                                                          float nodata, float* __restrict__ out, long long out_stride,
                                                          int height, int width) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width) return;
    for (int y = blockIdx.y; y < height; y += gridDim.y)
        out[(long long)y * out_stride + x] = rs_valid(in[(long long)y * in_stride + x], nd_mode, nodata) ? 1.f : 0.f;
}

// RefSpaceModel.apply after the parameters were brought to the source grid (kernel_model.py:493-503): parameters are
// masked with the (nearest re-projected) full-coverage mask, or with the source mask, then gain * src + offset.
__global__ void __launch_bounds__(256) apply_space_kernel(const float* __restrict__ src, long long src_stride, int nd_mode,
                                                          float nodata, const float* __restrict__ gain,
                                                          const float* __restrict__ offset, long long par_stride,
                                                          const float* __restrict__ keep, float* __restrict__ out,
                                                          long long out_stride, int height, int width) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width) return;
    const float nan = __int_as_float(0x7fc00000);
    for (int y = blockIdx.y; y < height; y += gridDim.y) {
        const float s = src[(long long)y * src_stride + x];
        const long long pi = (long long)y * par_stride + x;
        // param_us_ra.mask = mask_us (bool of the nearest-resampled mask, :498) or src_ra.mask (:500)
        const bool on = keep ? keep[pi] != 0.f : rs_valid(s, nd_mode, nodata);
        const float g = on ? gain[pi] : nan, o = on ? offset[pi] : nan;
        out[(long long)y * out_stride + x] = __fadd_rn(__fmul_rn(g, s), o);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// RefSpaceModel.apply fused (kernel_model.py:484-503): the up-sampled gain / offset never exist as full-resolution
// planes.  Per destination pixel the bilinear / cubic-spline values of BOTH parameter planes are formed exactly as
// resample_kernel<MODE> forms them (same weights, same tap order, same renormalisation rule), masked like apply_space_kernel and
// applied.  The work that does not depend on the pixel is hoisted: the row geometry and weights come from a table made
// by row_table_kernel (one entry per destination row, from rs_axis_taps), the column geometry and weights are computed once per
// thread, which then walks down its column.
// upsample_apply_kernel does NOT call hk_resample_taps.h: it is the one re-sampler on a measured hot path, and sharing rs_tap_sum
// with its general path cost it a wave per SIMD (cubic_spline 82 -> 118 VGPRs, bilinear 46 -> 58) for no change in results.  Its
// column set-up mirrors rs_centre and rs_axis_taps, its two tap sums mirror rs_tap_sum: a change of the rule there is made here too.
constexpr int UP_ROWS = 16;  // destination rows per thread of upsample_apply_kernel (amortises the column weights)
struct RowTab {
    double w[4];
    int iy;       // first tap row - T0
    int centre;   // source row under the destination centre, or -1 when outside
    int yy[4];    // tap rows clamped into the plane (always loadable)
    int all_in;   // every tap row lies inside the plane
};

template <int MODE>
__global__ void __launch_bounds__(256) row_table_kernel(RowTab* __restrict__ tab, int dh, int sh, double ky, double oy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dh) return;
    const double sy = scaled_coord(ky, oy, (double)i + 0.5);
    long long cy;
    RowTab t;
    t.centre = rs_centre_axis(sy, sh, cy) ? (int)cy : -1;
    t.iy = rs_axis_taps<MODE>(sy, t.w);
    t.all_in = 1;
    for (int tj = 0; tj < 4; ++tj) {
        const int yy = t.iy + RS_T0<MODE> + (tj < RS_NT<MODE> ? tj : RS_NT<MODE> - 1);
        if (yy < 0 || yy >= sh) t.all_in = 0;
        t.yy[tj] = min(max(yy, 0), sh - 1);
    }
    tab[i] = t;
}

struct UpApplyArgs {
    const float* src;     // full-resolution source (destination grid)
    long long src_stride;
    int nd_mode;
    float nodata;
    const float* gain;    // coarse parameter planes, NaN = nodata
    const float* offset;
    long long par_stride;
    int ph, pw;
    const float* keep;    // nullable full-resolution 0/1 plane (mask_partial)
    long long keep_stride;
    float* out;
    long long out_stride;
    int height, width;
    double kx, ox;
    const RowTab* rows;
};

template <int MODE>
__global__ void __launch_bounds__(256) upsample_apply_kernel(const UpApplyArgs a) {
    constexpr int NT = MODE == 1 ? 2 : 4, T0 = MODE == 1 ? 0 : -1;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.width) return;
    const float nan = __int_as_float(0x7fc00000);
    // column geometry and weights: once per thread
    const double sx = a.kx * ((double)j + 0.5) + a.ox;
    const long long cx = (long long)floor(sx + 1e-10);
    const bool cx_ok = cx >= 0 && cx < a.pw;
    const int ix = (int)floor(sx - 0.5);
    const double dx = sx - 0.5 - (double)ix;
    double wxs[4];
    if constexpr (MODE == 1) {
        wxs[0] = 1.0 - dx, wxs[1] = dx, wxs[2] = wxs[3] = 0.0;
    } else {
        bspline4(dx, wxs);
    }
    // first tap column, clamped so that NT consecutive columns are always loadable (straight-line path below)
    const bool col_all_in = ix + T0 >= 0 && ix + T0 + NT <= a.pw;
    const int xbase = min(max(ix + T0, 0), max(a.pw - NT, 0));
    // consecutive destination rows per block: neighbouring rows read the same parameter rows (L1 / L2 reuse)
    const int i_end = min(a.height, ((int)blockIdx.y + 1) * UP_ROWS);
    for (int i = blockIdx.y * UP_ROWS; i < i_end; ++i) {
        const RowTab t = a.rows[i];  // wave-uniform
        const float s = a.src[(long long)i * a.src_stride + j];
        const bool on = a.keep ? a.keep[(long long)i * a.keep_stride + j] != 0.f : rs_valid(s, a.nd_mode, a.nodata);
        float par[2] = {nan, nan};
        const bool need = on && cx_ok && t.centre >= 0;
        // Straight-line path (the interior of the raster): every tap of every lane that needs a value is inside the plane
        // and not NaN -> all 2 x NT x NT loads go out together, no per-tap control flow, and the sums run over the same
        // taps in the same order as below (the weight sum does not depend on the plane).  Otherwise: the general path.
        float tg[NT][NT], to[NT][NT];
        float chk = 0.f;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            // the NT taps of a row are consecutive columns when they are all inside (the only case that uses them):
            // one (possibly unaligned) NT-float load per row and plane from a base clamped into the plane
            const int off = t.yy[tj] * (int)a.par_stride + xbase;
            if constexpr (NT == 4) {
                const float4 vg = *reinterpret_cast<const float4*>(a.gain + off);
                const float4 vo = *reinterpret_cast<const float4*>(a.offset + off);
                tg[tj][0] = vg.x, tg[tj][1] = vg.y, tg[tj][2] = vg.z, tg[tj][3] = vg.w;
                to[tj][0] = vo.x, to[tj][1] = vo.y, to[tj][2] = vo.z, to[tj][3] = vo.w;
            } else {
                const float2 vg = *reinterpret_cast<const float2*>(a.gain + off);
                const float2 vo = *reinterpret_cast<const float2*>(a.offset + off);
                tg[tj][0] = vg.x, tg[tj][1] = vg.y, to[tj][0] = vo.x, to[tj][1] = vo.y;
            }
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) chk += tg[tj][ti] + to[tj][ti];  // NaN anywhere (or inf - inf) makes chk NaN
        }
        const bool straight = !need || (t.all_in && col_all_in && chk == chk);
        if (__all((int)straight)) {
            double wgt[NT][NT], wacc = 0.0, accg = 0.0, acco = 0.0;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    wgt[tj][ti] = wxs[ti] * t.w[tj];
                    accg += (double)tg[tj][ti] * wgt[tj][ti];
                    acco += (double)to[tj][ti] * wgt[tj][ti];
                    wacc += wgt[tj][ti];
                }
            }
            const bool renorm = wacc < 0.99999 || wacc > 1.00001;
            if (__any((int)(need && renorm))) {  // wave-uniform: interior weights sum to 1 within the tolerance
                accg = renorm ? accg / wacc : accg;
                acco = renorm ? acco / wacc : acco;
            }
            if (need && !(wacc < 1e-6)) par[0] = (float)accg, par[1] = (float)acco;
        } else if (need) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float* __restrict__ pp = b ? a.offset : a.gain;
                if (pp[(long long)t.centre * a.par_stride + cx] != pp[(long long)t.centre * a.par_stride + cx]) continue;  // NaN centre
                double acc = 0.0, wacc = 0.0;
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) {
                    const int yy = t.iy + T0 + tj;
                    if (yy < 0 || yy >= a.ph) continue;
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) {
                        const int xx = ix + T0 + ti;
                        if (xx < 0 || xx >= a.pw) continue;
                        const float v = pp[(long long)yy * a.par_stride + xx];
                        if (v != v) continue;
                        const double wgt = wxs[ti] * t.w[tj];
                        acc += (double)v * wgt;
                        wacc += wgt;
                    }
                }
                if (!(wacc < 1e-6)) par[b] = (float)((wacc < 0.99999 || wacc > 1.00001) ? acc / wacc : acc);
            }
        }
        a.out[(long long)i * a.out_stride + j] = __fadd_rn(__fmul_rn(par[0], s), par[1]);
    }
}

size_t upsample_apply_workspace_bytes(int height) { return (size_t)height * sizeof(RowTab); }

// mode: 1 bilinear, 3 cubic_spline (anything else: hipErrorInvalidValue -- the caller keeps the unfused path)
hipError_t launch_upsample_apply(int mode, const UpsampleApply& r, void* workspace, hipStream_t stream) {
    if (mode != 1 && mode != 3) return hipErrorInvalidValue;
    if ((long long)r.ph * r.par_stride >= 0x7fffffffLL) return hipErrorInvalidValue;  // 32-bit tap offsets
    if (r.pw < 4) return hipErrorInvalidValue;                                         // row loads of 4 consecutive taps
    RowTab* tab = static_cast<RowTab*>(workspace);
    const UpApplyArgs a = {r.src, r.src_stride, r.nd_mode, r.nodata, r.gain, r.offset, r.par_stride, r.ph, r.pw, r.keep, r.keep_stride,
                           r.out, r.out_stride, r.height, r.width, r.kx, r.ox, tab};
    const dim3 tgrid((r.height + 255) / 256), grid((r.width + 255) / 256, (r.height + UP_ROWS - 1) / UP_ROWS), block(256);
    if (mode == 1) {
        HK_LAUNCH(row_table_kernel<1>, tgrid, block, 0, stream, tab, r.height, r.ph, r.ky, r.oy);
        HK_LAUNCH(upsample_apply_kernel<1>, grid, block, 0, stream, a);
    } else {
        HK_LAUNCH(row_table_kernel<3>, tgrid, block, 0, stream, tab, r.height, r.ph, r.ky, r.oy);
        HK_LAUNCH(upsample_apply_kernel<3>, grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_valid_plane(const ValidPlane& r, hipStream_t stream) {
    HK_LAUNCH(valid_plane_kernel, dim3((r.width + 255) / 256, r.height < 1024 ? r.height : 1024), dim3(256), 0, stream,
                       r.in, r.in_stride, r.nd_mode, r.nodata, r.out, r.out_stride, r.height, r.width);
    return hipGetLastError();
}

hipError_t launch_apply_space(const ApplySpace& r, hipStream_t stream) {
    HK_LAUNCH(apply_space_kernel, dim3((r.width + 255) / 256, r.height < 1024 ? r.height : 1024), dim3(256), 0, stream,
                       r.src, r.src_stride, r.nd_mode, r.nodata, r.gain, r.offset, r.par_stride, r.keep, r.out, r.out_stride, r.height,
                       r.width);
    return hipGetLastError();
}

hipError_t launch_resample(int mode, const ResamplePlanes& p, double kx, double ox, double ky, double oy, hipStream_t stream) {
    const ResampleArgs a = {p, kx, ox, ky, oy};
    const dim3 grid((p.dw + 255) / 256, p.dh, p.n_bands), block(256);
    const bool stretched = resample_stretched(kx, ky);
    switch (mode) {
        case 0: HK_LAUNCH(resample_kernel<0>, grid, block, 0, stream, a); break;
        case 1:
            if (stretched) HK_LAUNCH(resample_conv_kernel<1>, grid, block, 0, stream, a);
            else HK_LAUNCH(resample_kernel<1>, grid, block, 0, stream, a);
            break;
        case 2: HK_LAUNCH(resample_conv_kernel<2>, grid, block, 0, stream, a); break;
        case 3:
            if (stretched) HK_LAUNCH(resample_conv_kernel<3>, grid, block, 0, stream, a);
            else HK_LAUNCH(resample_kernel<3>, grid, block, 0, stream, a);
            break;
        case 4: HK_LAUNCH(resample_conv_kernel<4>, grid, block, 0, stream, a); break;
        case 5: HK_LAUNCH(resample_kernel<5>, grid, block, 0, stream, a); break;
        case 6: HK_LAUNCH(resample_kernel<6>, grid, block, 0, stream, a); break;
        case 8: HK_LAUNCH(resample_kernel<8>, grid, block, 0, stream, a); break;
        case 9: HK_LAUNCH(resample_kernel<9>, grid, block, 0, stream, a); break;
        case 10: HK_LAUNCH(resample_kernel<10>, grid, block, 0, stream, a); break;
        case 11: HK_LAUNCH(resample_kernel<11>, grid, block, 0, stream, a); break;
        case 12: HK_LAUNCH(resample_kernel<12>, grid, block, 0, stream, a); break;
        case 13: HK_LAUNCH(resample_kernel<13>, grid, block, 0, stream, a); break;
        case 14: HK_LAUNCH(resample_kernel<14>, grid, block, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the request with its plane typed: what footprint_typed_kernel<T> receives
template <typename T>
static FootTypedArgs<T> foot_typed_args(const FootTypedArgs<void>& r) {
    return {static_cast<const T*>(r.src), r.src_stride, r.sh, r.sw, r.nd_mode, r.nodata, r.value, r.coverage, r.dst_stride, r.dh, r.dw,
            r.fill, r.kx, r.ox, r.ky, r.oy};
}

hipError_t launch_footprint_typed(int dtype, const FootTypedArgs<void>& r, hipStream_t stream) {
    const dim3 grid((r.dw + 255) / 256, r.dh), block(256);
#define HK_FOOT_TYPED(T) HK_LAUNCH(footprint_typed_kernel<T>, grid, block, 0, stream, foot_typed_args<T>(r))
    switch (dtype) {
        case 0: HK_FOOT_TYPED(float); break;
        case 1: HK_FOOT_TYPED(unsigned char); break;
        case 2: HK_FOOT_TYPED(unsigned short); break;
        case 3: HK_FOOT_TYPED(short); break;
        case 4: HK_FOOT_TYPED(unsigned int); break;
        case 5: HK_FOOT_TYPED(int); break;
        case 6: HK_FOOT_TYPED(double); break;
        default: return hipErrorInvalidValue;
    }
#undef HK_FOOT_TYPED
    return hipGetLastError();
}

}  // namespace hk
