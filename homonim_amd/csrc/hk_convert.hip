// hk_convert.hip -- data-format edges of the hot path on gfx950: integer / float64 rasters in, typed rasters out.
//
// Reference behaviour:
//   * input : RasterArray.from_rio_dataset reads every band with out_dtype float32 (homonim/raster_array.py:178-188):
//             a plain value conversion (exact for 8/16-bit integers, round-to-nearest for 32-bit integers / float64).
//   * output: RasterArray._convert_array_dtype (homonim/raster_array.py:353-387): promote to a float type that holds
//             the destination range (float32 for <= 16-bit integers, float64 for 32-bit ones), np.round (half to
//             even), np.clip to the destination range, cast; pixels that are nodata in the corrected block (NaN)
//             receive the output nodata value.
// Both are HBM-bound element-wise kernels; they exist so that host<->device traffic is 1-2 B per pixel instead of 4.
#include "hk_kernels.h"

namespace hk {

template <typename T>
__global__ void __launch_bounds__(256) cast_in_kernel(const T* __restrict__ in, long long in_stride, float* __restrict__ out,
                                                      long long out_stride, int height, int width) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * PX;
    if (x >= width) return;
    for (int y = blockIdx.y; y < height; y += gridDim.y) {
        const T* ip = in + (long long)y * in_stride + x;
        float v[PX];
#pragma unroll
        for (int i = 0; i < PX; ++i) v[i] = (float)ip[i];  // rows are padded to a multiple of PX elements
        *reinterpret_cast<float4*>(out + (long long)y * out_stride + x) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

template <typename T>
struct OutTraits;
template <> struct OutTraits<unsigned char>  { static constexpr double lo = 0., hi = 255.; static constexpr bool wide = false, is_float = false; };
template <> struct OutTraits<unsigned short> { static constexpr double lo = 0., hi = 65535.; static constexpr bool wide = false, is_float = false; };
template <> struct OutTraits<short>          { static constexpr double lo = -32768., hi = 32767.; static constexpr bool wide = false, is_float = false; };
template <> struct OutTraits<unsigned int>   { static constexpr double lo = 0., hi = 4294967295.; static constexpr bool wide = true, is_float = false; };
template <> struct OutTraits<int>            { static constexpr double lo = -2147483648., hi = 2147483647.; static constexpr bool wide = true, is_float = false; };
template <> struct OutTraits<float>          { static constexpr double lo = 0., hi = 0.; static constexpr bool wide = false, is_float = true; };
template <> struct OutTraits<double>         { static constexpr double lo = 0., hi = 0.; static constexpr bool wide = true, is_float = true; };

// one sample of the corrected plane as the output holds it: a masked pixel (NaN) -> the output nodata (without one: 0, or the NaN
// itself in a float type), everything else rounded half to even and clipped to the type's range
template <typename T>
__device__ __forceinline__ T cast_out_sample(float f, int has_nodata, T nd) {
    using TR = OutTraits<T>;
    if (f != f) {
        return has_nodata ? nd : (TR::is_float ? (T)f : (T)0);  // masked pixel -> output nodata
    } else if constexpr (TR::is_float) {
        return (T)f;
    } else if constexpr (TR::wide) {
        double v = rint((double)f);
        v = fmin(fmax(v, TR::lo), TR::hi);
        return (T)v;
    } else {
        float v = rintf(f);  // np.round: half to even
        v = fminf(fmaxf(v, (float)TR::lo), (float)TR::hi);
        return (T)v;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) cast_out_kernel(const float* __restrict__ in, long long in_stride, T* __restrict__ out,
                                                       long long out_stride, int height, int width, int has_nodata,
                                                       double nodata) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * PX;
    if (x >= width) return;
    const T nd = has_nodata ? (T)nodata : (T)0;
    for (int y = blockIdx.y; y < height; y += gridDim.y) {
        const float4 f4 = *reinterpret_cast<const float4*>(in + (long long)y * in_stride + x);
        const float f[PX] = {f4.x, f4.y, f4.z, f4.w};
        T* op = out + (long long)y * out_stride + x;
#pragma unroll
        for (int i = 0; i < PX; ++i) op[i] = cast_out_sample<T>(f[i], has_nodata, nd);
    }
}

// cast_out_kernel + the validity of every pixel from the same read: `valid` = 255 where the corrected value is not NaN, else 0 --
// the mask of the reference's corrected RasterArray, taken BEFORE the conversion (an integer output cannot tell a masked pixel
// from a 0).  The PX validity bytes of a lane are one 4-byte store (rows of `valid` are padded to PX like the others).
template <typename T>
__global__ void __launch_bounds__(256) cast_out_valid_kernel(const float* __restrict__ in, long long in_stride, T* __restrict__ out,
                                                             long long out_stride, unsigned char* __restrict__ valid,
                                                             long long valid_stride, int height, int width, int has_nodata,
                                                             double nodata) {
    static_assert(PX == 4, "the validity of a lane's pixels is one 4-byte word");
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * PX;
    if (x >= width) return;
    const T nd = has_nodata ? (T)nodata : (T)0;
    for (int y = blockIdx.y; y < height; y += gridDim.y) {
        const float4 f4 = *reinterpret_cast<const float4*>(in + (long long)y * in_stride + x);
        const float f[PX] = {f4.x, f4.y, f4.z, f4.w};
        T* op = out + (long long)y * out_stride + x;
        unsigned ok = 0;
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            op[i] = cast_out_sample<T>(f[i], has_nodata, nd);
            ok |= (f[i] == f[i] ? 255u : 0u) << (8 * i);
        }
        *reinterpret_cast<unsigned*>(valid + (long long)y * valid_stride + x) = ok;
    }
}

static dim3 cast_grid(int height, int width) {
    return dim3((width + 256 * PX - 1) / (256 * PX), height < 2048 ? height : 2048);
}

hipError_t launch_cast_in(int dtype, const CastPlane& r, hipStream_t stream) {
    const dim3 g = cast_grid(r.height, r.width), b(256);
#define HK_CAST_IN(T) \
    HK_LAUNCH(cast_in_kernel<T>, g, b, 0, stream, static_cast<const T*>(r.in), r.in_stride, static_cast<float*>(r.out), r.out_stride, r.height, r.width)
    switch (dtype) {
        case 1: HK_CAST_IN(unsigned char); break;
        case 2: HK_CAST_IN(unsigned short); break;
        case 3: HK_CAST_IN(short); break;
        case 4: HK_CAST_IN(unsigned int); break;
        case 5: HK_CAST_IN(int); break;
        case 6: HK_CAST_IN(double); break;
        default: return hipErrorInvalidValue;
    }
#undef HK_CAST_IN
    return hipGetLastError();
}

hipError_t launch_cast_out(int dtype, const CastPlane& r, hipStream_t stream) {
    const dim3 g = cast_grid(r.height, r.width), b(256);
#define HK_CAST_OUT(T)                                                                                                                      \
    HK_LAUNCH(cast_out_kernel<T>, g, b, 0, stream, static_cast<const float*>(r.in), r.in_stride, static_cast<T*>(r.out), r.out_stride, r.height, \
              r.width, r.has_nodata, r.nodata)
    switch (dtype) {
        case 0: HK_CAST_OUT(float); break;
        case 1: HK_CAST_OUT(unsigned char); break;
        case 2: HK_CAST_OUT(unsigned short); break;
        case 3: HK_CAST_OUT(short); break;
        case 4: HK_CAST_OUT(unsigned int); break;
        case 5: HK_CAST_OUT(int); break;
        case 6: HK_CAST_OUT(double); break;
        default: return hipErrorInvalidValue;
    }
#undef HK_CAST_OUT
    return hipGetLastError();
}

hipError_t launch_cast_out_valid(int dtype, const CastPlane& r, hipStream_t stream) {
    const dim3 g = cast_grid(r.height, r.width), b(256);
    if (!r.valid || r.valid_stride % PX || (uintptr_t)r.valid % PX) return hipErrorInvalidValue;
#define HK_CAST_OUT_VALID(T)                                                                                                                 \
    HK_LAUNCH(cast_out_valid_kernel<T>, g, b, 0, stream, static_cast<const float*>(r.in), r.in_stride, static_cast<T*>(r.out), r.out_stride, \
              r.valid, r.valid_stride, r.height, r.width, r.has_nodata, r.nodata)
    switch (dtype) {
        case 0: HK_CAST_OUT_VALID(float); break;
        case 1: HK_CAST_OUT_VALID(unsigned char); break;
        case 2: HK_CAST_OUT_VALID(unsigned short); break;
        case 3: HK_CAST_OUT_VALID(short); break;
        case 4: HK_CAST_OUT_VALID(unsigned int); break;
        case 5: HK_CAST_OUT_VALID(int); break;
        case 6: HK_CAST_OUT_VALID(double); break;
        default: return hipErrorInvalidValue;
    }
#undef HK_CAST_OUT_VALID
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Resident rasters of RasterFuse.process (device_config resident=True): the typed prefill of an output raster and the boundless
// window of an input raster.  Both are element-wise and HBM-bound; a lane owns one 16-byte unit of a row -- VEC = 16 / sizeof(T)
// samples, cut where the row's ADDRESSES are multiples of 16, not where its columns are -- so whole units move as one 16-byte
// access whatever the row's offset and the ragged ends go sample by sample behind their bounds.  All index arithmetic is 64-bit;
// nothing outside [row, row + width) of any plane is touched.

// N consecutive samples to `p`: 16-byte stores where `p` and N allow them, else one by one
template <typename U, int N>
__device__ __forceinline__ void store_run(U* __restrict__ p, const U (&v)[N]) {
    if constexpr ((N * sizeof(U)) % 16 == 0) {
        if (((uintptr_t)p & 15u) == 0) {
            union { uint4 q[N * sizeof(U) / 16]; U e[N]; } u;
#pragma unroll
            for (int i = 0; i < N; ++i) u.e[i] = v[i];
#pragma unroll
            for (int i = 0; i < (int)(N * sizeof(U) / 16); ++i) reinterpret_cast<uint4*>(p)[i] = u.q[i];
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = v[i];
}

// samples of a row before its first 16-byte boundary, counted back from it: unit k of the row holds the columns
// [k * VEC - lead, (k + 1) * VEC - lead)
template <typename T>
__device__ __forceinline__ long long row_lead(const T* row) {
    constexpr int VEC = 16 / sizeof(T);
    return (long long)(((uintptr_t)row / sizeof(T)) % VEC);
}

template <typename T>
__global__ void __launch_bounds__(256) fill_planes_kernel(FillPlanes<T> a) {
    constexpr int VEC = 16 / sizeof(T);
    const long long unit = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    T v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = a.value;
    for (long long b = blockIdx.z; b < a.n_bands; b += gridDim.z) {
        for (long long y = blockIdx.y; y < a.height; y += gridDim.y) {
            T* __restrict__ const row = a.out + b * a.band_stride + y * a.stride;
            const long long x0 = unit * VEC - row_lead(row);
            if (x0 >= a.width) continue;
            if (x0 >= 0 && x0 + VEC <= a.width) {
                store_run<T, VEC>(row + x0, v);
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (x0 + i >= 0 && x0 + i < a.width) row[x0 + i] = a.value;
            }
        }
    }
}

// RasterFuse._read_boundless of every band in one launch.  `to_float`: the raster has no nodata value, or NaN -- the window is
// float32 (out_f), the plain value conversion of every sample inside the raster and NaN outside; else it is of the raster's own
// type (out_t) with `fill` outside.
template <typename T>
__global__ void __launch_bounds__(256) boundless_window_kernel(BoundlessWindow<T> a) {
    constexpr int VEC = 16 / sizeof(T);
    const long long unit = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool to_float = a.out_f != nullptr;
    const float nan32 = __uint_as_float(0x7FC00000u);
    for (long long b = blockIdx.z; b < a.n_bands; b += gridDim.z) {
        for (long long y = blockIdx.y; y < a.out_height; y += gridDim.y) {
            const long long ry = y + a.row_off;
            const bool row_in = ry >= 0 && ry < a.height;
            // the raster's row, or -- outside it -- row 0 for the cut of the units only: nothing of it is read
            const T* __restrict__ const in_row = a.in + b * a.in_band_stride + (row_in ? ry : 0) * a.in_stride;
            const long long lead = row_lead(in_row);
            // the first unit that holds a column of the window (floor division: col_off may be negative)
            const long long c = (long long)a.col_off + lead;
            const long long k0 = c >= 0 ? c / VEC : -((-c + VEC - 1) / VEC);
            const long long cx0 = (k0 + unit) * VEC - lead;   // raster column of this lane's first sample
            const long long x0 = cx0 - a.col_off;             // ... and its column in the window
            if (x0 >= a.out_width) continue;
            T v[VEC];
            if (row_in && cx0 >= 0 && cx0 + VEC <= a.width) {
                union { uint4 q; T e[VEC]; } u;
                u.q = *reinterpret_cast<const uint4*>(in_row + cx0);
#pragma unroll
                for (int i = 0; i < VEC; ++i) v[i] = u.e[i];
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) v[i] = (row_in && cx0 + i >= 0 && cx0 + i < a.width) ? in_row[cx0 + i] : a.fill;
            }
            const bool whole = x0 >= 0 && x0 + VEC <= a.out_width;
            if (to_float) {
                float f[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) f[i] = (row_in && cx0 + i >= 0 && cx0 + i < a.width) ? (float)v[i] : nan32;
                float* __restrict__ const out_row = a.out_f + b * a.out_band_stride + y * a.out_stride;
                if (whole) {
                    store_run<float, VEC>(out_row + x0, f);
                } else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        if (x0 + i >= 0 && x0 + i < a.out_width) out_row[x0 + i] = f[i];
                }
            } else {
                T* __restrict__ const out_row = a.out_t + b * a.out_band_stride + y * a.out_stride;
                if (whole) {
                    store_run<T, VEC>(out_row + x0, v);
                } else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        if (x0 + i >= 0 && x0 + i < a.out_width) out_row[x0 + i] = v[i];
                }
            }
        }
    }
}

// units of 16 bytes that can hold a sample of a row of `width` samples of `es` bytes, wherever the row starts
static dim3 unit_grid(long long width, int es, int height, int n_bands) {
    const long long units = width / (16 / es) + 2;
    return dim3((unsigned)((units + 255) / 256), height < 2048 ? height : 2048, n_bands < 64 ? n_bands : 64);
}

hipError_t launch_fill_planes(int dtype, const PlaneFill& r, hipStream_t stream) {
    const dim3 g = unit_grid(r.width, dtype_size(dtype) ? dtype_size(dtype) : 1, r.height, r.n_bands), b(256);
#define HK_FILL_PLANES(T) \
    HK_LAUNCH(fill_planes_kernel<T>, g, b, 0, stream, FillPlanes<T>{static_cast<T*>(r.out), r.stride, r.band_stride, r.n_bands, r.height, r.width, (T)r.value})
    switch (dtype) {
        case 0: HK_FILL_PLANES(float); break;
        case 1: HK_FILL_PLANES(unsigned char); break;
        case 2: HK_FILL_PLANES(unsigned short); break;
        case 3: HK_FILL_PLANES(short); break;
        case 4: HK_FILL_PLANES(unsigned int); break;
        case 5: HK_FILL_PLANES(int); break;
        case 6: HK_FILL_PLANES(double); break;
        default: return hipErrorInvalidValue;
    }
#undef HK_FILL_PLANES
    return hipGetLastError();
}

template <typename T>
static BoundlessWindow<T> boundless_args(const WindowGather& r) {
    BoundlessWindow<T> a;
    a.in = static_cast<const T*>(r.in);
    a.out_t = r.to_float ? nullptr : static_cast<T*>(r.out);
    a.out_f = r.to_float ? static_cast<float*>(r.out) : nullptr;
    a.in_stride = r.in_stride, a.in_band_stride = r.in_band_stride, a.out_stride = r.out_stride, a.out_band_stride = r.out_band_stride;
    a.n_bands = r.n_bands, a.height = r.height, a.width = r.width;
    a.row_off = r.row_off, a.col_off = r.col_off, a.out_height = r.out_height, a.out_width = r.out_width;
    a.fill = r.to_float ? (T)0 : (T)r.fill;
    return a;
}

hipError_t launch_boundless_window(int dtype, const WindowGather& r, hipStream_t stream) {
    const dim3 g = unit_grid(r.out_width, dtype_size(dtype) ? dtype_size(dtype) : 1, r.out_height, r.n_bands), b(256);
#define HK_BOUNDLESS(T) HK_LAUNCH(boundless_window_kernel<T>, g, b, 0, stream, boundless_args<T>(r))
    switch (dtype) {
        case 0: HK_BOUNDLESS(float); break;
        case 1: HK_BOUNDLESS(unsigned char); break;
        case 2: HK_BOUNDLESS(unsigned short); break;
        case 3: HK_BOUNDLESS(short); break;
        case 4: HK_BOUNDLESS(unsigned int); break;
        case 5: HK_BOUNDLESS(int); break;
        case 6: HK_BOUNDLESS(double); break;
        default: return hipErrorInvalidValue;
    }
#undef HK_BOUNDLESS
    return hipGetLastError();
}

}  // namespace hk
