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

}  // namespace hk
