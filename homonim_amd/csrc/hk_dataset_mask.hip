// hk_dataset_mask.hip -- the per-dataset mask of a GeoTIFF (an internal 1-bit mask or an alpha band) applied to its bands on gfx950.
//
// Reference behaviour: RasterArray.from_rio_dataset (homonim/raster_array.py:161-197) reads a dataset whose bands carry a
// per-dataset mask as float32 with NaN wherever dataset_mask() is false, every band alike; valid pixels get the plain value
// conversion of cast_in_kernel (hk_convert.hip).
//
// HBM-bound and element-wise: per pixel, n_bands samples in and n_bands float32 out, plus one bit (BITS) or one sample (ALPHA) of
// validity.  A lane owns GROUPS of 8 consecutive pixels -- one byte of a packed mask row (hk_maskbits_core.h) -- reads the group's
// validity ONCE and loops the bands inside, so the mask costs 1/8 byte (BITS) or one sample (ALPHA) per pixel whatever the band
// count.  Whole groups of aligned rows move as 8- or 16-byte loads and 16-byte stores; the tail group of a row, and every group of
// a row that starts at another address, goes pixel by pixel behind `x < width`.  No LDS.  Nothing outside [row, row + width) of any
// plane and outside ceil(width / 8) bytes of a mask row is touched.
#include <type_traits>

#include "hk_kernels.h"
#include "hk_maskbits_core.h"

namespace hk {

constexpr int BITS = maskbits::KIND_BITS, ALPHA = maskbits::KIND_ALPHA;

template <typename T, int KIND>
__global__ void __launch_bounds__(256) dataset_mask_kernel(DatasetMask a) {
    using namespace maskbits;
    using A = std::conditional_t<KIND == ALPHA, T, unsigned char>;   // what a validity row holds
    const long long width = a.planes.width;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = g < groups_of(width);   // (no early return: the whole-wave path below needs every lane of its wave)
    const bool whole = g * GROUP + GROUP <= width;
    const bool upper = (threadIdx.x & 32u) != 0;   // the lanes 32..63 of the wave
    const HKM_G T* const planes = (const HKM_G T*)a.planes.src;
    const HKM_G A* const mask = (const HKM_G A*)a.mask;
    HKM_G float* const out = (HKM_G float*)a.out;
    for (int y = blockIdx.y; y < a.planes.height; y += gridDim.y) {
        const HKM_G A* const vrow = mask + (long long)y * a.mask_stride;
        unsigned valid = 0;
        if (active) {
            if constexpr (KIND == BITS) valid = bits_group(vrow, g);
            else valid = alpha_group<A>(vrow, g, width, whole && row_wide<A>(vrow));
        }
        for (int b = 0; b < a.planes.n_bands; ++b) {
            const HKM_G T* const in_row = planes + (long long)b * a.planes.band_stride + (long long)y * a.planes.stride;
            HKM_G float* const out_row = out + (long long)b * a.out_band_stride + (long long)y * a.out_stride;
            const bool wide = active && whole && row_wide<T>(in_row) && out_row_wide(out_row);
            if (__builtin_amdgcn_ballot_w64(wide) == ~0ull) {
                // All 64 groups of the wave are whole and wide: 512 consecutive pixels.  Stored group by group, each of the two
                // store instructions would write 16 bytes in every 32; so the halves of the wave exchange first (lanes 32..63 hand
                // their first quad down and get the lower lanes' second quad), and each instruction writes 1 KiB without a gap:
                // the first the pixels of the groups of lanes 0..31, the second those of lanes 32..63.  The same bytes at the
                // same addresses, all inside the wave's own 512 pixels.
                float f[GROUP];
                wide_values<T>(in_row, g, valid, f);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(f[i]), __float_as_uint(f[4 + i]), false, false);
                    f[i] = __uint_as_float(r[0]), f[4 + i] = __uint_as_float(r[1]);
                }
                // lower lane i: [own first quad | first quad of lane i + 32]; upper lane i + 32: [second quad of lane i | own second]
                HKM_G float* const p = out_row + g * GROUP;
                store_quad(upper ? p - 32 * GROUP + 4 : p, f[0], f[1], f[2], f[3]);
                store_quad(upper ? p + 4 : p + 32 * GROUP, f[4], f[5], f[6], f[7]);
            } else if (active) {
                put_group<T>(in_row, out_row, g, width, valid, wide);
            }
        }
    }
}

hipError_t launch_dataset_mask(int dtype, const DatasetMask& a, hipStream_t stream) {
    const long long groups = maskbits::groups_of(a.planes.width);
    const dim3 g((unsigned)((groups + 255) / 256), a.planes.height < 2048 ? a.planes.height : 2048), b(256);
#define HK_DATASET_MASK(T, KIND) HK_LAUNCH((dataset_mask_kernel<T, KIND>), g, b, 0, stream, a)
    if (a.kind == ALPHA) {
        switch (dtype) {
            case 1: HK_DATASET_MASK(unsigned char, ALPHA); break;
            case 2: HK_DATASET_MASK(unsigned short, ALPHA); break;
            default: return hipErrorInvalidValue;
        }
    } else if (a.kind == BITS) {
        switch (dtype) {
            case 0: HK_DATASET_MASK(float, BITS); break;
            case 1: HK_DATASET_MASK(unsigned char, BITS); break;
            case 2: HK_DATASET_MASK(unsigned short, BITS); break;
            case 3: HK_DATASET_MASK(short, BITS); break;
            case 4: HK_DATASET_MASK(unsigned int, BITS); break;
            case 5: HK_DATASET_MASK(int, BITS); break;
            case 6: HK_DATASET_MASK(double, BITS); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        return hipErrorInvalidValue;
    }
#undef HK_DATASET_MASK
    return hipGetLastError();
}

}  // namespace hk
