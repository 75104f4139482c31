// hk_maskbits_core.h -- the group arithmetic of hk_dataset_mask.hip: a row of a raster is worked in GROUPS of 8 consecutive pixels
// starting at a multiple of 8, which is what one byte of a packed 1-bit mask row covers (TIFF FillOrder 1: the most significant bit
// is the first pixel).  A host program compiles the same functions as plain C++ (HKM_HOST: no HIP; tests/c/maskbits_core_host.cpp),
// which is how the bounds below are held without a GPU.
//
// WHAT A GROUP TOUCHES.  Group g of a row of `width` pixels covers the pixels [8g, min(8g + 8, width)).  Nothing outside them is
// read from a plane row or an alpha row or written to an output row, and of a mask row only byte g, g < ceil(width / 8): the pad
// bits of the last byte are read with it and never looked at.
//
// WIDE AND NARROW.  A group that is WHOLE (8g + 8 <= width) in a row whose address allows it is moved with wide accesses: the 8
// samples of a plane or alpha row as one 8-byte load (1-byte samples) or as 16-byte loads, the 8 results as two 16-byte stores.
// `row_wide<T>()` says whether a row's address allows it: the row starts at a multiple of min(16, 8 * sizeof(T)) bytes -- every
// group then does, its offset being a multiple of 8 samples -- and the output row at a multiple of 16.  Every other group (the
// tail of a row; all groups of a row that starts elsewhere) goes pixel by pixel, each access behind its own `x < width`.
//
// THE VALUE.  A valid pixel gets `(float)sample`, the plain conversion cast_in_kernel states (hk_convert.hip); every other one the
// quiet NaN 0x7FC00000.  A valid float32 sample keeps its bits, NaN payloads included.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef HKM_HOST
#include <stdlib.h>
#define HKM_FN inline
#define HKM_G
#define HKM_UNROLL
#else
#include <hip/hip_runtime.h>
#define HKM_FN __device__ __forceinline__
#define HKM_G __attribute__((address_space(1)))
#define HKM_UNROLL _Pragma("unroll")
#endif

namespace hk {
namespace maskbits {

constexpr int GROUP = 8;                   // pixels per group: one byte of a packed mask row
constexpr int KIND_BITS = 0, KIND_ALPHA = 1;   // (HK_MASK_BITS, HK_MASK_ALPHA of include/homonim_hk.h)
constexpr unsigned NAN_BITS = 0x7FC00000u;

// groups of a row = bytes of a packed mask row (constexpr: the launcher on the host sizes its grid with it)
constexpr long long groups_of(long long width) { return (width + GROUP - 1) / GROUP; }

template <typename T>
constexpr unsigned wide_align() { return 8 * sizeof(T) < 16 ? 8 * (unsigned)sizeof(T) : 16u; }

HKM_FN bool aligned_to(const HKM_G void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// may the whole groups of this (plane or alpha) row be loaded wide?
template <typename T>
HKM_FN bool row_wide(const HKM_G T* row) { return aligned_to(row, wide_align<T>()); }
// ... and those of this output row stored wide?
HKM_FN bool out_row_wide(const HKM_G float* row) { return aligned_to(row, 16); }

HKM_FN float nan_value() {
    const unsigned b = NAN_BITS;
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}

#ifdef HKM_HOST
// (the host build states the contract of the wide accesses: the alignment row_wide() promised; the bounds are the sanitizer's)
template <typename T>
inline void load_group(const T* p, T (&v)[GROUP]) {
    if (!aligned_to(p, wide_align<T>())) abort();
    memcpy(v, p, sizeof v);
}
inline void store_quad(float* p, float a, float b, float c, float d) {
    if (!aligned_to(p, 16)) abort();
    const float q[4] = {a, b, c, d};
    memcpy(p, q, sizeof q);
}
#else
template <typename T>
__device__ __forceinline__ void load_group(const HKM_G T* p, T (&v)[GROUP]) {
    if constexpr (sizeof(T) == 1) {
        const unsigned long long w = *(const HKM_G unsigned long long*)p;
        HKM_UNROLL
        for (int i = 0; i < GROUP; ++i) v[i] = (T)(w >> (8 * i));
    } else {
        constexpr int PER = 16 / sizeof(T);
        typedef T quad_t __attribute__((ext_vector_type(PER)));
        HKM_UNROLL
        for (int q = 0; q < GROUP / PER; ++q) {
            const quad_t w = *((const HKM_G quad_t*)p + q);
            HKM_UNROLL
            for (int j = 0; j < PER; ++j) v[q * PER + j] = w[j];
        }
    }
}
typedef float f32x4_ __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_quad(HKM_G float* p, float a, float b, float c, float d) {
    *(HKM_G f32x4_*)p = f32x4_{a, b, c, d};
}
#endif

// The validity of group g as 8 bits, bit 7 - i for pixel 8g + i (the layout of a mask byte).  BITS: the byte itself.
HKM_FN unsigned bits_group(const HKM_G unsigned char* mask_row, long long g) { return mask_row[g]; }

// ALPHA: a pixel is valid iff its alpha sample is not 0.  `wide`: the group is whole and row_wide(alpha_row).  The bits of pixels
// at or past `width` are 0.
template <typename A>
HKM_FN unsigned alpha_group(const HKM_G A* alpha_row, long long g, long long width, bool wide) {
    const long long x = g * GROUP;
    unsigned valid = 0;
    if (wide) {
        A a[GROUP];
        load_group<A>(alpha_row + x, a);
        HKM_UNROLL
        for (int i = 0; i < GROUP; ++i) valid |= (unsigned)(a[i] != 0) << (7 - i);
    } else {
        HKM_UNROLL
        for (int i = 0; i < GROUP; ++i)
            if (x + i < width) valid |= (unsigned)(alpha_row[x + i] != 0) << (7 - i);
    }
    return valid;
}

// Group g of one band's row: out[x] = valid ? (float)in[x] : NaN for its pixels.  `wide`: the group is whole, row_wide(in_row) and
// out_row_wide(out_row).
// (the 8 results of a whole group, loaded wide: what put_group stores, and what the kernel's whole-wave path exchanges first)
template <typename T>
HKM_FN void wide_values(const HKM_G T* in_row, long long g, unsigned valid, float (&f)[GROUP]) {
    const float nan = nan_value();
    T v[GROUP];
    load_group<T>(in_row + g * GROUP, v);
    HKM_UNROLL
    for (int i = 0; i < GROUP; ++i) f[i] = ((valid >> (7 - i)) & 1u) ? (float)v[i] : nan;
}

template <typename T>
HKM_FN void put_group(const HKM_G T* in_row, HKM_G float* out_row, long long g, long long width, unsigned valid, bool wide) {
    const long long x = g * GROUP;
    const float nan = nan_value();
    if (wide) {
        float f[GROUP];
        wide_values<T>(in_row, g, valid, f);
        store_quad(out_row + x, f[0], f[1], f[2], f[3]);
        store_quad(out_row + x + 4, f[4], f[5], f[6], f[7]);
    } else {
        HKM_UNROLL
        for (int i = 0; i < GROUP; ++i)
            if (x + i < width) out_row[x + i] = ((valid >> (7 - i)) & 1u) ? (float)in_row[x + i] : nan;
    }
}

}  // namespace maskbits
}  // namespace hk
