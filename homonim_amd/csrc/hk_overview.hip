// hk_overview.hip -- the internal overviews of homonim/fuse.py:152-165 (RasterFuse.build_overviews: factors 2, 4, ... with
// Resampling.average): every level of the pyramid from ONE pass over the source.
//
// Semantics.  Level m has shape (ceil(H / 2^m), ceil(W / 2^m)) and is computed from level m - 1 AS STORED: its
// pixel (i, j) takes the pixels (2i..2i+1, 2j..2j+1) of level m - 1 that lie inside that level and are valid under
// (nodata_mode, nodata) -- NONE: all (a NaN is data and propagates), NAN: not NaN, VALUE: not equal to the value.  A cell without
// a valid pixel gives nodata.  float32: the valid values summed as float64 in row-major order, divided by their count in float64,
// rounded once (bit-identical to resample_kernel<5> of hk_resample.hip for the mapping (2, 0, 2, 0)); float64: the same without
// the rounding; integers: floor((2 S + n) / (2 n)) of the exact 64-bit sum S -- round half up.  (2 S + n < 2^36 is exact as a
// double, and a quotient that is not an integer is at least 1 / 8 away from one, so floor of the float64 division is exact.)
//
// One workgroup owns a source tile of 64 rows x TW columns (TW = 64 pixels of 4 or 8 bytes, 128 of 2, 256 of 1: at least 256
// bytes per row), reads it with one 16-byte load per lane and row, forms level 1 in registers -- a lane that holds the same
// 16 bytes of two adjacent rows owns 8 bytes of complete cells -- and hands levels 2..6 down through LDS (two buffers, one
// barrier per level), storing every level as it goes: 6 levels per launch, which is all six of a 16384^2 raster.
// WHY THE CASCADE INSIDE A TILE IS THE GLOBAL CASCADE: tile origins are multiples of 64 = 2^6 in both directions, so on level
// m - 1 (m <= 6) a tile starts at an even index, and the 2 x 2 cell of any level-m pixel never straddles two tiles; a cell is
// clipped against the GLOBAL shape of level m - 1 (ceil(H / 2^(m-1)), ...), which is what an odd edge means.  Deeper levels (at
// most 2 of the 8 the rule allows, 4^-6 of the data) come from a second launch of the same kernel over level 6.
// The arithmetic of a cell does not depend on how its pixels were loaded: where 16-byte loads are not legal (base or strides
// not 16-byte aligned, the raster's last columns) a scalar path reads the same elements, so the bits do not depend on alignment.
//
// HBM-bound: one read of the source + 1/3 of it written, no atomics.  The sample type is a template argument; the nodata mode is
// a RUN-TIME value: validity is two compares combined with the (wave-uniform) mode without a branch -- the disassembly of the
// pixel path holds v_cmp / s_and only, no s_cbranch on the mode -- and a third of the builds the launch ledger has to see checked.
//
// THE MASKED BUILD (overview_valid_kernel): validity comes from a uint8 plane of the raster (255 / 0, one plane for
// all bands) instead of from a nodata value.  A pixel counts where it lies inside its level AND its validity byte is not 0; the
// arithmetic of a cell is the one above under mode NONE (a NaN under a valid byte is data and propagates); a cell without a valid
// pixel gives 0 (integers) or NaN (floats).  The same pass writes every level's own validity plane -- 255 where the cell had a
// valid pixel -- through a second pair of LDS buffers, and level m + 1 cascades from level m's values and validity as stored.  A
// lane reads the validity of its VEC pixels with one VEC-byte load (16 .. 2 bytes) where that is legal, else byte by byte: the
// same bits either way.  The workgroups of band 0 store the validity planes.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hk_kernels.h"

namespace hk {

namespace {

constexpr int OVW_THREADS = 256;
constexpr int OVW_ROWS = 1 << OVERVIEW_PASS_LEVELS;  // tile rows

template <class T>
__device__ __forceinline__ bool ovalid(T v, int mode, double nodata) {
    if constexpr (std::is_floating_point<T>::value)
        return !(((mode == 1) & (v != v)) | ((mode == 2) & ((double)v == nodata)));
    else
        return !((mode == 2) & ((double)v == nodata));
}

// one output pixel from the (up to) four pixels of its cell in row-major order; p*: the pixel lies inside the source level
template <class T>
__device__ __forceinline__ T cell(T a, T b, T c, T d, bool pa, bool pb, bool pc, bool pd, int mode, double nodata, T fill) {
    const bool ma = pa & ovalid(a, mode, nodata), mb = pb & ovalid(b, mode, nodata), mc = pc & ovalid(c, mode, nodata),
               md = pd & ovalid(d, mode, nodata);
    const int n = (int)ma + (int)mb + (int)mc + (int)md;
    if constexpr (std::is_floating_point<T>::value) {
        double s = 0.0;  // masked pixels add zeros (the sum starts at +0 and never is -0: adding +0 changes nothing)
        s += ma ? (double)a : 0.0;
        s += mb ? (double)b : 0.0;
        s += mc ? (double)c : 0.0;
        s += md ? (double)d : 0.0;
        return n ? (T)(s / (double)n) : fill;
    } else {
        long long s = 0;
        s += ma ? (long long)a : 0;
        s += mb ? (long long)b : 0;
        s += mc ? (long long)c : 0;
        s += md ? (long long)d : 0;
        return n ? (T)(long long)floor((double)(2 * s + n) / (double)(2 * n)) : fill;
    }
}

// the unsigned word of N bytes: N validity bytes as one load / store
template <int N> struct Word;
template <> struct Word<16> { using type = uint4; };
template <> struct Word<8> { using type = uint2; };
template <> struct Word<4> { using type = unsigned; };
template <> struct Word<2> { using type = unsigned short; };
template <> struct Word<1> { using type = unsigned char; };

template <class T>
struct Tile {
    static constexpr int VEC = 16 / (int)sizeof(T);                              // pixels per 16-byte load
    static constexpr int TW = sizeof(T) >= 4 ? 64 : 256 / (int)sizeof(T);        // tile columns
    static constexpr int QPR = TW / VEC;                                         // lanes per tile row
};

// VEC pixels of one row from column gx on (`rem` = width - gx of them exist, none when !row_ok); absent ones read as 0
template <class T>
__device__ __forceinline__ void load_row(const T* __restrict__ p, int rem, bool row_ok, bool vec_ok, T (&r)[Tile<T>::VEC]) {
    constexpr int VEC = Tile<T>::VEC;
    if (row_ok && vec_ok && rem >= VEC) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        __builtin_memcpy(r, &t, 16);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) r[i] = (row_ok && i < rem) ? p[i] : T(0);
    }
}

// the validity bytes of N pixels of one row, as load_row reads the pixels; absent ones read as 0 (invalid)
template <int N>
__device__ __forceinline__ void load_valid(const unsigned char* __restrict__ p, int rem, bool row_ok, bool vec_ok,
                                           unsigned char (&r)[N]) {
    if (row_ok && vec_ok && rem >= N) {
        const typename Word<N>::type t = *reinterpret_cast<const typename Word<N>::type*>(p);
        __builtin_memcpy(r, &t, N);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) r[i] = (row_ok && i < rem) ? p[i] : (unsigned char)0;
    }
}

// level M (2..6) of the tile from level M - 1 in LDS; stores it to LDS and to the level's plane.  MASKED: validity from / to
// lvsrc / lvdst beside the values, and to the level's validity plane
template <int M, bool MASKED, class T>
__device__ __forceinline__ void level_step(const OverviewArgs& a, const OverviewValid* v, const T* __restrict__ lsrc,
                                           T* __restrict__ ldst, const unsigned char* __restrict__ lvsrc,
                                           unsigned char* __restrict__ lvdst, int band, T fill) {
    constexpr int TW = Tile<T>::TW;
    constexpr int hm = OVW_ROWS >> M, wm = TW >> M, ws = TW >> (M - 1);
    const int sh = (a.height + (1 << (M - 1)) - 1) >> (M - 1), sw = (a.width + (1 << (M - 1)) - 1) >> (M - 1);  // level M - 1
    const int sy0 = blockIdx.y * (OVW_ROWS >> (M - 1)), sx0 = blockIdx.x * ws;
    T* __restrict__ out = static_cast<T*>(a.out[M - 1]) + (long long)band * a.out_band_stride[M - 1];
    for (int c = threadIdx.x; c < hm * wm; c += OVW_THREADS) {
        const int i = c / wm, j = c % wm;
        const bool y0 = sy0 + 2 * i < sh, y1 = sy0 + 2 * i + 1 < sh, x0 = sx0 + 2 * j < sw, x1 = sx0 + 2 * j + 1 < sw;
        const T* __restrict__ q = lsrc + 2 * i * ws + 2 * j;
        bool pa = y0 & x0, pb = y0 & x1, pc = y1 & x0, pd = y1 & x1;
        if constexpr (MASKED) {
            const unsigned char* __restrict__ qv = lvsrc + 2 * i * ws + 2 * j;
            pa &= qv[0] != 0, pb &= qv[1] != 0, pc &= qv[ws] != 0, pd &= qv[ws + 1] != 0;
        }
        const T val = cell<T>(q[0], q[1], q[ws], q[ws + 1], pa, pb, pc, pd, a.nd_mode, a.nodata, fill);
        ldst[i * wm + j] = val;
        if (y0 & x0) out[(long long)(blockIdx.y * hm + i) * a.out_stride[M - 1] + blockIdx.x * wm + j] = val;
        if constexpr (MASKED) {
            const unsigned char ok = (pa | pb | pc | pd) ? 255 : 0;
            lvdst[i * wm + j] = ok;
            if ((y0 & x0) && band == 0)
                v->out[M - 1][(long long)(blockIdx.y * hm + i) * v->out_stride[M - 1] + blockIdx.x * wm + j] = ok;
        }
    }
}

// level 1 of the tile in registers: lane `item` holds VEC pixels of rows 2 rp and 2 rp + 1 and owns the VEC / 2 cells under them.
// INTERIOR (the whole tile lies inside the raster and 16-byte loads are legal; wave-uniform): no bounds, and the loads of all of
// the lane's items (2, or 4 of float64) are issued before the first cell is formed.  MASKED: the validity bytes of the same pixels
// are loaded beside them, and the cells' validity goes to lds_va and, from band 0, to the level-1 validity plane.
template <bool INTERIOR, bool MASKED, class T>
__device__ __forceinline__ void level_one(const OverviewArgs& a, const OverviewValid* v, const T* __restrict__ plane,
                                          T* __restrict__ out1, T* __restrict__ lds_a, unsigned char* __restrict__ lds_va, T fill) {
    constexpr int VEC = Tile<T>::VEC, TW = Tile<T>::TW, QPR = Tile<T>::QPR, HALF = VEC / 2;
    constexpr int ITEMS = QPR * (OVW_ROWS / 2), NIT = ITEMS / OVW_THREADS;
    static_assert(ITEMS % OVW_THREADS == 0, "every lane owns the same number of items");
    const int w1 = (a.width + 1) >> 1;
    const int y0 = blockIdx.y * OVW_ROWS, x0 = blockIdx.x * TW;
    // the cells under one item's two rows: to LDS and to the level-1 plane
    auto finish = [&](int q, int rp, const T(&r0)[VEC], const T(&r1)[VEC], const unsigned char* v0, const unsigned char* v1,
                      bool r0ok, bool r1ok, int rem) {
        const int gy = y0 + 2 * rp, gx = x0 + q * VEC;
        T res[HALF];
        unsigned char ok[HALF];
#pragma unroll
        for (int c = 0; c < HALF; ++c) {
            const bool c0 = 2 * c < rem, c1 = 2 * c + 1 < rem;
            bool pa = r0ok & c0, pb = r0ok & c1, pc = r1ok & c0, pd = r1ok & c1;
            if constexpr (MASKED) {
                pa &= v0[2 * c] != 0, pb &= v0[2 * c + 1] != 0, pc &= v1[2 * c] != 0, pd &= v1[2 * c + 1] != 0;
                ok[c] = (pa | pb | pc | pd) ? 255 : 0;
            }
            res[c] = cell<T>(r0[2 * c], r0[2 * c + 1], r1[2 * c], r1[2 * c + 1], pa, pb, pc, pd, a.nd_mode, a.nodata, fill);
        }
        uint2 packed;
        __builtin_memcpy(&packed, res, 8);
        *reinterpret_cast<uint2*>(&lds_a[rp * (TW / 2) + q * HALF]) = packed;
        const int ox = gx >> 1;
        T* __restrict__ o = out1 + (long long)(gy >> 1) * a.out_stride[0] + ox;
        if (r0ok && a.out_vec_ok && ox + HALF <= w1) {
            *reinterpret_cast<uint2*>(o) = packed;
        } else if (r0ok) {
#pragma unroll
            for (int c = 0; c < HALF; ++c)
                if (ox + c < w1) o[c] = res[c];
        }
        if constexpr (MASKED) {
            typename Word<HALF>::type word;
            __builtin_memcpy(&word, ok, HALF);
            *reinterpret_cast<typename Word<HALF>::type*>(&lds_va[rp * (TW / 2) + q * HALF]) = word;
            if (blockIdx.z == 0 && r0ok) {
                unsigned char* __restrict__ ov = v->out[0] + (long long)(gy >> 1) * v->out_stride[0] + ox;
                if (v->out_vec_ok && ox + HALF <= w1) {
                    *reinterpret_cast<typename Word<HALF>::type*>(ov) = word;
                } else {
#pragma unroll
                    for (int c = 0; c < HALF; ++c)
                        if (ox + c < w1) ov[c] = ok[c];
                }
            }
        }
    };
    if constexpr (INTERIOR) {
        T r0[NIT][VEC], r1[NIT][VEC];
        unsigned char v0[MASKED ? NIT : 1][VEC], v1[MASKED ? NIT : 1][VEC];
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int item = threadIdx.x + k * OVW_THREADS;
            const T* __restrict__ p = plane + (long long)(y0 + 2 * (item / QPR)) * a.stride + x0 + (item % QPR) * VEC;
            load_row<T>(p, VEC, true, true, r0[k]);
            load_row<T>(p + a.stride, VEC, true, true, r1[k]);
            if constexpr (MASKED) {
                const unsigned char* __restrict__ pv = v->src + (long long)(y0 + 2 * (item / QPR)) * v->stride + x0 + (item % QPR) * VEC;
                load_valid<VEC>(pv, VEC, true, true, v0[k]);
                load_valid<VEC>(pv + v->stride, VEC, true, true, v1[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int item = threadIdx.x + k * OVW_THREADS;
            finish(item % QPR, item / QPR, r0[k], r1[k], v0[MASKED ? k : 0], v1[MASKED ? k : 0], true, true, VEC);
        }
    } else {
        for (int item = threadIdx.x; item < ITEMS; item += OVW_THREADS) {
            const int q = item % QPR, rp = item / QPR;
            const int gy = y0 + 2 * rp, gx = x0 + q * VEC;
            const bool r0ok = gy < a.height, r1ok = gy + 1 < a.height;
            const T* __restrict__ p = plane + (long long)gy * a.stride + gx;
            T r0[VEC], r1[VEC];
            unsigned char v0[VEC], v1[VEC];
            load_row<T>(p, a.width - gx, r0ok, a.vec_ok, r0);
            load_row<T>(p + a.stride, a.width - gx, r1ok, a.vec_ok, r1);
            if constexpr (MASKED) {
                const unsigned char* __restrict__ pv = v->src + (long long)gy * v->stride + gx;
                load_valid<VEC>(pv, a.width - gx, r0ok, v->vec_ok, v0);
                load_valid<VEC>(pv + v->stride, a.width - gx, r1ok, v->vec_ok, v1);
            }
            finish(q, rp, r0, r1, v0, v1, r0ok, r1ok, a.width - gx);
        }
    }
}

// one tile of one band through all levels of the launch; `v`: the validity planes of the masked build, unused otherwise
template <bool MASKED, class T>
__device__ __forceinline__ void overview_tile(const OverviewArgs& a, const OverviewValid* v) {
    constexpr int TW = Tile<T>::TW;
    static_assert(Tile<T>::VEC / 2 * sizeof(T) == 8, "a lane's level-1 pixels are one 8-byte store");
    __shared__ __attribute__((aligned(16))) T lds_a[(OVW_ROWS / 2) * (TW / 2)];
    __shared__ __attribute__((aligned(16))) T lds_b[(OVW_ROWS / 4) * (TW / 4)];
    __shared__ __attribute__((aligned(16))) unsigned char lds_va[MASKED ? (OVW_ROWS / 2) * (TW / 2) : 1];
    __shared__ __attribute__((aligned(16))) unsigned char lds_vb[MASKED ? (OVW_ROWS / 4) * (TW / 4) : 1];
    const int band = blockIdx.z;
    const T* __restrict__ plane = static_cast<const T*>(a.src) + (long long)band * a.band_stride;
    T* __restrict__ out1 = static_cast<T*>(a.out[0]) + (long long)band * a.out_band_stride[0];
    // what a cell without a valid pixel gets: the nodata, and under a mask (nd_mode is 0 then) NaN in a float type
    const T fill = (a.nd_mode == 0) ? ((MASKED && std::is_floating_point<T>::value) ? (T)__builtin_nanf("") : T(0)) : (T)a.nodata;
    const int y0 = blockIdx.y * OVW_ROWS, x0 = blockIdx.x * TW;
    if (a.vec_ok && (!MASKED || v->vec_ok) && y0 + OVW_ROWS <= a.height && x0 + TW <= a.width)
        level_one<true, MASKED, T>(a, v, plane, out1, lds_a, lds_va, fill);
    else
        level_one<false, MASKED, T>(a, v, plane, out1, lds_a, lds_va, fill);
    if (a.n_levels < 2) return;
    __syncthreads();
    level_step<2, MASKED, T>(a, v, lds_a, lds_b, lds_va, lds_vb, band, fill);
    if (a.n_levels < 3) return;
    __syncthreads();
    level_step<3, MASKED, T>(a, v, lds_b, lds_a, lds_vb, lds_va, band, fill);
    if (a.n_levels < 4) return;
    __syncthreads();
    level_step<4, MASKED, T>(a, v, lds_a, lds_b, lds_va, lds_vb, band, fill);
    if (a.n_levels < 5) return;
    __syncthreads();
    level_step<5, MASKED, T>(a, v, lds_b, lds_a, lds_vb, lds_va, band, fill);
    if (a.n_levels < 6) return;
    __syncthreads();
    level_step<6, MASKED, T>(a, v, lds_a, lds_b, lds_va, lds_vb, band, fill);
}

}  // namespace

template <class T>
__global__ void __launch_bounds__(OVW_THREADS) overview_kernel(const OverviewArgs a) {
    overview_tile<false, T>(a, nullptr);
}

template <class T>
__global__ void __launch_bounds__(OVW_THREADS) overview_valid_kernel(const OverviewArgs a, const OverviewValid v) {
    overview_tile<true, T>(a, &v);
}

namespace {

template <class T>
int tile_width() { return Tile<T>::TW; }

bool aligned_to(const void* p, long long stride, long long band_stride, int esize, int bytes) {
    return ((uintptr_t)p % bytes == 0) && ((stride * esize) % bytes == 0) && ((band_stride * esize) % bytes == 0);
}

}  // namespace

hipError_t launch_overviews(int dtype, const OverviewLevels& r, hipStream_t stream) {
    const int esize = dtype_size(dtype);
    if (!esize) return hipErrorInvalidValue;
    const bool is_float = dtype == 0 || dtype == 6;
    BandPlanes p = r.planes;  // what a pass reads: the raster, then the coarsest level of the pass before
    const unsigned char* valid = r.valid;  // ... and, in the masked build, its validity plane
    long long valid_stride = r.valid_stride;
    for (int l0 = 0; l0 < r.n_levels; l0 += OVERVIEW_PASS_LEVELS) {
        OverviewArgs a;
        memset(&a, 0, sizeof(a));
        a.src = p.src, a.height = p.height, a.width = p.width, a.stride = p.stride, a.band_stride = p.band_stride;
        a.nd_mode = (valid || (!is_float && r.nd_mode == 1)) ? 0 : r.nd_mode;  // an integer never is NaN; a mask replaces the nodata
        a.nodata = dtype == 0 ? (double)(float)r.nodata : r.nodata;
        a.n_levels = r.n_levels - l0 < OVERVIEW_PASS_LEVELS ? r.n_levels - l0 : OVERVIEW_PASS_LEVELS;
        for (int k = 0; k < a.n_levels; ++k)
            a.out[k] = r.out[l0 + k], a.out_stride[k] = r.out_stride[l0 + k], a.out_band_stride[k] = r.out_band_stride[l0 + k];
        a.vec_ok = aligned_to(p.src, p.stride, p.band_stride, esize, 16);
        a.out_vec_ok = aligned_to(a.out[0], a.out_stride[0], a.out_band_stride[0], esize, 8);
        const int tw = esize >= 4 ? tile_width<float>() : (esize == 2 ? tile_width<short>() : tile_width<unsigned char>());
        const dim3 grid((p.width + tw - 1) / tw, (p.height + OVW_ROWS - 1) / OVW_ROWS, p.n_bands), block(OVW_THREADS);
        if (valid) {
            OverviewValid v;
            memset(&v, 0, sizeof(v));
            v.src = valid, v.stride = valid_stride;
            for (int k = 0; k < a.n_levels; ++k) v.out[k] = r.out_valid[l0 + k], v.out_stride[k] = r.out_valid_stride[l0 + k];
            v.vec_ok = aligned_to(valid, valid_stride, 0, 1, 16);
            v.out_vec_ok = aligned_to(v.out[0], v.out_stride[0], 0, 1, 8);
            switch (dtype) {
                case 0: HK_LAUNCH(overview_valid_kernel<float>, grid, block, 0, stream, a, v); break;
                case 1: HK_LAUNCH(overview_valid_kernel<unsigned char>, grid, block, 0, stream, a, v); break;
                case 2: HK_LAUNCH(overview_valid_kernel<unsigned short>, grid, block, 0, stream, a, v); break;
                case 3: HK_LAUNCH(overview_valid_kernel<short>, grid, block, 0, stream, a, v); break;
                case 4: HK_LAUNCH(overview_valid_kernel<unsigned int>, grid, block, 0, stream, a, v); break;
                case 5: HK_LAUNCH(overview_valid_kernel<int>, grid, block, 0, stream, a, v); break;
                default: HK_LAUNCH(overview_valid_kernel<double>, grid, block, 0, stream, a, v); break;
            }
            valid = v.out[a.n_levels - 1], valid_stride = v.out_stride[a.n_levels - 1];
        } else switch (dtype) {
            case 0: HK_LAUNCH(overview_kernel<float>, grid, block, 0, stream, a); break;
            case 1: HK_LAUNCH(overview_kernel<unsigned char>, grid, block, 0, stream, a); break;
            case 2: HK_LAUNCH(overview_kernel<unsigned short>, grid, block, 0, stream, a); break;
            case 3: HK_LAUNCH(overview_kernel<short>, grid, block, 0, stream, a); break;
            case 4: HK_LAUNCH(overview_kernel<unsigned int>, grid, block, 0, stream, a); break;
            case 5: HK_LAUNCH(overview_kernel<int>, grid, block, 0, stream, a); break;
            default: HK_LAUNCH(overview_kernel<double>, grid, block, 0, stream, a); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const int k = a.n_levels;
        p.src = a.out[k - 1], p.stride = a.out_stride[k - 1], p.band_stride = a.out_band_stride[k - 1];
        p.height = (int)(((long long)p.height + (1 << k) - 1) >> k), p.width = (int)(((long long)p.width + (1 << k) - 1) >> k);
    }
    return hipSuccess;
}

}  // namespace hk
