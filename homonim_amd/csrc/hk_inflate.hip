// hk_inflate.hip -- the DEFLATE (zlib) blocks of a GeoTIFF image inflated on the device and put in their place in the raster: what
// tiff._decode_image otherwise does with zlib.decompress, np.cumsum and a slice copy, block after block on one host thread.
//
// THE CONTRACT.  A block is a tile or a strip; its stream is any legal zlib stream (stored, fixed and dynamic
// blocks, codes up to 15 bits, distances up to 32768, lengths up to 258, overlapping copies) that inflates to EXACTLY the block's
// raw size: rows x block_w x (spp of a pixel-interleaved block, else 1) x sample_bytes, where rows = block_h, or what is left of
// the image in the last strip.  Bytes behind the Adler-32 are not looked at.  Anything else gives the block a status other than
// 0 (HK_INFLATE_*), leaves its pixels untouched and does not disturb the other blocks.
//
// inflate_block_kernel: one wave per workgroup, one workgroup per block; hk_inflate_core.h is the decoder (and says why it stops
// and how it is tested without a GPU).  The 64 KiB output ring, a 1 KiB input window and the code tables are about 70 KiB of LDS:
// two workgroups per CU.  The raw bytes go to the block's slot in `work` (raw size rounded up to 16), the status to status[block].
// untile_kernel<ES>: one wave per block row and sample of a pixel: the slot's rows to the (spp, height, width) raster, cropped at
// the image's edge, pixel-interleaved samples to their planes; predictor 2 (horizontal differencing) is undone by a wave scan of
// 64 samples with a carry from step to step -- a modular sum in the sample's width.  Rows of one-sample blocks without a
// predictor move as 16-byte groups where everything is 16-byte aligned.  Blocks with a status are skipped.
// untile_fp_kernel<ES>, ES = 4 or 8: the same second stage for predictor 3 (the floating-point predictor; hk_fpred_core.h).
#include <hip/hip_runtime.h>

#include "hk_fpred_core.h"
#include "hk_inflate_core.h"
#include "hk_kernels.h"

namespace hk {

namespace {

using namespace inflate;

typedef __attribute__((address_space(1))) const long long g_cll;
typedef __attribute__((address_space(1))) const int g_cint;
typedef __attribute__((address_space(1))) int g_int;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 g_cuint4;
typedef __attribute__((address_space(1))) u32x4 g_uint4;

template <int ES> struct Sample;
template <> struct Sample<1> { typedef unsigned char type; typedef unsigned sum; };
template <> struct Sample<2> { typedef unsigned short type; typedef unsigned sum; };
template <> struct Sample<4> { typedef unsigned type; typedef unsigned sum; };
template <> struct Sample<8> { typedef unsigned long long type; typedef unsigned long long sum; };

__device__ __forceinline__ long long uni64(long long v) {
    const unsigned lo = uni((unsigned)v), hi = uni((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// block b of the image: its plane (0 for pixel-interleaved blocks), block row and block column
__device__ __forceinline__ void block_place(const InflateArgs& a, long long b, int& plane, int& by, int& bx) {
    const long long per = (long long)a.across * a.down;
    plane = (int)(b / per);
    const int rem = (int)(b % per);
    by = rem / a.across, bx = rem % a.across;
}

}  // namespace

__global__ void __launch_bounds__(inflate::WAVE) inflate_block_kernel(const InflateArgs a) {
    __shared__ Shared S;
    const long long b = blockIdx.x;
    int plane, by, bx;
    block_place(a, b, plane, by, bx);
    const int rows = a.tiled ? a.bh : (a.bh < a.height - by * a.bh ? a.bh : a.height - by * a.bh);
    const unsigned raw = (unsigned)((long long)rows * a.bw * a.cspp * a.es);   // (at most HK_INFLATE_MAX_BLOCK: the launcher's check)
    const long long off = uni64(((g_cll*)a.offsets)[b]), size = uni64(((g_cll*)a.sizes)[b]);
    unsigned st = TRUNCATED;   // a stream that is not there
    if (off >= 0 && size > 0)
        st = inflate_stream(S, (in_ptr)a.streams + off, size, (out_ptr)a.work + b * a.slot, raw);
    if (threadIdx.x == 0) ((g_int*)a.status)[b] = (int)st;
}

template <int ES>
__global__ void __launch_bounds__(256) untile_kernel(const InflateArgs a) {
    typedef typename Sample<ES>::type T;
    typedef typename Sample<ES>::sum Sum;
    typedef __attribute__((address_space(1))) const T g_cT;
    typedef __attribute__((address_space(1))) T g_T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.x;
    if (((g_cint*)a.status)[b] != 0) return;
    int plane, by, bx;
    block_place(a, b, plane, by, bx);
    const int y0 = by * a.bh, x0 = bx * a.bw;
    const int rows = a.bh < a.height - y0 ? a.bh : a.height - y0, cols = a.bw < a.width - x0 ? a.bw : a.width - x0;
    g_cT* const src = (g_cT*)((__attribute__((address_space(1))) const unsigned char*)a.work + b * a.slot);
    constexpr int N16 = 16 / ES;   // samples of a 16-byte group
    for (int r = blockIdx.y * 4 + wave; r < rows; r += gridDim.y * 4) {
        g_cT* const row = src + (long long)r * a.bw * a.cspp;
        for (int c = 0; c < a.cspp; ++c) {
            g_T* const dst = (g_T*)a.out + (long long)(a.separate ? plane : c) * a.band_stride + (long long)(y0 + r) * a.stride + x0;
            if (a.predictor == 2) {
                Sum carry = 0;
                for (int xs = 0; xs < cols; xs += 64) {
                    const int x = xs + lane;
                    Sum v = x < cols ? (Sum)row[(long long)x * a.cspp + c] : (Sum)0;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const Sum o = __shfl_up(v, d, 64);
                        if (lane >= d) v += o;
                    }
                    v += carry;
                    if (x < cols) dst[x] = (T)v;
                    carry = __shfl(v, 63, 64);
                }
            } else if (a.vec_ok && a.cspp == 1) {
                for (int x = lane * N16; x < cols; x += 64 * N16) {
                    if (x + N16 <= cols) {
                        *(g_uint4*)(dst + x) = *(g_cuint4*)(row + x);
                    } else {
                        for (int j = 0; x + j < cols; ++j) dst[x + j] = row[x + j];
                    }
                }
            } else {
                for (int x = lane; x < cols; x += 64) dst[x] = row[(long long)x * a.cspp + c];
            }
        }
    }
}

// untile_kernel<ES> for predictor 3 (hk_fpred_core.h states it): the same wave per block row and sample of a pixel, the same crop,
// de-interleaving and strides.  A first sweep over the row's bw pixels sums every plane's bytes of the sample's chain (one byte-wise
// wave reduction per four planes) and gives each plane what it starts from; a second sweep in steps of 64 pixels over [0, cols)
// scans the ES planes in lock-step, four to a word, with lane 63's word carried from step to step as in the predictor-2 path; the
// scanned words are the sample.  Nothing is sized by the row: a strip's row is as wide as the image.  Every byte read is at
// k * n + x * cspp + c with k < ES, x < bw, c < cspp: inside the row's n * ES bytes of the slot.
template <int ES>
__global__ void __launch_bounds__(256) untile_fp_kernel(const InflateArgs a) {
    typedef typename Sample<ES>::type T;
    typedef __attribute__((address_space(1))) T g_T;
    constexpr int W = ES / 4;   // words of four planes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.x;
    if (((g_cint*)a.status)[b] != 0) return;
    int plane, by, bx;
    block_place(a, b, plane, by, bx);
    const int y0 = by * a.bh, x0 = bx * a.bw;
    const int rows = a.bh < a.height - y0 ? a.bh : a.height - y0, cols = a.bw < a.width - x0 ? a.bw : a.width - x0;
    const fpred::in_ptr src = (fpred::in_ptr)a.work + b * a.slot;
    const long long n = (long long)a.bw * a.cspp;
    for (int r = blockIdx.y * 4 + wave; r < rows; r += gridDim.y * 4) {
        const fpred::in_ptr row = src + (long long)r * n * ES;
        for (int c = 0; c < a.cspp; ++c) {
            g_T* const dst = (g_T*)a.out + (long long)(a.separate ? plane : c) * a.band_stride + (long long)(y0 + r) * a.stride + x0;
            unsigned carry[W];
#pragma unroll
            for (int w = 0; w < W; ++w) carry[w] = 0;
            for (int x = lane; x < a.bw; x += 64) {
#pragma unroll
                for (int w = 0; w < W; ++w) carry[w] = fpred::add4(carry[w], fpred::load4(row, n, (long long)x * a.cspp + c, 4 * w));
            }
            unsigned before = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                unsigned t = carry[w];
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) t = fpred::add4(t, __shfl_xor(t, d, 64));
                carry[w] = fpred::carries4(t, before);
                before = (before + fpred::total4(t)) & 255u;
            }
            for (int xs = 0; xs < cols; xs += 64) {
                const int x = xs + lane;
                unsigned v[W];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    v[w] = x < cols ? fpred::load4(row, n, (long long)x * a.cspp + c, 4 * w) : 0u;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const unsigned o = __shfl_up(v[w], d, 64);
                        if (lane >= d) v[w] = fpred::add4(v[w], o);
                    }
                    v[w] = fpred::add4(v[w], carry[w]);
                    carry[w] = __shfl(v[w], 63, 64);
                }
                if (x < cols) {
                    if constexpr (W == 1) dst[x] = v[0];
                    else dst[x] = ((unsigned long long)v[0] << 32) | v[W - 1];
                }
            }
        }
    }
}

hipError_t launch_inflate_image(InflateArgs a, long long n_blocks, hipStream_t stream) {
    if (n_blocks < 1 || n_blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    HK_LAUNCH(inflate_block_kernel, dim3((unsigned)n_blocks), dim3(inflate::WAVE), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_untile(a, n_blocks, stream);
}

// the second stage, behind whatever filled the slots and the statuses (hk_lzw.hip launches it too)
hipError_t launch_untile(InflateArgs a, long long n_blocks, hipStream_t stream) {
    if (n_blocks < 1 || n_blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    a.vec_ok = a.cspp == 1 && ((uintptr_t)a.out % 16 == 0) && ((uintptr_t)a.work % 16 == 0) && ((a.stride * a.es) % 16 == 0) &&
               ((a.band_stride * a.es) % 16 == 0) && (((long long)a.bw * a.es) % 16 == 0);
    const int rows = a.bh < a.height ? a.bh : a.height;
    const dim3 grid((unsigned)n_blocks, (unsigned)((rows + 3) / 4 < 64 ? (rows + 3) / 4 : 64));
    if (a.predictor == 3) {
        switch (a.es) {
            case 4: HK_LAUNCH(untile_fp_kernel<4>, grid, dim3(256), 0, stream, a); break;
            case 8: HK_LAUNCH(untile_fp_kernel<8>, grid, dim3(256), 0, stream, a); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (a.es) {
        case 1: HK_LAUNCH(untile_kernel<1>, grid, dim3(256), 0, stream, a); break;
        case 2: HK_LAUNCH(untile_kernel<2>, grid, dim3(256), 0, stream, a); break;
        case 4: HK_LAUNCH(untile_kernel<4>, grid, dim3(256), 0, stream, a); break;
        case 8: HK_LAUNCH(untile_kernel<8>, grid, dim3(256), 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace hk
