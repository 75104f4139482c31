// hk_lzw.hip -- the LZW blocks (TIFF compression 5) of a GeoTIFF image decoded on the device and put in their place in the raster:
// hk_inflate.hip with another first stage.
//
// THE CONTRACT.  A block is a tile or a strip; its stream is TIFF 6.0 LZW (codes of 9 to 12 bits, most significant
// bit first, libtiff's early change) that gives at least the block's raw size -- rows x block_w x (spp of a pixel-interleaved
// block, else 1) x sample_bytes, rows = block_h, or what is left of the image in the last strip.  What lies behind the raw size is
// not looked at.  Anything else gives the block a status other than 0 (HK_LZW_*), leaves its pixels untouched and does not disturb
// the other blocks.
//
// lzw_block_kernel: one wave per workgroup, one workgroup per block; hk_lzw_core.h is the decoder (and says why it stays inside
// its memory, why it stops and how it is tested without a GPU).  The 32 KiB output ring, the 36 KiB string table and a 1 KiB input
// window are 69 KiB of LDS: two workgroups per CU.  The raw bytes go to the block's slot in `work` (raw size rounded up to 16),
// the status to status[block]; untile_kernel<ES> of hk_inflate.hip (untile_fp_kernel<ES> for predictor 3) follows as it does there
// (launch_untile).
#include <hip/hip_runtime.h>

#include "hk_lzw_core.h"
#include "hk_kernels.h"

namespace hk {

namespace {

typedef __attribute__((address_space(1))) const long long g_cll;
typedef __attribute__((address_space(1))) int g_int;

__device__ __forceinline__ long long uni64(long long v) {
    const unsigned lo = lzw::uni((unsigned)v), hi = lzw::uni((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

}  // namespace

__global__ void __launch_bounds__(lzw::WAVE) lzw_block_kernel(const InflateArgs a) {
    __shared__ lzw::Shared S;
    const long long b = blockIdx.x;
    const int by = (int)(b % ((long long)a.across * a.down)) / a.across;   // the block row (hk_inflate.hip block_place)
    const int rows = a.tiled ? a.bh : (a.bh < a.height - by * a.bh ? a.bh : a.height - by * a.bh);
    const unsigned raw = (unsigned)((long long)rows * a.bw * a.cspp * a.es);   // (at most HK_INFLATE_MAX_BLOCK: the launcher's check)
    const long long off = uni64(((g_cll*)a.offsets)[b]), size = uni64(((g_cll*)a.sizes)[b]);
    unsigned st = lzw::TRUNCATED;   // a stream that is not there
    if (off >= 0 && size > 0)
        st = lzw::lzw_stream(S, (lzw::in_ptr)a.streams + off, size, (lzw::out_ptr)a.work + b * a.slot, raw);
    if (threadIdx.x == 0) ((g_int*)a.status)[b] = (int)st;
}

hipError_t launch_lzw_image(InflateArgs a, long long n_blocks, hipStream_t stream) {
    if (n_blocks < 1 || n_blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    HK_LAUNCH(lzw_block_kernel, dim3((unsigned)n_blocks), dim3(lzw::WAVE), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_untile(a, n_blocks, stream);
}

}  // namespace hk
