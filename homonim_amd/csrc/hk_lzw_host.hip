// hk_lzw_host.hip -- hk_lzw_image_host: the LZW blocks of a GeoTIFF image decoded on the calling thread, for callers without a
// device at hand and as the default of the product's `inflate` switch.  The decoder is the HOST build of hk_lzw_core.h -- the
// functions of lzw_block_kernel with a loop over the lane index in place of the wave -- and what untile_kernel<ES> does behind it
// (crop, de-interleave, predictor 2) is plain C++ here, and what untile_fp_kernel<ES> does for predictor 3 is the row function of
// hk_fpred_core.h.  No kernel, no HIP call.
#define HKI_HOST
#include "hk_fpred_core.h"
#include "hk_lzw_core.h"
#include "hk_kernels.h"

#include <memory>

namespace hk {

namespace {

// block b's slot to the (spp, height, width) raster: hk_inflate.hip untile_kernel<ES>, one row and sample after the other
template <typename T>
void untile_block(const InflateArgs& a, int plane, int by, int bx, const unsigned char* slot) {
    const int y0 = by * a.bh, x0 = bx * a.bw;
    const int rows = a.bh < a.height - y0 ? a.bh : a.height - y0, cols = a.bw < a.width - x0 ? a.bw : a.width - x0;
    const T* const src = reinterpret_cast<const T*>(slot);
    for (int r = 0; r < rows; ++r) {
        const T* const row = src + (long long)r * a.bw * a.cspp;
        for (int c = 0; c < a.cspp; ++c) {
            T* const dst = static_cast<T*>(a.out) + (long long)(a.separate ? plane : c) * a.band_stride + (long long)(y0 + r) * a.stride + x0;
            if constexpr (sizeof(T) >= 4) {
                if (a.predictor == 3) {   // (4- and 8-byte samples only: the caller's check)
                    fpred::unpredict_row<(int)sizeof(T), T>(reinterpret_cast<const unsigned char*>(row), a.bw, a.cspp, c, cols, dst);
                    continue;
                }
            }
            T sum = 0;   // (predictor 2: a modular sum in the sample's width)
            for (int x = 0; x < cols; ++x) {
                const T v = row[(long long)x * a.cspp + c];
                dst[x] = a.predictor == 2 ? (sum = (T)(sum + v)) : v;
            }
        }
    }
}

}  // namespace

long long lzw_image_host(const InflateArgs& a, long long n_blocks, int* first_status) {
    std::unique_ptr<lzw::Shared> S(new lzw::Shared());
    const long long per = (long long)a.across * a.down;
    long long first_bad = -1;
    for (long long b = 0; b < n_blocks; ++b) {
        const int plane = (int)(b / per), rem = (int)(b % per), by = rem / a.across, bx = rem % a.across;
        const int rows = a.tiled ? a.bh : (a.bh < a.height - by * a.bh ? a.bh : a.height - by * a.bh);
        const unsigned raw = (unsigned)((long long)rows * a.bw * a.cspp * a.es);
        const long long off = a.offsets[b], size = a.sizes[b];
        unsigned st = lzw::TRUNCATED;   // a stream that is not there
        if (off >= 0 && size > 0) st = lzw::lzw_stream(*S, static_cast<const unsigned char*>(a.streams) + off, size, a.work, raw);
        if (a.status) a.status[b] = (int)st;
        if (st) {
            if (first_bad < 0) first_bad = b, *first_status = (int)st;
            continue;
        }
        switch (a.es) {
            case 1: untile_block<unsigned char>(a, plane, by, bx, a.work); break;
            case 2: untile_block<unsigned short>(a, plane, by, bx, a.work); break;
            case 4: untile_block<unsigned>(a, plane, by, bx, a.work); break;
            default: untile_block<unsigned long long>(a, plane, by, bx, a.work); break;
        }
    }
    return first_bad;
}

}  // namespace hk
