// hk_fpred_core.h -- TIFF predictor 3 (libtiff's floating-point predictor, fpAcc) undone on one block row: the arithmetic that the
// second stage of the block decoders (hk_inflate.hip untile_fp_kernel<ES>) and the library's host decoder (hk_lzw_host.hip) share.
// A host program compiles it as plain C++ (HKI_HOST, as hk_inflate_core.h): tests/c/fpred_core_host.cpp.
//
// THE STATEMENT (tiff._unpredict_float is its numpy form and the tests' oracle).  One block row holds bw pixels of
// cspp samples of es bytes (es = 4 or 8): n = bw * cspp samples, n * es raw bytes.
//   * the raw bytes are summed byte by byte, modulo 256, at a distance of cspp, over the WHOLE row: s[i] = raw[i] + s[i - cspp]
//     (s[i] = raw[i] for i < cspp).  The sum runs straight across the plane boundaries.
//   * the summed row is es planes of n bytes, the most significant byte of every sample first: byte k (0 the most significant) of
//     sample (x, c) is s[k * n + x * cspp + c].
//   * the output sample is little-endian.
// The row is always bw wide: in an edge tile of which only cols < bw pixels are stored, the planes still start at multiples of
// n = bw * cspp, and the bytes of the pixels that are cropped away still count in the sums of the planes behind them.
//
// HOW IT IS COMPUTED.  The bytes at i = c (mod cspp) are one chain per sample c of a pixel; in plane k the chain has the bw bytes
// raw[k * n + x * cspp + c].  With T[k] the sum of plane k's bytes of the chain,
//     s[k * n + x * cspp + c] = T[0] + ... + T[k - 1]  +  the sum of plane k's bytes of the chain up to and including pixel x,
// so a first sweep over all bw pixels gives every plane's carry-in, and a second sweep over the cols stored pixels scans the es
// planes in lock-step.  Four planes travel in one 32-bit word, the first plane in the highest byte, and are added byte-wise
// (add4): the scanned word of planes 0..3 IS the float32 sample's bit pattern, and two words are the float64's.
#pragma once
#include "hk_inflate_core.h"

namespace hk {
namespace fpred {

using inflate::in_ptr;

// four sums modulo 256 at once: no carry passes from one byte to the next
HKI_FN unsigned add4(unsigned a, unsigned b) { return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u); }

// the raw bytes of planes k0 .. k0 + 3 at `at` = x * cspp + c of a row whose planes are n bytes apart; plane k0 highest
HKI_FN unsigned load4(in_ptr row, long long n, long long at, int k0) {
    in_ptr const p = row + k0 * n + at;
    return ((unsigned)p[0] << 24) | ((unsigned)p[n] << 16) | ((unsigned)p[2 * n] << 8) | (unsigned)p[3 * n];
}

// the sum of a word's four bytes, modulo 256
HKI_FN unsigned total4(unsigned t) { return ((t >> 24) + (t >> 16) + (t >> 8) + t) & 255u; }

// what each of a word's four planes starts from: the totals of the planes before it -- those of the word itself (`t`: the four
// planes' totals), and `before`, the sum modulo 256 of the totals of all planes of the words before this one
HKI_FN unsigned carries4(unsigned t, unsigned before) {
    const unsigned s = t >> 8;   // (the highest byte is 0 from here on: shifting further brings nothing in)
    return add4(add4(s, s >> 8), add4(s >> 16, before * 0x01010101u));
}

#ifdef HKI_HOST
// sample c of the first `cols` pixels of one row to dst[0 .. cols): the two sweeps one pixel at a time.  T is the unsigned integer
// of ES bytes; the host is little-endian (as everywhere in the host decoder, whose samples are the raster's).
template <int ES, typename T>
inline void unpredict_row(const unsigned char* row, int bw, int cspp, int c, int cols, T* dst) {
    static_assert((ES == 4 || ES == 8) && sizeof(T) == ES, "float32 or float64");
    constexpr int W = ES / 4;
    const long long n = (long long)bw * cspp;
    unsigned acc[W] = {};
    for (int x = 0; x < bw; ++x)
        for (int w = 0; w < W; ++w) acc[w] = add4(acc[w], load4(row, n, (long long)x * cspp + c, 4 * w));
    unsigned before = 0;
    for (int w = 0; w < W; ++w) {
        const unsigned t = acc[w];
        acc[w] = carries4(t, before);
        before = (before + total4(t)) & 255u;
    }
    for (int x = 0; x < cols; ++x) {
        for (int w = 0; w < W; ++w) acc[w] = add4(acc[w], load4(row, n, (long long)x * cspp + c, 4 * w));
        unsigned long long v = acc[0];
        if (W == 2) v = (v << 32) | acc[W - 1];
        dst[x] = (T)v;
    }
}
#endif

}  // namespace fpred
}  // namespace hk
