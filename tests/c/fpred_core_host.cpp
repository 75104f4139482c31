// The predictor-3 row function of the library's host decoder (homonim_amd/csrc/hk_fpred_core.h, HKI_HOST) as a plain C++ program.
// tests/test_predictor3_cpu.py runs it, built with AddressSanitizer + UBSan, over the raw blocks of its layouts.
//
//   fpred_core_host IN
// IN: uint32 n, then n times { uint32 es, bw, cspp, rows, cols, then rows x bw x cspp x es raw bytes }   (little-endian)
// Prints one line per block: "s1 s2", the sums over the block's output bytes b[i] -- row after row, within a row sample c of a
// pixel after sample c - 1, cols little-endian samples each -- of b[i] and of (i + 1) x b[i], modulo 2^64.
// Every block and every output row is a malloc of exactly its size, so that the sanitizer sees any access outside them.
#define HKI_HOST
#include "hk_fpred_core.h"

#include <cstdio>
#include <cstdlib>

static bool read_u32(FILE* f, unsigned& v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    v = b[0] | (b[1] << 8) | (b[2] << 16) | ((unsigned)b[3] << 24);
    return true;
}

template <int ES, typename T>
static void block_sums(const unsigned char* raw, unsigned bw, unsigned cspp, unsigned rows, unsigned cols, unsigned long long& s1,
                       unsigned long long& s2) {
    unsigned long long i = 0;
    for (unsigned r = 0; r < rows; ++r)
        for (unsigned c = 0; c < cspp; ++c) {
            T* dst = static_cast<T*>(malloc((size_t)cols * ES));
            hk::fpred::unpredict_row<ES, T>(raw + (size_t)r * bw * cspp * ES, (int)bw, (int)cspp, (int)c, (int)cols, dst);
            for (unsigned x = 0; x < cols; ++x)
                for (int k = 0; k < ES; ++k) {
                    const unsigned long long byte = (unsigned long long)(dst[x] >> (8 * k)) & 255u;
                    s1 += byte, s2 += ++i * byte;
                }
            free(dst);
        }
}

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s IN\n", argv[0]), 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return fprintf(stderr, "cannot open the file\n"), 2;
    unsigned n = 0;
    if (!read_u32(in, n)) return 2;
    for (unsigned i = 0; i < n; ++i) {
        unsigned es = 0, bw = 0, cspp = 0, rows = 0, cols = 0;
        if (!read_u32(in, es) || !read_u32(in, bw) || !read_u32(in, cspp) || !read_u32(in, rows) || !read_u32(in, cols))
            return fprintf(stderr, "block %u: short file\n", i), 2;
        if ((es != 4 && es != 8) || !bw || !cspp || !rows || !cols || cols > bw) return fprintf(stderr, "block %u: bad header\n", i), 2;
        const size_t bytes = (size_t)rows * bw * cspp * es;
        unsigned char* raw = static_cast<unsigned char*>(malloc(bytes));
        if (fread(raw, 1, bytes, in) != bytes) return fprintf(stderr, "block %u: short file\n", i), 2;
        unsigned long long s1 = 0, s2 = 0;
        if (es == 4) block_sums<4, unsigned>(raw, bw, cspp, rows, cols, s1, s2);
        else block_sums<8, unsigned long long>(raw, bw, cspp, rows, cols, s1, s2);
        printf("%llu %llu\n", s1, s2);
        free(raw);
    }
    fclose(in);
    return 0;
}
